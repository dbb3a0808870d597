#!/usr/bin/env python3
"""Measurements of the bidirectional call and the consistency kernel; prints
one JSON line (kept as profiles/bidir_probe.json, quoted in DESIGN.md).

(a) Two calls against one, 1920x1080 MEDIUM, 32 device-resident pairs: arm
    "two_calls" is calc_device(I0, I1) + calc_device(I1, I0) with graphs on
    (what a caller had before), arm "bidir" one calc_bidir_device. One context
    per arm in one process, the arms alternating round by round as tools/ab.py
    does; host clock around work that ends in a device synchronise.
(b) The check kernel on the 32 forward and 32 backward fields of (a), both
    directions per repetition, with and without err, timed with device events;
    GB/s by the bytes model 8 (fw) + 8 (bw, counted once) + 1 (mask) [+ 4 err]
    per pixel, and as a fraction of the copy bandwidth tools/bw measures on
    the same box in the same session (--bw-exe, a child process; build it with
    hipcc --offload-arch=gfx950 -O3 -o tools/bw tools/bw.hip -- without it the
    fraction is null)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import disflow  # noqa: E402
from disflow import boxstate  # noqa: E402


def spread(t):
    q = statistics.quantiles(t, n=4)
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "iqr_ms": round(q[2] - q[0], 4), "n": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--rounds", type=int, default=24, help="timed repetitions per arm (>= 20)")
    ap.add_argument("--steps", type=int, default=3, help="calls per repetition")
    ap.add_argument("--bw-exe", default=os.path.join(ROOT, "tools", "bw"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bidir_probe: no GPU (a measurement never falls back)")
    W, H, B = a.width, a.height, a.batch
    dev = torch.device("cuda", 0)
    out = {"probe": "bidir", "width": W, "height": H, "batch": B, "preset": a.preset, "rounds": a.rounds,
           "steps": a.steps, "device": torch.cuda.get_device_name(0)}

    copy_tbs = None
    if os.access(a.bw_exe, os.X_OK):  # before this process holds much memory
        r = subprocess.run([a.bw_exe], capture_output=True, text=True, timeout=120)
        m = re.search(r"^copy\s+[0-9.]+ ms\s+([0-9.]+) TB/s", r.stdout, re.M)
        if r.returncode == 0 and m:
            copy_tbs = float(m.group(1))
    out["copy_TBps"] = copy_tbs

    pairs = [disflow.synth_pair(k, W, H) for k in range(B)]
    d0 = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    d1 = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    p = disflow.preset_params(disflow.Preset[a.preset.upper()], W, H)
    eng2 = disflow.DenseInverseSearch(p, W, H, max_batch=B)
    eng1 = disflow.DenseInverseSearch(p, W, H, max_batch=B)
    eng2.set_graphs(True)
    f = [torch.empty((B, H, W, 2), dtype=torch.float32, device=dev) for _ in range(4)]
    s = torch.cuda.current_stream(dev).cuda_stream
    i0, i1 = d0.data_ptr(), d1.data_ptr()

    def two_calls():
        eng2.calc_device(B, i0, i1, f[0].data_ptr(), s)
        eng2.calc_device(B, i1, i0, f[1].data_ptr(), s)

    def bidir():
        eng1.calc_bidir_device(B, i0, i1, f[2].data_ptr(), f[3].data_ptr(), s)

    arms = (("two_calls", two_calls), ("bidir", bidir))
    times = {k: [] for k, _ in arms}
    sampler = boxstate.Sampler(boxstate.torch_hwmon_dir(0))
    for r in range(a.rounds + 2):  # two warm-up rounds (graph capture, code objects)
        for name, fn in arms:
            torch.cuda.synchronize()
            with sampler.phase(name if r >= 2 else "warmup"):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.steps * 1e3
            if r >= 2:
                times[name].append(dt)
    same = bool(torch.equal(f[0].view(torch.int32), f[2].view(torch.int32)) and
                torch.equal(f[1].view(torch.int32), f[3].view(torch.int32)))
    t2, t1 = statistics.median(times["two_calls"]), statistics.median(times["bidir"])
    out["a"] = {"two_calls": spread(times["two_calls"]), "bidir": spread(times["bidir"]),
                "bidir_over_two_calls": round(t1 / t2, 4), "same_bits": same,
                "pairs_per_s_two_calls": round(B / t2 * 1e3, 1), "pairs_per_s_bidir": round(B / t1 * 1e3, 1),
                "box": {k: sampler.summary(k) for k, _ in arms}}

    # (b) the check kernel, both directions per repetition
    mask = torch.empty((2, B, H, W), dtype=torch.uint8, device=dev)
    err = torch.empty((2, B, H, W), dtype=torch.float32, device=dev)
    fw, bw = f[2], f[3]
    px = B * H * W
    res = {}
    for label, with_err in (("mask_only", False), ("mask_and_err", True)):
        ts = []
        for r in range(a.rounds + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with sampler.phase("check_" + label if r >= 3 else "warmup"):
                e0.record()
                disflow.flow_consistency_device(fw.data_ptr(), bw.data_ptr(), B, W, H, mask[0].data_ptr(),
                                                err[0].data_ptr() if with_err else 0, stream=s)
                disflow.flow_consistency_device(bw.data_ptr(), fw.data_ptr(), B, W, H, mask[1].data_ptr(),
                                                err[1].data_ptr() if with_err else 0, stream=s)
                e1.record()
                e1.synchronize()
            if r >= 3:
                ts.append(e0.elapsed_time(e1))
        bytes_moved = 2 * px * (17 + (4 if with_err else 0))
        med = statistics.median(ts)
        gbs = bytes_moved / med / 1e6
        res[label] = dict(spread(ts), bytes=bytes_moved, GBps=round(gbs, 1),
                          fraction_of_copy=round(gbs / (copy_tbs * 1e3), 4) if copy_tbs else None,
                          box=sampler.summary("check_" + label))
    res["consistent_fraction_fw"] = round(float((mask[0] == 255).float().mean()), 4)
    out["b"] = res
    sampler.close()
    eng1.close()
    eng2.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
