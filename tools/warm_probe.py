#!/usr/bin/env python3
"""Measurements of the temporal warm start; prints one JSON line (kept as
profiles/warm_probe.json, quoted in DESIGN.md "Temporal warm start").

(a) The init launch (k_flow_to_init) at 1920x1080 MEDIUM, batch 1 and 32, by
    the kernel-timing id KERNEL_INIT: time per launch and GB/s by the bytes it
    reads (8 * W * H * n), as a fraction of the copy bandwidth tools/bw
    measures on the same box in the same session (--bw-exe, a child process;
    build it with hipcc --offload-arch=gfx950 -O3 -o tools/bw tools/bw.hip --
    without it the fraction is null).
(b) The warm call against the plain call, both eager (set_graphs(0)), batch 1
    and 32: one context per arm in one process, the arms alternating round by
    round as tools/ab.py does; host clock around work that ends in a device
    synchronise.
(c) A shallower pyramid: batch 1, device-resident frames of a synthetic
    sequence (one texture moving by --motion pixels per frame). Arm "cold" is
    the preset's C with graphs on (what a caller has today), arm "warm" is
    C - 3 started from the previous pair's flow; latency per pair (each call
    followed by a synchronise) and the mean end-point distance of each arm,
    and of a cold C - 3 run, from the cold full-pyramid flow.
(d) DIS_PRECISION_FMA against DIS_PRECISION_EXACT on the 128x96 shifted pair of
    tests/test_gpu_warmstart.py (C = 1), warm (init = the true flow) and cold:
    mean and p99.9 end-point distance."""
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


def spread(t):
    q = statistics.quantiles(t, n=4)
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "iqr_ms": round(q[2] - q[0], 4), "n": len(t)}


def alternate(arms, rounds, steps, sync_each=False):
    """arms: (name, fn) pairs run alternately; ms per call per round."""
    times = {k: [] for k, _ in arms}
    for r in range(rounds + 2):  # two warm-up rounds
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
                if sync_each:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
    return times


def epe(a, b):
    d = (a.double() - b.double())
    return float(torch.sqrt((d * d).sum(-1)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--motion", type=int, nargs=2, default=(5, -3))
    ap.add_argument("--bw-exe", default=os.path.join(ROOT, "tools", "bw"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warm_probe: no GPU (a measurement never falls back)")
    W, H = a.width, a.height
    dev = torch.device("cuda", 0)
    out = {"probe": "warm", "width": W, "height": H, "preset": a.preset, "rounds": a.rounds, "steps": a.steps,
           "device": torch.cuda.get_device_name(0)}

    copy_tbs = None
    if os.access(a.bw_exe, os.X_OK):  # before this process holds much memory
        r = subprocess.run([a.bw_exe], capture_output=True, text=True, timeout=120)
        m = re.search(r"^copy\s+[0-9.]+ ms\s+([0-9.]+) TB/s", r.stdout, re.M)
        if r.returncode == 0 and m:
            copy_tbs = float(m.group(1))
    out["copy_TBps"] = copy_tbs

    p = disflow.preset_params(disflow.Preset[a.preset.upper()], W, H)
    out["coarsest_scale"] = p.coarsest_scale
    s = torch.cuda.current_stream(dev).cuda_stream
    B = 32
    pairs = [disflow.synth_pair(k, W, H) for k in range(B)]
    d0 = torch.from_numpy(np.stack([q[0] for q in pairs])).to(dev)
    d1 = torch.from_numpy(np.stack([q[1] for q in pairs])).to(dev)
    i0, i1 = d0.data_ptr(), d1.data_ptr()
    plain = disflow.DenseInverseSearch(p, W, H, max_batch=B)
    warm = disflow.DenseInverseSearch(p, W, H, max_batch=B)
    plain.set_graphs(False)
    warm.set_graphs(False)
    prior = torch.empty((B, H, W, 2), dtype=torch.float32, device=dev)
    f_plain = torch.empty_like(prior)
    f_warm = torch.empty_like(prior)
    plain.calc_device(B, i0, i1, prior.data_ptr(), s)
    torch.cuda.synchronize()

    # (a) the init launch
    res_a = {}
    for n in (1, B):
        warm.set_kernel_timing(True)
        for _ in range(a.rounds + 3):
            warm.calc_device(n, i0, i1, f_warm.data_ptr(), s, init_ptr=prior.data_ptr())
        torch.cuda.synchronize()
        launches, ms = warm.kernel_time(disflow.KERNEL_INIT)
        warm.set_kernel_timing(False)
        per = ms / launches
        gbs = 8.0 * W * H * n / per / 1e6
        res_a[f"batch_{n}"] = {"launches": launches, "mean_us": round(per * 1e3, 2), "bytes": 8 * W * H * n,
                               "GBps": round(gbs, 1),
                               "fraction_of_copy": round(gbs / (copy_tbs * 1e3), 4) if copy_tbs else None}
    out["a"] = res_a

    # (b) warm call against plain call, both eager
    res_b = {}
    for n in (1, B):
        arms = (("plain", lambda: plain.calc_device(n, i0, i1, f_plain.data_ptr(), s)),
                ("warm", lambda: warm.calc_device(n, i0, i1, f_warm.data_ptr(), s, init_ptr=prior.data_ptr())))
        t = alternate(arms, a.rounds, a.steps)
        mp, mw = statistics.median(t["plain"]), statistics.median(t["warm"])
        res_b[f"batch_{n}"] = {"plain": spread(t["plain"]), "warm": spread(t["warm"]),
                               "warm_minus_plain_us": round((mw - mp) * 1e3, 2), "warm_over_plain": round(mw / mp, 4)}
    out["b"] = res_b
    plain.close()
    warm.close()
    del d0, d1, prior, f_plain, f_warm

    # (c) a shallower pyramid, batch 1
    mx, my = a.motion
    nf = 5
    T = disflow.synth_pair(900, W + abs(mx) * nf + 8, H + abs(my) * nf + 8)[0]
    frames = []
    for k in range(nf):  # the texture moves by (mx, my) per frame: frame k shows T shifted
        x0 = (abs(mx) * nf if mx > 0 else 0) - mx * k + 4 * (mx <= 0)
        y0 = (abs(my) * nf if my > 0 else 0) - my * k + 4 * (my <= 0)
        frames.append(torch.from_numpy(np.ascontiguousarray(T[y0:y0 + H, x0:x0 + W])).to(dev))
    ps = disflow.Params(**{**p.__dict__, "coarsest_scale": max(p.coarsest_scale - 3, p.finest_scale)})
    deep = disflow.DenseInverseSearch(p, W, H)
    shallow = disflow.DenseInverseSearch(ps, W, H)
    fd = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
    fs = torch.empty_like(fd)
    fc = torch.empty_like(fd)
    k0 = nf - 2  # the timed pair; the pairs before it warm the flow up
    for k in range(k0):
        shallow.calc_device(1, frames[k].data_ptr(), frames[k + 1].data_ptr(), fs.data_ptr(), s,
                            init_ptr=fs.data_ptr() if k else 0)
    torch.cuda.synchronize()
    seed = fs.clone()  # the previous pair's flow: every timed warm call starts from it
    a0, a1 = frames[k0].data_ptr(), frames[k0 + 1].data_ptr()
    arms = (("cold", lambda: deep.calc_device(1, a0, a1, fd.data_ptr(), s)),
            ("warm", lambda: shallow.calc_device(1, a0, a1, fs.data_ptr(), s, init_ptr=seed.data_ptr())))
    t = alternate(arms, a.rounds, a.steps, sync_each=True)
    shallow.calc_device(1, a0, a1, fc.data_ptr(), s)
    torch.cuda.synchronize()
    truth = torch.tensor([float(mx), float(my)], device=dev).expand(H, W, 2)
    mc, mw = statistics.median(t["cold"]), statistics.median(t["warm"])
    out["c"] = {"motion": [mx, my], "C_cold": p.coarsest_scale, "C_warm": ps.coarsest_scale,
                "cold": spread(t["cold"]), "warm": spread(t["warm"]), "warm_over_cold": round(mw / mc, 4),
                "epe_warm_vs_cold_full": round(epe(fs, fd), 5), "epe_cold_shallow_vs_cold_full": round(epe(fc, fd), 5),
                "epe_cold_full_vs_true_motion": round(epe(fd, truth), 5),
                "epe_warm_vs_true_motion": round(epe(fs, truth), 5),
                "epe_cold_shallow_vs_true_motion": round(epe(fc, truth), 5)}
    deep.close()
    shallow.close()

    # (d) FMA against exact on the tests' shifted pair
    Tt = disflow.synth_pair(7, 160, 120)[0]
    vx, vy = 16, -12
    I0 = np.ascontiguousarray(Tt[4:100, 24:152])
    I1 = np.ascontiguousarray(Tt[4 - vy:100 - vy, 24 - vx:152 - vx])
    truth = np.broadcast_to(np.array((vx, vy), np.float32), (96, 128, 2))
    pe = disflow.Params(coarsest_scale=1, finest_scale=0, patch_size=8, iterations=12, patch_overlap=0.5)
    eng = disflow.DenseInverseSearch(pe, 128, 96)
    res_d = {}
    for label, init in (("warm", truth), ("cold", None)):
        eng.set_precision(disflow.PRECISION_EXACT)
        ex = eng.calc(I0, I1, init=init)
        eng.set_precision(disflow.PRECISION_FMA)
        fm = eng.calc(I0, I1, init=init)
        d = np.sqrt(((fm.astype(np.float64) - ex) ** 2).sum(-1))
        res_d[label] = {"mean_epe": float(d.mean()), "p999_epe": float(np.quantile(d, 0.999)), "max_epe": float(d.max())}
    eng.close()
    out["d"] = res_d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
