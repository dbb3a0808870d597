#!/usr/bin/env python3
"""Measurements of the luma kernel (dis_luma.hip; dis_frames_to_gray_u8 and the
front stage of a colour context); one process, one JSON result (kept as
profiles/luma_probe.json, quoted in DESIGN.md 3h).

The 64 device-resident 1920x1080 BGR frames of a 32-pair MEDIUM step. Cases:
  engine:     the step itself with kernel timing on, dis_kernel_time class 7 (the
              luma launches of the step: one per sub-batch, both frames of its
              pairs), summed per step; next to class 0 (the pyramid) of the same steps;
  standalone: dis_frames_to_gray_u8 on the same 64 frames as one launch, per
              format, timed one by one with events on the stream;
  copy:       the yardstick, measured in the same process the same way: a
              device-to-device copy that moves the kernel's read + write byte
              total (it reads half of them and writes half).
Reported: time, GB/s by the algorithmic bytes (W*H*(channels + 1) per frame), the
copy's GB/s and the fraction of it the kernel reaches. --aligned 0 offsets the
source by one byte, so that the general (byte by byte) path runs."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd"))
import torch  # noqa: E402

import disflow  # noqa: E402

CHANNELS = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "gray": 1}


def spread(t):
    q = statistics.quantiles(t, n=4)
    return {"mean_ms": round(statistics.fmean(t), 4), "median_ms": round(statistics.median(t), 4),
            "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "iqr_ms": round(q[2] - q[0], 4), "n": len(t)}


def timed(fn, warmup, launches):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed launches / steps per case (>= 30)")
    ap.add_argument("--aligned", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "luma_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("luma_probe: no GPU (a measurement never falls back)")
    W, H, B = a.width, a.height, a.pairs
    n = 2 * B
    dev = torch.device("cuda", 0)
    px = n * H * W
    lead = 0 if a.aligned else 1
    s = torch.cuda.current_stream(dev).cuda_stream
    out = {"probe": "luma", "width": W, "height": H, "frames": n, "launches": a.launches, "aligned": bool(a.aligned),
           "device": torch.cuda.get_device_name(0), "cases": {}}

    gray = torch.zeros(px, dtype=torch.uint8, device=dev)
    for fmt in ("bgr", "bgra", "gray"):
        C = CHANNELS[fmt]
        src = torch.randint(0, 256, (lead + px * C,), dtype=torch.uint8, device=dev)[lead:]
        nbytes = px * (C + 1)
        ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
        del ca, cb
        t = timed(lambda: disflow.frames_to_gray_device(src.data_ptr(), fmt, n, W, H, gray.data_ptr(), stream=s),
                  a.warmup, a.launches)
        gbs = nbytes / statistics.fmean(t) / 1e6
        copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
        out["cases"][f"standalone_{fmt}"] = dict(spread(t), bytes=nbytes, GBps=round(gbs, 1), copy=spread(t_copy),
                                                 copy_GBps=round(copy_gbs, 1), fraction_of_copy=round(gbs / copy_gbs, 4))
        if fmt == "bgr":
            keep = src
        else:
            del src

    # the engine's own launches: a 32-pair MEDIUM step on the BGR frames, kernel timing on
    p = disflow.preset_params(disflow.Preset.MEDIUM, W, H)
    eng = disflow.DenseInverseSearch(p, W, H, max_batch=B, frame_format="bgr")
    flow = torch.empty((B, H, W, 2), dtype=torch.float32, device=dev)
    fb = W * H * 3
    i0, i1 = keep.data_ptr(), keep.data_ptr() + B * fb
    for _ in range(a.warmup):
        eng.calc_device(B, i0, i1, flow.data_ptr(), s)
    torch.cuda.synchronize()
    eng.set_kernel_timing(True)
    for _ in range(a.launches):
        eng.calc_device(B, i0, i1, flow.data_ptr(), s)
    torch.cuda.synchronize()
    ln, lms = eng.kernel_time(disflow.KERNEL_LUMA)
    pn, pms = eng.kernel_time(disflow.KERNEL_PYRAMID)
    eng.set_kernel_timing(False)
    eng.close()
    nbytes = px * 4
    out["cases"]["engine_bgr"] = dict(steps=a.launches, luma_launches=ln, luma_ms_per_step=round(lms / a.launches, 4),
                                      pyramid_launches=pn, pyramid_ms_per_step=round(pms / a.launches, 4), bytes=nbytes,
                                      GBps=round(nbytes / (lms / a.launches) / 1e6, 1))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
