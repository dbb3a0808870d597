#!/usr/bin/env python3
"""Measurements of the 4:2:0 conversion kernels (dis_yuv.hip;
dis_yuv420_to_frames_u8 and dis_frames_to_yuv420_u8); one process, one JSON
result (kept as profiles/yuv_probe.json, quoted in DESIGN.md 3n).

64 device-resident 1920x1080 surfaces, one launch a call, timed one by one with
events on the stream. Cases: both directions x the surface layouts (NV12 from an
aligned base: the vector forms; NV12 from a base one byte in: the surface side
byte by byte; I420: planar chroma) x the frame formats BGR8 and BGRA8.
  copy: the yardstick, measured in the same process the same way: a
        device-to-device copy that moves the kernel's read + write byte total
        (it reads half of them and writes half).
Reported: time, GB/s by the algorithmic bytes (W*H*(3/2 + channels) per
surface), the copy's GB/s and the fraction of it the kernel reaches."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd"))
import torch  # noqa: E402

import disflow  # noqa: E402

CHANNELS = {"bgr": 3, "bgra": 4}


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
    ap.add_argument("--surfaces", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed launches per case (>= 30)")
    ap.add_argument("--matrix", default="bt709")
    ap.add_argument("--range", default="limited")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_probe: no GPU (a measurement never falls back)")
    W, H, n = a.width, a.height, a.surfaces
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    img = W * H * 3 // 2
    out = {"probe": "yuv", "width": W, "height": H, "surfaces": n, "launches": a.launches, "matrix": a.matrix,
           "range": a.range, "device": torch.cuda.get_device_name(0), "cases": {}}

    surf = torch.randint(0, 256, (n * img + 16,), dtype=torch.uint8, device=dev)
    for fmt, C in CHANNELS.items():
        frames = torch.randint(0, 256, (n * H * W * C,), dtype=torch.uint8, device=dev)
        nbytes = n * W * H * C + n * img
        ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
        del ca, cb
        copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
        for layout, lead, planar in (("nv12", 0, False), ("nv12_offset", 1, False), ("i420", 0, True)):
            y = surf.data_ptr() + lead
            c0 = y + W * H
            c1 = c0 + ((W // 2) * (H // 2) if planar else 1)
            step, cst = (1, W // 2) if planar else (2, W)
            kw = dict(y_stride=W, y_image_stride=img, c_stride=cst, c_image_stride=img, stream=s)

            def to_frames():
                disflow.yuv420_to_frames_device(y, c0, c1, step, n, W, H, frames.data_ptr(), fmt, a.matrix, a.range,
                                                255, **kw)

            def from_frames():
                disflow.frames_to_yuv420_device(frames.data_ptr(), fmt, n, W, H, y, c0, c1, step, a.matrix, a.range,
                                                **kw)
            # (from_frames last: it overwrites the random surfaces, which the timing does not depend on)
            for name, fn in (("to_frames", to_frames), ("from_frames", from_frames)):
                t = timed(fn, a.warmup, a.launches)
                gbs = nbytes / statistics.fmean(t) / 1e6
                out["cases"][f"{name}_{layout}_{fmt}"] = dict(spread(t), bytes=nbytes, GBps=round(gbs, 1),
                                                              copy=spread(t_copy), copy_GBps=round(copy_gbs, 1),
                                                              fraction_of_copy=round(gbs / copy_gbs, 4))
        del frames
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
