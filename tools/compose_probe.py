#!/usr/bin/env python3
"""Measurements of the flow composition and point advection kernels
(dis_flow_compose, dis_flow_advect_points); one process, one JSON result (kept
as profiles/compose_probe.json, quoted in DESIGN.md 3i).

32 device-resident 1920x1080 fields a and b, smooth and of up to +-6 px (a
sinusoidal field per pair, as the synthetic pairs move). Cases: f32/f32 -> f32
and f16/f16 -> f32, each without the byte planes and with all three (valid_a
and mask_b about a fifth zeros, valid_out written). Each case: warm-up
launches, then --launches launches timed one by one with events on the stream.
The yardstick is measured in the same process right before each case: a
device-to-device copy that moves the case's algorithmic bytes (a read once, b
read once, out written, the planes read or written once; the copy reads half
of them and writes half), timed the same way. Reported per case: time per
launch, GB/s by the algorithmic bytes, the copy's GB/s and the fraction of it
the kernel reaches. Then the advection of 32 x 10,000 points through the f32
and the f16 fields (time per launch only: 0.6 MB of points is a launch, not a
stream). --aligned 0 offsets every buffer so that no vector form applies (the
scalar forms' price)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import disflow  # noqa: E402


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
    ap.add_argument("--fields", type=int, default=32)
    ap.add_argument("--points", type=int, default=10000, help="points per field of the advection case")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed launches per case (>= 30)")
    ap.add_argument("--aligned", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compose_probe: no GPU (a measurement never falls back)")
    W, H, n = a.width, a.height, a.fields
    dev = torch.device("cuda", 0)
    px = n * H * W
    lead = 0 if a.aligned else 1
    s = torch.cuda.current_stream(dev).cuda_stream

    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    fields = {}
    for name, ph in (("a", 0.0), ("b", 1.3)):
        f32 = torch.zeros(2 * lead + 2 * px, dtype=torch.float32, device=dev)[2 * lead:]
        f = f32.view(n, H, W, 2)
        f[..., 0] = 6.0 * torch.sin(x / 50.0 + y / 90.0 + k + ph)
        f[..., 1] = 6.0 * torch.cos(y / 40.0 - x / 120.0 + k + ph)
        f16 = torch.zeros(2 * lead + 2 * px, dtype=torch.float16, device=dev)[2 * lead:]
        f16.copy_(f32)
        fields[name] = {np.float32: f32, np.float16: f16}
    del x, y, k, f
    planes = []
    for _ in range(2):
        p = torch.zeros(lead + px, dtype=torch.uint8, device=dev)[lead:]
        p.copy_(torch.where(torch.rand(px, device=dev) < 0.2, 0, 255).to(torch.uint8))
        planes.append(p)
    valid_a, mask_b = planes
    valid_out = torch.zeros(lead + px, dtype=torch.uint8, device=dev)[lead:]
    out = torch.zeros(2 * lead + 2 * px, dtype=torch.float32, device=dev)[2 * lead:]

    res = {"probe": "compose", "width": W, "height": H, "fields": n, "launches": a.launches, "aligned": bool(a.aligned),
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for dtype in (np.float32, np.float16):
        fa, fb = fields["a"][dtype], fields["b"][dtype]
        for with_planes in (False, True):
            nbytes = px * (2 * 2 * fa.element_size() + 8 + (3 if with_planes else 0))
            ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
            del ca, cb
            t = timed(lambda: disflow.flow_compose_device(
                fa.data_ptr(), dtype, fb.data_ptr(), dtype, n, W, H, out.data_ptr(), out_dtype=np.float32,
                valid_a_ptr=valid_a.data_ptr() if with_planes else 0, mask_b_ptr=mask_b.data_ptr() if with_planes else 0,
                valid_out_ptr=valid_out.data_ptr() if with_planes else 0, stream=s), a.warmup, a.launches)
            gbs = nbytes / statistics.fmean(t) / 1e6
            copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
            name = f"{np.dtype(dtype).name}_{'planes' if with_planes else 'plain'}"
            res["cases"][name] = dict(
                spread(t), bytes=nbytes, bytes_per_pixel=nbytes // px, GBps=round(gbs, 1), copy=spread(t_copy),
                copy_GBps=round(copy_gbs, 1), fraction_of_copy=round(gbs / copy_gbs, 4),
                valid_fraction=round(float((out.view(-1, 2)[:, 0] == out.view(-1, 2)[:, 0]).float().mean()), 4))
    cnt = a.points
    pts = torch.zeros(2 * lead + 2 * n * cnt, dtype=torch.float32, device=dev)[2 * lead:]
    v = pts.view(n, cnt, 2)
    v[..., 0] = torch.rand(n, cnt, device=dev) * (W - 1)
    v[..., 1] = torch.rand(n, cnt, device=dev) * (H - 1)
    pout = torch.zeros(2 * lead + 2 * n * cnt, dtype=torch.float32, device=dev)[2 * lead:]
    status = torch.zeros(lead + n * cnt, dtype=torch.uint8, device=dev)[lead:]
    for dtype in (np.float32, np.float16):
        fb = fields["b"][dtype]
        t = timed(lambda: disflow.advect_points_device(fb.data_ptr(), dtype, n, W, H, pts.data_ptr(), cnt,
                                                       pout.data_ptr(), status_ptr=status.data_ptr(), stream=s),
                  a.warmup, a.launches)
        res["cases"][f"advect_{np.dtype(dtype).name}"] = dict(
            spread(t), points=n * cnt, moved_fraction=round(float((status == 255).float().mean()), 4))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
