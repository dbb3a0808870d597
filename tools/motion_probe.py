#!/usr/bin/env python3
"""Measurements of the global-motion fit (dis_flow_fit_motion); one process, one
JSON result (profiles/motion_probe.json; quoted in DESIGN.md 3k).

32 device-resident 1920x1080 fields: an affine motion per field with 0.15 px of
noise, a block of an eighth of the frame moving on its own and 4 % random
vectors. Cases: f32 and f16 fields, each without and with a mask of about a
fifth zeros; the affine model. Each case: warm-up calls, then --launches calls
with iterations = 0 (one pass: two launches) and as many with iterations = 3
(four passes), timed one by one with events on the stream. The time of a pass
is the difference of the two means divided by 3. A pass reads every vector and
mask byte once and writes next to nothing, so the yardstick, measured in the
same process right before each case and timed the same way, is a
device-to-device copy that moves the same bytes (half of them read, half
written). Reported per case: the time per call, the time per pass, the GB/s of
a pass, the copy's GB/s and the fraction of it the pass reaches; and the same
for a call with the inlier plane."""
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed calls per case and iteration count (>= 30)")
    ap.add_argument("--model", default="affine")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("motion_probe: no GPU (a measurement never falls back)")
    W, H, n = a.width, a.height, a.fields
    dev = torch.device("cuda", 0)
    px = n * H * W
    s = torch.cuda.current_stream(dev).cuda_stream

    torch.manual_seed(7)
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    f32 = torch.zeros(2 * px, dtype=torch.float32, device=dev)
    f = f32.view(n, H, W, 2)
    f[..., 0] = (3.25 - 0.1 * k) + 0.004 * x - 0.002 * y
    f[..., 1] = (-1.5 + 0.05 * k) + 0.003 * x + 0.005 * y
    f += 0.15 * torch.randn_like(f)
    f[:, H // 4:H // 4 + H // 3, W // 8:W // 8 + (3 * W) // 8] += torch.tensor([9.0, -7.0], device=dev)
    wild = torch.rand(n, H, W, device=dev) < 0.04
    f[wild] = 40.0 * torch.rand(int(wild.sum()), 2, device=dev) - 20.0
    f16 = f32.to(torch.float16)
    fields = {np.float32: f32, np.float16: f16}
    del x, y, k, f, wild
    mask = torch.where(torch.rand(px, device=dev) < 0.2, 0, 255).to(torch.uint8)
    inliers = torch.zeros(px, dtype=torch.uint8, device=dev)
    params = torch.zeros(6 * n, dtype=torch.float32, device=dev)
    info = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    ws_bytes = disflow.fit_motion_workspace(n, W, H)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)

    res = {"probe": "motion", "width": W, "height": H, "fields": n, "launches": a.launches, "model": a.model,
           "device": torch.cuda.get_device_name(0), "workspace_bytes": ws_bytes, "cases": {}}
    for dtype in (np.float32, np.float16):
        fl = fields[dtype]
        for with_mask in (False, True):
            nbytes = px * (2 * fl.element_size() + (1 if with_mask else 0))  # what one pass reads
            ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
            del ca, cb

            def call(its, with_inliers=False):
                disflow.fit_motion_device(fl.data_ptr(), dtype, n, W, H, params.data_ptr(), ws.data_ptr(), model=a.model,
                                          iterations=its, threshold=1.0, mask_ptr=mask.data_ptr() if with_mask else 0,
                                          info_ptr=info.data_ptr(), inliers_ptr=inliers.data_ptr() if with_inliers else 0,
                                          stream=s)
            t0 = timed(lambda: call(0), a.warmup, a.launches)
            t3 = timed(lambda: call(3), a.warmup, a.launches)
            t3i = timed(lambda: call(3, True), a.warmup, a.launches)
            torch.cuda.synchronize()
            inf = info.cpu().numpy().view(np.uint32).reshape(n, 4)
            pass_ms = (statistics.fmean(t3) - statistics.fmean(t0)) / 3.0
            gbs = nbytes / pass_ms / 1e6
            copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
            name = f"{np.dtype(dtype).name}_{'mask' if with_mask else 'plain'}"
            res["cases"][name] = dict(
                iterations0=spread(t0), iterations3=spread(t3), iterations3_inliers=spread(t3i),
                pass_ms=round(pass_ms, 4), inlier_pass_ms=round(statistics.fmean(t3i) - statistics.fmean(t3), 4),
                bytes_per_pass=nbytes, bytes_per_pixel=round(nbytes / px, 2), pass_GBps=round(gbs, 1), copy=spread(t_copy),
                copy_GBps=round(copy_gbs, 1), fraction_of_copy=round(gbs / copy_gbs, 4),
                fitted_fields=int(inf[:, 0].sum()), mean_fitted_share=round(float((inf[:, 2] / inf[:, 1]).mean()), 4),
                mean_agree_share=round(float((inf[:, 3] / inf[:, 1]).mean()), 4))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
