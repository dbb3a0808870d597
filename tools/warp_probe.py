#!/usr/bin/env python3
"""Measurements of the flow warp kernel (dis_flow_warp_u8); one process, one
JSON result (kept as profiles/warp_probe.json, quoted in DESIGN.md 3f).

64 device-resident 1920x1080 images of random bytes warped by 64 smooth fields
of up to +-6 px (a sinusoidal field per image, as the synthetic pairs move), with
valid written. Cases: 1 channel with f32 flow, 1 channel with f16 flow, 3 and 4
channels with f32 flow. Each case: warm-up launches, then --launches launches
timed one by one with events on the stream. The yardstick is measured in the
same process right before each case: a device-to-device copy that moves the
case's algorithmic bytes (flow read + one image read + image written + mask;
the copy reads half of them and writes half), timed the same way. Reported per
case: time per launch, GB/s by the algorithmic bytes, the copy's GB/s and the
fraction of it the kernel reaches. --aligned 0 offsets every buffer so that no
vector form applies (the scalar forms' price)."""
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
    ap.add_argument("--fields", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed launches per case (>= 30)")
    ap.add_argument("--aligned", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warp_probe: no GPU (a measurement never falls back)")
    W, H, n = a.width, a.height, a.fields
    dev = torch.device("cuda", 0)
    px = n * H * W
    lead = 0 if a.aligned else 1
    s = torch.cuda.current_stream(dev).cuda_stream

    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    flow32 = torch.zeros(2 * lead + 2 * px, dtype=torch.float32, device=dev)[2 * lead:]
    f = flow32.view(n, H, W, 2)
    f[..., 0] = 6.0 * torch.sin(x / 50.0 + y / 90.0 + k)
    f[..., 1] = 6.0 * torch.cos(y / 40.0 - x / 120.0 + k)
    flow16 = torch.zeros(2 * lead + 2 * px, dtype=torch.float16, device=dev)[2 * lead:]
    flow16.copy_(flow32)
    del x, y, k, f
    valid = torch.zeros(lead + px, dtype=torch.uint8, device=dev)[lead:]

    out = {"probe": "warp", "width": W, "height": H, "fields": n, "launches": a.launches, "aligned": bool(a.aligned),
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for C, dtype in ((1, np.float32), (1, np.float16), (3, np.float32), (4, np.float32)):
        flow = flow32 if dtype == np.float32 else flow16
        src = torch.randint(0, 256, (lead + px * C,), dtype=torch.uint8, device=dev)[lead:]
        dst = torch.zeros(lead + px * C, dtype=torch.uint8, device=dev)[lead:]
        nbytes = px * (2 * flow.element_size() + 2 * C + 1)
        ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
        del ca, cb
        t = timed(lambda: disflow.flow_warp_device(src.data_ptr(), flow.data_ptr(), dtype, n, W, H, C, dst.data_ptr(),
                                                   valid.data_ptr(), stream=s), a.warmup, a.launches)
        gbs = nbytes / statistics.fmean(t) / 1e6
        copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
        out["cases"][f"c{C}_{np.dtype(dtype).name}"] = dict(
            spread(t), bytes=nbytes, bytes_per_pixel=nbytes // px, GBps=round(gbs, 1), copy=spread(t_copy),
            copy_GBps=round(copy_gbs, 1), fraction_of_copy=round(gbs / copy_gbs, 4),
            valid_fraction=round(float((valid == 255).float().mean()), 4))
        del src, dst
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
