#!/usr/bin/env python3
"""Measurements of the homography family (dis_flow_fit_homography,
dis_warp_homography_u8); one process, one JSON result
(profiles/homography_probe.json; quoted in DESIGN.md 3o).

Fit: 32 device-resident 1920x1080 fields, a homography per field with 0.15 px
of noise, a block moving on its own and 4 % random vectors, as f32 and f16,
without a mask. Each case: warm-up calls, then --launches calls with iterations
= 0 and as many with iterations = 3, timed one by one with events on the stream;
the time of a pass is the difference of the two means divided by 3. Beside it,
in the same process and timed the same way: dis_flow_fit_motion's affine fit of
the same fields, and a device-to-device copy that moves the bytes a pass reads.
Reported: the pass times, their ratio, and the fraction of the copy's GB/s.

Warp: 64 device-resident 1920x1080 images of 1, 3 and 4 channels, one mild
homography per image. dis_warp_homography_u8 beside dis_warp_motion_u8 (the
models' affine parts), beside the chain dis_homography_to_flow +
dis_flow_warp_u8, and beside a copy of the bytes the warp reads and writes."""
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


def fit_part(a, dev, s):
    W, H, n = a.width, a.height, a.fields
    px = n * H * W
    torch.manual_seed(7)
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    f32 = torch.zeros(2 * px, dtype=torch.float32, device=dev)
    f = f32.view(n, H, W, 2)
    g = (1e-5 + 1e-7 * k) * x - 6e-6 * y
    f[..., 0] = ((3.25 - 0.1 * k) + 0.004 * x - 0.002 * y - x * g) / (1 + g)
    f[..., 1] = ((-1.5 + 0.05 * k) + 0.003 * x + 0.005 * y - y * g) / (1 + g)
    f += 0.15 * torch.randn_like(f)
    f[:, H // 4:H // 4 + H // 3, W // 8:W // 8 + (3 * W) // 8] += torch.tensor([9.0, -7.0], device=dev)
    wild = torch.rand(n, H, W, device=dev) < 0.04
    f[wild] = 40.0 * torch.rand(int(wild.sum()), 2, device=dev) - 20.0
    fields = {np.float32: f32, np.float16: f32.to(torch.float16)}
    del x, y, k, f, g, wild
    params = torch.zeros(8 * n, dtype=torch.float32, device=dev)
    info = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(disflow.fit_homography_workspace(n, W, H), disflow.fit_motion_workspace(n, W, H)), dtype=torch.uint8,
                     device=dev)
    out = {}
    for dtype in (np.float32, np.float16):
        fl = fields[dtype]
        nbytes = px * 2 * fl.element_size()  # what one pass reads
        ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
        del ca, cb

        def hom(its):
            disflow.fit_homography_device(fl.data_ptr(), dtype, n, W, H, params.data_ptr(), ws.data_ptr(), iterations=its,
                                          threshold=1.0, info_ptr=info.data_ptr(), stream=s)

        def aff(its):
            disflow.fit_motion_device(fl.data_ptr(), dtype, n, W, H, params.data_ptr(), ws.data_ptr(), model="affine",
                                      iterations=its, threshold=1.0, info_ptr=info.data_ptr(), stream=s)
        a0, a3 = timed(lambda: aff(0), a.warmup, a.launches), timed(lambda: aff(3), a.warmup, a.launches)
        h0, h3 = timed(lambda: hom(0), a.warmup, a.launches), timed(lambda: hom(3), a.warmup, a.launches)
        torch.cuda.synchronize()
        inf = info.cpu().numpy().view(np.uint32).reshape(n, 4)
        hp = (statistics.fmean(h3) - statistics.fmean(h0)) / 3.0
        apass = (statistics.fmean(a3) - statistics.fmean(a0)) / 3.0
        copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
        out[np.dtype(dtype).name] = dict(
            homography_iterations0=spread(h0), homography_iterations3=spread(h3), affine_iterations0=spread(a0),
            affine_iterations3=spread(a3), homography_pass_ms=round(hp, 4), affine_pass_ms=round(apass, 4),
            first_pass_ratio=round(statistics.fmean(h0) / statistics.fmean(a0), 3), refit_pass_ratio=round(hp / apass, 3),
            bytes_per_pass=nbytes, copy=spread(t_copy), copy_GBps=round(copy_gbs, 1),
            homography_fraction_of_copy=round(nbytes / hp / 1e6 / copy_gbs, 4),
            affine_fraction_of_copy=round(nbytes / apass / 1e6 / copy_gbs, 4),
            fitted_fields=int(inf[:, 0].sum()), mean_fitted_share=round(float((inf[:, 2] / inf[:, 1]).mean()), 4))
    return out


def warp_part(a, dev, s):
    W, H, n = a.width, a.height, a.images
    px = n * H * W
    rng = np.random.default_rng(5)
    p8 = np.zeros((n, 8), np.float32)
    p8[:, :6] = rng.normal(0, 1, (n, 6)) * [3, 0.004, 0.004, 3, 0.004, 0.004]
    p8[:, 6:] = rng.normal(0, 5e-6, (n, 2))
    d8 = torch.from_numpy(p8).to(dev)
    d6 = torch.from_numpy(np.ascontiguousarray(p8[:, :6])).to(dev)
    field = torch.empty(2 * px, dtype=torch.float32, device=dev)
    out = {}
    for C in (1, 3, 4):
        src = torch.randint(0, 256, (px * C,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ca, cb = torch.empty(px * C, dtype=torch.uint8, device=dev), torch.empty(px * C, dtype=torch.uint8, device=dev)
        t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)

        def hom():
            disflow.warp_homography_device(src.data_ptr(), d8.data_ptr(), n, W, H, C, dst.data_ptr(), stream=s)

        def aff():
            disflow.warp_motion_device(src.data_ptr(), d6.data_ptr(), n, W, H, C, dst.data_ptr(), stream=s)

        def chain():
            disflow.homography_to_flow_device(d8.data_ptr(), n, W, H, field.data_ptr(), stream=s)
            disflow.flow_warp_device(src.data_ptr(), field.data_ptr(), np.float32, n, W, H, C, dst.data_ptr(), stream=s)
        th, ta, tc = (timed(fn, a.warmup, a.launches) for fn in (hom, aff, chain))
        mh, ma, mc = statistics.fmean(th), statistics.fmean(ta), statistics.fmean(tc)
        out[f"{C}ch"] = dict(warp_homography=spread(th), warp_motion=spread(ta), chain=spread(tc), copy=spread(t_copy),
                             against_warp_motion=round(mh / ma, 3), chain_over_warp=round(mc / mh, 3),
                             fraction_of_copy=round(statistics.fmean(t_copy) / mh, 4))
        del src, dst, ca, cb
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--fields", type=int, default=32)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed calls per case (>= 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_probe: no GPU (a measurement never falls back)")
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    res = {"probe": "homography", "width": a.width, "height": a.height, "fields": a.fields, "images": a.images,
           "launches": a.launches, "device": torch.cuda.get_device_name(0)}
    res["fit"] = fit_part(a, dev, s)
    res["warp"] = warp_part(a, dev, s)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
