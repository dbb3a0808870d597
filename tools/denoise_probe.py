#!/usr/bin/env python3
"""Measurements of temporal denoising (dis_temporal_denoise_u8); one process,
one JSON result (profiles/denoise_probe.json; quoted in DESIGN.md 3l).

32 device-resident single-channel 1920x1080 frames with K = 2 and K = 4
neighbours each: the frame moved by a few pixels with fresh noise, and flows
that point back with sub-pixel jitter. Cases: f32 and f16 flows at both K, with
support. Each case: warm-up calls, then --launches calls timed one by one with
events on the stream. Yardsticks, measured in the same process right before
each case and timed the same way: the same images through K dis_flow_warp_u8
calls (what the interface offered before; it writes K warped stacks and still
lacks the blend), and a device-to-device copy that moves the bytes the call
must move (cur, K neighbours, K flows in; dst and support out; half of them
read, half written). Reported per case: the call's time, the K warps' time, the
bytes, the GB/s, the copy's GB/s and the fraction of it the call reaches."""
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed calls per case (>= 30)")
    ap.add_argument("--sigma", type=float, default=12.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_probe: no GPU (a measurement never falls back)")
    W, H, n, KMAX = a.width, a.height, a.frames, 4
    dev = torch.device("cuda", 0)
    px = n * H * W
    s = torch.cuda.current_stream(dev).cuda_stream
    table = disflow.denoise_weights(a.sigma)

    torch.manual_seed(11)
    four = [disflow.synth_pair(k, W, H)[0] for k in range(4)]
    base = torch.from_numpy(np.stack([four[k % 4] for k in range(n)])).to(dev)
    noisy = lambda t: (t.float() + 8.0 * torch.randn(t.shape, device=dev)).round().clamp(0, 255).to(torch.uint8)  # noqa: E731
    cur = noisy(base)
    shifts = [(3, 1), (-3, -1), (6, 2), (-6, -2)]
    nbs = [noisy(torch.roll(base, (dy, dx), (1, 2))) for dx, dy in shifts]
    f32 = []
    for dx, dy in shifts:
        f = torch.empty(n, H, W, 2, dtype=torch.float32, device=dev)
        f[..., 0], f[..., 1] = float(dx), float(dy)
        f += 0.3 * torch.randn_like(f)
        f32.append(f)
    flows = {np.float32: f32, np.float16: [f.to(torch.float16) for f in f32]}
    del base
    dst = torch.zeros(px, dtype=torch.uint8, device=dev)
    sup = torch.zeros(px, dtype=torch.uint8, device=dev)
    warped = [torch.zeros(px, dtype=torch.uint8, device=dev) for _ in range(KMAX)]
    valid = [torch.zeros(px, dtype=torch.uint8, device=dev) for _ in range(KMAX)]

    res = {"probe": "denoise", "width": W, "height": H, "frames": n, "channels": 1, "launches": a.launches,
           "sigma": a.sigma, "device": torch.cuda.get_device_name(0), "cases": {}}
    for dtype in (np.float32, np.float16):
        for K in (2, 4):
            fl = flows[dtype][:K]
            nbytes = px * (1 + K + 2 * K * fl[0].element_size() + 2)  # cur, neighbours, flows; dst, support
            ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
            del ca, cb

            def call():
                disflow.temporal_denoise_device(cur.data_ptr(), [t.data_ptr() for t in nbs[:K]],
                                                [t.data_ptr() for t in fl], dtype, n, W, H, 1, dst.data_ptr(),
                                                weights=table, support_ptr=sup.data_ptr(), stream=s)

            def warps():
                for k in range(K):
                    disflow.flow_warp_device(nbs[k].data_ptr(), fl[k].data_ptr(), dtype, n, W, H, 1, warped[k].data_ptr(),
                                             valid_ptr=valid[k].data_ptr(), stream=s)
            t_warp = timed(warps, a.warmup, a.launches)
            t_call = timed(call, a.warmup, a.launches)
            torch.cuda.synchronize()
            ms = statistics.fmean(t_call)
            gbs = nbytes / ms / 1e6
            copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
            diff = (dst.float() - cur.reshape(-1).float()).abs().mean().item()
            res["cases"][f"{np.dtype(dtype).name}_K{K}"] = dict(
                call=spread(t_call), warps=spread(t_warp), warps_over_call=round(statistics.fmean(t_warp) / ms, 3),
                bytes=nbytes, bytes_per_pixel=round(nbytes / px, 2), call_GBps=round(gbs, 1), copy=spread(t_copy),
                copy_GBps=round(copy_gbs, 1), fraction_of_copy=round(gbs / copy_gbs, 4),
                mean_support=round(sup.float().mean().item(), 3), mean_abs_change=round(diff, 3))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
