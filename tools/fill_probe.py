#!/usr/bin/env python3
"""Measurements of the push-pull fill (dis_flow_fill); one process, one JSON
result (profiles/fill_probe.json, and fill_probe_offset.json for --aligned 0;
quoted in DESIGN.md 3j).

32 device-resident 1920x1080 fields, smooth and of up to +-6 px (a sinusoidal
field per pair, as the synthetic pairs move), with a mask of about a fifth
zeros. Cases: f32 -> f32 and f16 -> f32, each without and with the level map.
Each case: warm-up calls, then --launches calls (three launches each) timed one
by one with events on the stream. The yardstick is measured in the same
process right before each case: a device-to-device copy that moves the case's
bytes by the three stages' model (pull: field and mask read, levels 1..5
written, 8 * 0.333 B a pixel; top: nothing to speak of; push: field and mask
read again, levels 1..5 read, out written, level written: about 33 B a pixel
for f32 -> f32), timed the same way. Reported per case: time per call, GB/s by
the model, the copy's GB/s and the fraction of it the fill reaches. --aligned 0
offsets every buffer so that no vector form applies.

The time of each stage is not taken here (the entry point is one call): it
comes from a kernel trace of this probe in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/fill_probe.py --quality 0;
profiles/fill_kernel_stats.txt). bench.py --full's hbm_measured_peak of the
same box stands beside this probe's copy figure in DESIGN.md 3j.

Then, for the record (--quality 1): the error of the filled vectors on a smooth
160x120 field (20 % random holes, a 40 x 30 hole, a 10-column border strip),
and the valid share of the field accumulated over a 160x120 value-noise
sequence with and without the fill after each composition."""
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


def quality():
    """Host arrays through flow_fill: the smooth-field error and the accumulated
    field's valid share with and without the fill."""
    W, H = 160, 120
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    truth = np.stack([6 * np.sin(x / 50 + y / 90), 6 * np.cos(y / 40 - x / 120)], -1).astype(np.float32)
    rng = np.random.default_rng(5)
    mask = np.where(rng.random((H, W)) < 0.2, 0, 255).astype(np.uint8)
    mask[45:75, 60:100] = 0
    mask[:, :10] = 0
    out, level = disflow.flow_fill(truth, mask, with_level=True)
    hole = mask == 0
    err = np.sqrt(((out - truth) ** 2).sum(-1))[hole]
    res = {"smooth_field": {"holes": int(hole.sum()), "mean_err_px": round(float(err.mean()), 4),
                            "max_err_px": round(float(err.max()), 4), "max_level": int(level.max())}}
    # the value-noise sequence: content moving by whole pixels, pair flows chained
    margin, moves = 8, [(0, 0), (3, 1), (5, -1), (6, 1), (8, 2), (7, 0)]
    big, _ = disflow.synth_pair(11, W + 2 * margin, H + 2 * margin)
    frames = [np.ascontiguousarray(big[margin - dy:margin - dy + H, margin - dx:margin - dx + W]) for dx, dy in moves]
    eng = disflow.DenseInverseSearch(disflow.Params(3, 1, 8, 25, 0.625, 1), W, H)
    flows = [eng.calc(a, b) for a, b in zip(frames, frames[1:])]
    eng.close()
    shares = {"plain": [], "filled": []}
    for name in shares:
        acc, valid = flows[0], np.full((H, W), 255, np.uint8)
        for f in flows[1:]:
            acc, valid = disflow.flow_compose(acc, f, valid_a=valid, with_valid=True)
            shares[name].append(round(float((valid == 255).mean()), 4))
            if name == "filled":
                acc, valid = disflow.flow_fill(acc, valid), np.full((H, W), 255, np.uint8)
    res["accumulated_valid_share"] = shares
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--fields", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40, help="timed calls per case (>= 30)")
    ap.add_argument("--aligned", type=int, default=1)
    ap.add_argument("--quality", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fill_probe: no GPU (a measurement never falls back)")
    W, H, n = a.width, a.height, a.fields
    dev = torch.device("cuda", 0)
    px = n * H * W
    lead = 0 if a.aligned else 1
    s = torch.cuda.current_stream(dev).cuda_stream

    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    f32 = torch.zeros(2 * lead + 2 * px, dtype=torch.float32, device=dev)[2 * lead:]
    f = f32.view(n, H, W, 2)
    f[..., 0] = 6.0 * torch.sin(x / 50.0 + y / 90.0 + k)
    f[..., 1] = 6.0 * torch.cos(y / 40.0 - x / 120.0 + k)
    f16 = torch.zeros(2 * lead + 2 * px, dtype=torch.float16, device=dev)[2 * lead:]
    f16.copy_(f32)
    fields = {np.float32: f32, np.float16: f16}
    del x, y, k, f
    mask = torch.zeros(lead + px, dtype=torch.uint8, device=dev)[lead:]
    mask.copy_(torch.where(torch.rand(px, device=dev) < 0.2, 0, 255).to(torch.uint8))
    level = torch.zeros(lead + px, dtype=torch.uint8, device=dev)[lead:]
    out = torch.zeros(2 * lead + 2 * px, dtype=torch.float32, device=dev)[2 * lead:]
    ws_bytes = disflow.flow_fill_workspace(n, W, H)
    ws = torch.zeros(8 * lead + ws_bytes, dtype=torch.uint8, device=dev)[8 * lead:]
    cells15 = sum(((W + (1 << l) - 1) >> l) * ((H + (1 << l) - 1) >> l) for l in range(1, 6)) * n

    res = {"probe": "fill", "width": W, "height": H, "fields": n, "launches": a.launches, "aligned": bool(a.aligned),
           "device": torch.cuda.get_device_name(0), "workspace_bytes": ws_bytes, "cases": {}}
    for dtype in (np.float32, np.float16):
        fl = fields[dtype]
        for with_level in (False, True):
            # pull: field + mask in, levels 1..5 out; push: field + mask + levels 1..5 in, out (+ level) out
            nbytes = px * (2 * (2 * fl.element_size() + 1) + 8 + (1 if with_level else 0)) + 2 * 8 * cells15
            ca, cb = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            t_copy = timed(lambda: cb.copy_(ca), a.warmup, a.launches)
            del ca, cb
            t = timed(lambda: disflow.flow_fill_device(
                fl.data_ptr(), dtype, n, W, H, out.data_ptr(), ws.data_ptr(), out_dtype=np.float32,
                mask_ptr=mask.data_ptr(), level_ptr=level.data_ptr() if with_level else 0, stream=s), a.warmup, a.launches)
            gbs = nbytes / statistics.fmean(t) / 1e6
            copy_gbs = 2 * (nbytes // 2) / statistics.fmean(t_copy) / 1e6
            name = f"{np.dtype(dtype).name}_{'level' if with_level else 'plain'}"
            res["cases"][name] = dict(
                spread(t), bytes=nbytes, bytes_per_pixel=round(nbytes / px, 2), GBps=round(gbs, 1), copy=spread(t_copy),
                copy_GBps=round(copy_gbs, 1), fraction_of_copy=round(gbs / copy_gbs, 4),
                time_over_model=round(statistics.fmean(t) / statistics.fmean(t_copy), 3),
                nan_left=int((out != out).sum()))
    if a.quality:
        res["quality"] = quality()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
