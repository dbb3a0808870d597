#!/usr/bin/env python3
"""Timing of dis_flow_interp_u8 against two dis_flow_warp_u8
calls over the same images and against the box's copy bandwidth over a bytes
model: 32 device-resident single-channel 1920 x 1080 pairs (synthetic pairs 0-3
and their ground-truth flows, bw = -fw), t = 0.5, f32 and f16 flows, with bw
and without; HIP events around each call, medians after warm-up, one process.
Prints one JSON object; --out FILE also writes it; --quick: 3 repetitions (for
a run under a profiler: rocprofv3 --kernel-trace --stats gives the kernel
split). DISFLOW_LIB selects another build of the library."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd"))
import numpy as np
import torch
import disflow

quick = "--quick" in sys.argv
W, H, N = 1920, 1080, 32
REPS, WARM = (3, 1) if quick else (15, 3)
px = N * W * H
dev = "cuda:0"
pairs = [disflow.synth_pair(s, W, H, with_gt=True) for s in range(4)]
I0 = torch.from_numpy(np.stack([pairs[k % 4][0] for k in range(N)])).to(dev)
I1 = torch.from_numpy(np.stack([pairs[k % 4][1] for k in range(N)])).to(dev)
gt = np.stack([pairs[k % 4][2] for k in range(N)])
fw32 = torch.from_numpy(gt).to(dev)
bw32 = torch.from_numpy(-gt).to(dev)
fw16, bw16 = fw32.half(), bw32.half()
dst = torch.empty(px, dtype=torch.uint8, device=dev)
dst2 = torch.empty(px, dtype=torch.uint8, device=dev)
fill = torch.empty(px, dtype=torch.uint8, device=dev)
ws = torch.empty(px, dtype=torch.int64, device=dev)
torch.cuda.synchronize()

def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}

s = torch.cuda.current_stream().cuda_stream
out = {"W": W, "H": H, "n": N, "reps": REPS, "t": 0.5}
for name, fw, bw, dt in (("f32", fw32, bw32, np.float32), ("f16", fw16, bw16, np.float16)):
    for with_bw in (True, False):
        def run():
            disflow.flow_interp_device(I0.data_ptr(), I1.data_ptr(), fw.data_ptr(), dt, N, W, H, 1, 0.5, dst.data_ptr(),
                                       ws.data_ptr(), bw_ptr=bw.data_ptr() if with_bw else 0, fill_ptr=fill.data_ptr(), stream=s)
        out[f"interp_{name}_{'bw' if with_bw else 'nobw'}"] = timed(run)
    def warps():
        disflow.flow_warp_device(I0.data_ptr(), fw.data_ptr(), dt, N, W, H, 1, dst.data_ptr(), scale=-0.5, stream=s)
        disflow.flow_warp_device(I1.data_ptr(), fw.data_ptr(), dt, N, W, H, 1, dst2.data_ptr(), scale=0.5, stream=s)
    out[f"two_warps_{name}"] = timed(warps)
    fsz = 8 if name == "f32" else 4
    # bytes model: both frames in, fw read by the splat and gathered by the blend, bw read by the blend,
    # the workspace set, updated and read once each, dst and fill out
    for with_bw in (True, False):
        out[f"bytes_{name}_{'bw' if with_bw else 'nobw'}"] = px * (2 + 2 * fsz + (fsz if with_bw else 0) + 24 + 2)
    out[f"bytes_two_warps_{name}"] = px * (2 + 2 * fsz + 2)
torch.cuda.synchronize()
fills = fill.cpu().numpy()
out["sha_dst_fill_last"] = hashlib.sha256(dst.cpu().numpy().tobytes() + fills.tobytes()).hexdigest()[:16]
out["lib"] = os.environ.get("DISFLOW_LIB", "tree")
out["fill_fractions_last"] = [float((fills == c).mean()) for c in (0, 1, 2)]
src = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
dstc = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
c = timed(lambda: dstc.copy_(src))
out["copy_256MiB"] = c
out["copy_GBps_read_plus_write"] = 2 * (1 << 28) / (c["median_ms"] * 1e-3) / 1e9
ms = timed(lambda: ws.fill_(-1))
out["fill_workspace_531MB"] = ms
for k in list(out):
    if k.startswith("bytes_"):
        out["floor_ms_" + k[6:]] = out[k] / (out["copy_GBps_read_plus_write"] * 1e9) * 1e3
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
