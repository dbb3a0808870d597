"""numpy float32 restatement of the backward warp (csrc/dis_warp.hip,
dis_flow_warp_u8 in include/dis_abi.h): whole arrays, np.float32 throughout
(never float64), one separately rounded operation per numpy call, in the
kernel's order -- so the results agree bit for bit. The sampler is
tests/fbref.py's (same taps, weights and order of sums), applied to bytes."""
import numpy as np

F32 = np.float32

REPLICATE, ZERO = 0, 1


def warp(image, flow, scale=1.0, border=REPLICATE):
    """(dst u8, valid u8) of image (H, W), (H, W, C), (n, H, W) or (n, H, W, C)
    warped by flow (H, W, 2) or (n, H, W, 2), float32 or float16 (widened
    exactly, as the kernel does). A 3-D image is (H, W, C) when its leading
    dimensions are the flow's (H, W), else (n, H, W)."""
    image = np.asarray(image)
    flow = np.asarray(flow)
    assert image.dtype == np.uint8 and flow.dtype in (np.float32, np.float16) and flow.shape[-1] == 2
    fl = flow.astype(F32)  # exact for float16
    H, W = fl.shape[-3:-1]
    if fl.ndim == 4 or (image.ndim == 3 and image.shape[:2] != (H, W)):
        fl4 = fl if fl.ndim == 4 else fl[None]
        assert len(image) == len(fl4)
        out = [warp(i, f, scale, border) for i, f in zip(image, fl4)]
        return np.stack([d for d, _ in out]), np.stack([m for _, m in out]).reshape(flow.shape[:-1])
    img = image.reshape(H, W, -1)
    u, v = fl[..., 0], fl[..., 1]
    sc = F32(scale)
    x = np.arange(W, dtype=F32)[None, :]
    y = np.arange(H, dtype=F32)[:, None]
    xm, ym, zero, one = F32(W - 1), F32(H - 1), F32(0), F32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(u) < F32(1e9)) & (np.abs(v) < F32(1e9))  # False for NaN
        us = np.where(ok, u, zero)
        vs = np.where(ok, v, zero)
        su = sc * us
        sv = sc * vs
        px = x + su
        py = y + sv
    assert px.dtype == F32 and py.dtype == F32
    inside = ok & (px >= zero) & (px <= xm) & (py >= zero) & (py <= ym)
    px = np.minimum(np.maximum(px, zero), xm)
    py = np.minimum(np.maximum(py, zero), ym)
    x0 = np.floor(px)
    y0 = np.floor(py)
    a = px - x0
    b = py - y0
    ix0 = x0.astype(np.int64)
    iy0 = y0.astype(np.int64)
    ix1 = np.minimum(ix0 + 1, W - 1)
    iy1 = np.minimum(iy0 + 1, H - 1)
    ia, ib = one - a, one - b
    w00, w01, w10, w11 = ia * ib, a * ib, ia * b, a * b
    assert all(w.dtype == F32 for w in (w00, w01, w10, w11))
    dst = np.empty(img.shape, np.uint8)
    written = ok if border == REPLICATE else inside
    for c in range(img.shape[2]):
        P = img[..., c].astype(F32)
        s = ((w00 * P[iy0, ix0] + w01 * P[iy0, ix1]) + w10 * P[iy1, ix0]) + w11 * P[iy1, ix1]
        assert s.dtype == F32
        r = np.minimum(np.maximum(np.rint(s), zero), F32(255))
        dst[..., c] = np.where(written, r, zero).astype(np.uint8)
    valid = np.where(inside, 255, 0).astype(np.uint8)
    return dst.reshape(image.shape), valid
