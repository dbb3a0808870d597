"""numpy restatement of motion-compensated temporal denoising
(csrc/dis_denoise.hip, dis_temporal_denoise_u8 in include/dis_abi.h), built on
tests/warpref.py: whole arrays, integers exact, np.float32 throughout (never
float64), one separately rounded operation per numpy call, in the kernel's
order -- so the results agree bit for bit."""
import numpy as np

import warpref

F32 = np.float32
MAX_NEIGHBOURS = 8


def weights(sigma):
    """dis_denoise_weights: exp(-d^2 / (2 sigma^2)) in double, rounded once."""
    s = float(F32(sigma))
    d = np.arange(256, dtype=np.float64)
    return np.exp(-(d * d) / (2.0 * s * s)).astype(F32)


def _window_sum(a):
    """(H, W) integers -> the sum over each pixel's 3 x 3 window, clamped to the frame."""
    p = np.pad(a, 1, mode="edge")
    H, W = a.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def denoise(cur, neighbours, flows, table, masks=None):
    """(dst u8, support u8) of cur (H, W), (H, W, C), (n, H, W) or (n, H, W, C) and
    K neighbours of its shape, K flows (H, W, 2) or (n, H, W, 2) of one dtype
    (float32 or float16), a float32 (256,) table and masks None or K entries,
    each None or u8 (..., H, W). A 3-D image is (H, W, C) when its leading
    dimensions are the flow's (H, W), else (n, H, W), as warpref.warp's."""
    cur = np.asarray(cur)
    table = np.asarray(table)
    K = len(neighbours)
    assert 1 <= K <= MAX_NEIGHBOURS and len(flows) == K and (masks is None or len(masks) == K)
    assert cur.dtype == np.uint8 and table.dtype == F32 and table.shape == (256,)
    fshape = np.asarray(flows[0]).shape
    H, W = fshape[-3:-1]
    n = fshape[0] if len(fshape) == 4 else 1
    c4 = cur.reshape(n, H, W, -1)
    C = c4.shape[3]
    cnt = 9 * C
    ci = c4.astype(np.int64)
    cf = c4.astype(F32)
    num = np.zeros(c4.shape, F32)
    sw = np.zeros((n, H, W), F32)
    support = np.zeros((n, H, W), np.uint8)
    for k in range(K):
        nb = np.asarray(neighbours[k])
        assert nb.shape == cur.shape and nb.dtype == np.uint8 and np.asarray(flows[k]).shape == fshape
        wk, vk = warpref.warp(nb.reshape(n, H, W, C), np.asarray(flows[k]).reshape(n, H, W, 2), 1.0, warpref.REPLICATE)
        wi = wk.reshape(n, H, W, C).astype(np.int64)
        ok = vk.reshape(n, H, W) != 0
        if masks is not None and masks[k] is not None:
            ok &= np.asarray(masks[k]).reshape(n, H, W) != 0
        ad = np.abs(wi - ci).sum(axis=3)
        D = np.stack([_window_sum(ad[i]) for i in range(n)])
        idx = (D + cnt // 2) // cnt
        assert idx.min() >= 0 and idx.max() <= 255
        w = np.where(ok, table[idx], F32(0))
        assert w.dtype == F32
        diff = (wi - ci).astype(F32)  # exact
        t = w[..., None] * diff
        num = num + t
        sw = sw + w
        support += (ok & (w > 0)).astype(np.uint8)
        assert t.dtype == F32 and num.dtype == F32 and sw.dtype == F32
    den = F32(1) + sw
    q = num / den[..., None]
    r = cf + q
    assert den.dtype == F32 and q.dtype == F32 and r.dtype == F32
    dst = np.minimum(np.maximum(np.rint(r), F32(0)), F32(255)).astype(np.uint8)
    return dst.reshape(cur.shape), support.reshape(fshape[:-1])


def psnr(a, b):
    """PSNR in dB of two u8 arrays."""
    e = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if e == 0 else 10.0 * np.log10(255.0 ** 2 / e)
