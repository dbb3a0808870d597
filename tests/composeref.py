"""numpy float32 restatement of flow composition and point advection
(csrc/dis_compose.hip; dis_flow_compose and dis_flow_advect_points in
include/dis_abi.h): whole arrays, np.float32 throughout (never float64), one
separately rounded operation per numpy call, in the kernel's order -- so the
results agree bit for bit. The taps are tests/fbref.py's."""
import numpy as np

import fbref

F32 = np.float32

NAN32 = np.uint32(0x7fc00000)  # the canonical quiet NaN an invalid pixel gets
NAN16 = np.uint16(0x7e00)


def _ok(f):
    """|u| < 1e9 and |v| < 1e9 of (..., 2) vectors; False for NaN."""
    with np.errstate(invalid="ignore"):
        return (np.abs(f[..., 0]) < F32(1e9)) & (np.abs(f[..., 1]) < F32(1e9))


def _sample(b, mask_b, valid, ix0, ix1, iy0, iy1, a, bb):
    """Field b (H, W, 2) float32 sampled at fbref-style taps -> (ok, su, sv): ok
    where `valid` holds and all four tap vectors (and mask bytes) are good."""
    one = F32(1)
    ia, ib = one - a, one - bb
    w00, w01, w10, w11 = ia * ib, a * ib, ia * bb, a * bb
    assert all(w.dtype == F32 for w in (w00, w01, w10, w11))
    good = _ok(b)
    if mask_b is not None:
        good = good & (np.asarray(mask_b) != 0)
    ok = valid & good[iy0, ix0] & good[iy0, ix1] & good[iy1, ix0] & good[iy1, ix1]
    s = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(2):
            B = b[..., c]
            s.append(((w00 * B[iy0, ix0] + w01 * B[iy0, ix1]) + w10 * B[iy1, ix0]) + w11 * B[iy1, ix1])
    assert s[0].dtype == F32 and s[1].dtype == F32
    return ok, s[0], s[1]


def compose(a, b, valid_a=None, mask_b=None, out_dtype=np.float32):
    """(out, valid_out) of (H, W, 2) or (n, H, W, 2) fields a and b, float32 or
    float16 each (widened exactly, as the kernel does); valid_a, mask_b: u8
    (..., H, W) or None. out has out_dtype (float32 or float16)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.shape[-1] == 2
    assert a.dtype in (np.float32, np.float16) and b.dtype in (np.float32, np.float16)
    out_dtype = np.dtype(out_dtype)
    assert out_dtype in (np.float32, np.float16)
    if a.ndim == 4:
        res = [compose(a[k], b[k], None if valid_a is None else valid_a[k], None if mask_b is None else mask_b[k],
                       out_dtype) for k in range(len(a))]
        return np.stack([o for o, _ in res]), np.stack([v for _, v in res])
    fa, fb = a.astype(F32), b.astype(F32)  # exact for float16
    ok_a = _ok(fa)
    if valid_a is not None:
        ok_a = ok_a & (np.asarray(valid_a) != 0)
    # (an untrusted vector takes no part: zero keeps the tap arithmetic quiet)
    fa0 = np.where(ok_a[..., None], fa, F32(0))
    inside, ix0, ix1, iy0, iy1, wa, wb = fbref.taps(fa0)
    ok, su, sv = _sample(fb, mask_b, ok_a & inside, ix0, ix1, iy0, iy1, wa, wb)
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.stack([fa0[..., 0] + su, fa0[..., 1] + sv], axis=-1)
        assert o.dtype == F32
        o = o.astype(out_dtype)  # the engine's narrowing: round to nearest even
    if out_dtype == np.float32:
        bits = np.where(ok[..., None], o.view(np.uint32), NAN32)
        out = bits.astype(np.uint32).view(np.float32)
    else:
        bits = np.where(ok[..., None], o.view(np.uint16), NAN16)
        out = bits.astype(np.uint16).view(np.float16)
    return out, np.where(ok, 255, 0).astype(np.uint8)


def advect(points, flow):
    """(points_out, status) of points (count, 2) through flow (H, W, 2), or
    (n, count, 2) through (n, H, W, 2); flow float32 or float16. A point that
    does not move keeps its bits."""
    pts = np.ascontiguousarray(points, dtype=F32)
    flow = np.asarray(flow)
    assert flow.dtype in (np.float32, np.float16) and flow.shape[-1] == 2 and pts.shape[-1] == 2
    if flow.ndim == 4:
        assert pts.ndim == 3 and len(pts) == len(flow)
        res = [advect(p, f) for p, f in zip(pts, flow)]
        return np.stack([o for o, _ in res]), np.stack([s for _, s in res])
    assert pts.ndim == 2
    fl = flow.astype(F32)
    H, W = fl.shape[:2]
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore"):
        inside = (x >= F32(0)) & (x <= F32(W - 1)) & (y >= F32(0)) & (y <= F32(H - 1))  # False for NaN
    xs, ys = np.where(inside, x, F32(0)), np.where(inside, y, F32(0))
    x0, y0 = np.floor(xs), np.floor(ys)
    wa, wb = xs - x0, ys - y0
    ix0, iy0 = x0.astype(np.int64), y0.astype(np.int64)
    ix1, iy1 = np.minimum(ix0 + 1, W - 1), np.minimum(iy0 + 1, H - 1)
    ok, su, sv = _sample(fl, None, inside, ix0, ix1, iy0, iy1, wa, wb)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = np.stack([x + su, y + sv], axis=-1)
    assert moved.dtype == F32
    bits = np.where(ok[:, None], moved.view(np.uint32), pts.view(np.uint32))
    return bits.astype(np.uint32).view(np.float32), np.where(ok, 255, 0).astype(np.uint8)
