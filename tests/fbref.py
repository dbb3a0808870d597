"""numpy float32 restatement of the forward-backward consistency check
(csrc/dis_consistency.hip, DESIGN.md "Bidirectional flow"): whole arrays,
np.float32 throughout (never float64), one separately rounded operation per
numpy call, in the kernel's order -- so the results agree bit for bit."""
import numpy as np

F32 = np.float32


def taps(fw):
    """Tap indices and validity of one (H, W, 2) forward field: (valid, ix0, ix1,
    iy0, iy1, a, b); indices are 0 where the target leaves the frame."""
    fw = np.asarray(fw, F32)
    H, W = fw.shape[:2]
    u, v = fw[..., 0], fw[..., 1]
    x = np.arange(W, dtype=F32)[None, :]
    y = np.arange(H, dtype=F32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        px = x + u
        py = y + v
        valid = (px >= F32(0)) & (px <= F32(W - 1)) & (py >= F32(0)) & (py <= F32(H - 1))  # False for NaN
    pxs = np.where(valid, px, F32(0))
    pys = np.where(valid, py, F32(0))
    x0 = np.floor(pxs)
    y0 = np.floor(pys)
    a = pxs - x0
    b = pys - y0
    ix0 = x0.astype(np.int64)
    iy0 = y0.astype(np.int64)
    ix1 = np.minimum(ix0 + 1, W - 1)
    iy1 = np.minimum(iy0 + 1, H - 1)
    return valid, ix0, ix1, iy0, iy1, a, b


def check(fw, bw, alpha1=0.01, alpha2=0.5):
    """(mask u8, err f32) of (H, W, 2) or (n, H, W, 2) fields."""
    fw = np.asarray(fw, F32)
    bw = np.asarray(bw, F32)
    assert fw.shape == bw.shape and fw.shape[-1] == 2
    if fw.ndim == 4:
        out = [check(f, b, alpha1, alpha2) for f, b in zip(fw, bw)]
        return np.stack([m for m, _ in out]), np.stack([e for _, e in out])
    a1, a2 = F32(alpha1), F32(alpha2)
    u, v = fw[..., 0], fw[..., 1]
    valid, ix0, ix1, iy0, iy1, a, b = taps(fw)
    one = F32(1)
    ia, ib = one - a, one - b
    w00, w01, w10, w11 = ia * ib, a * ib, ia * b, a * b
    assert all(w.dtype == F32 for w in (w00, w01, w10, w11))
    with np.errstate(invalid="ignore", over="ignore"):
        s = []
        for c in range(2):
            B = bw[..., c]
            s.append(((w00 * B[iy0, ix0] + w01 * B[iy0, ix1]) + w10 * B[iy1, ix0]) + w11 * B[iy1, ix1])
        su, sv = s
        dx, dy = u + su, v + sv
        err = dx * dx + dy * dy
        thr = a1 * ((u * u + v * v) + (su * su + sv * sv)) + a2
        ok = valid & (err <= thr)
    assert err.dtype == F32 and thr.dtype == F32
    mask = np.where(ok, 255, 0).astype(np.uint8)
    err = np.where(valid, err, F32(np.inf)).astype(F32)
    return mask, err
