"""dis_motion_stabilize and dis_warp_motion_u8 (include/dis_abi.h) restated:
the path math in Python floats (IEEE doubles, one rounding per operation) in
the contract's order; the warp as warpref.warp of motionref.to_flow's field
plus the rule for models that are not finite; and the block routes of
csrc/dis_warpmotion.hip (staged / direct, and the pixels of staged blocks that
read global memory) from the same float32 operations as the kernel's decision.
The tests compare with all of it bit for bit."""
import math

import numpy as np

import motionref
import warpref

F32 = np.float32
TILE_W, TILE_H, STAGE_DWORDS = 64, 16, 4096


def _mul(a, b):
    """a . b of 2 x 3 matrices (six floats, row-major), the contract's order."""
    r = [0.0] * 6
    for i in range(2):
        a0, a1, a2 = a[3 * i], a[3 * i + 1], a[3 * i + 2]
        r[3 * i] = a0 * b[0] + a1 * b[3]
        r[3 * i + 1] = a0 * b[1] + a1 * b[4]
        r[3 * i + 2] = (a0 * b[2] + a1 * b[5]) + a2
    return r


def path(pair_params):
    """(the matrices C_0 .. C_{N-1}, the number of replaced models)."""
    p = np.asarray(pair_params, np.float32).reshape(-1, 6)
    C = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]]
    bad = 0
    for q in p:
        if np.isfinite(q).all():
            f = [float(v) for v in q]
            A = [1.0 + f[1], f[2], f[0], f[4], 1.0 + f[5], f[3]]
        else:
            A = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            bad += 1
        C.append(_mul(A, C[-1]))
    return C, bad


def weights(sigma, count):
    s = float(F32(sigma))
    s2 = 2.0 * s * s
    return [float(F32(math.exp(-(float(d) * d) / s2))) for d in range(count)]


def smooth(C, radius, sigma):
    n = len(C)
    reach = min(radius, n - 1)
    g = weights(sigma, reach + 1)
    S = []
    for k in range(n):
        s, wsum = [0.0] * 6, 0.0
        for j in range(max(0, k - reach), min(n - 1, k + reach) + 1):
            w = g[abs(j - k)]
            for e in range(6):
                s[e] = s[e] + w * C[j][e]
            wsum = wsum + w
        with np.errstate(all="ignore"):
            S.append([float(np.float64(v) / np.float64(wsum)) for v in s])
    return S


def invert(s):
    with np.errstate(all="ignore"):
        d = np.float64
        det = float(d(s[0]) * d(s[4]) - d(s[1]) * d(s[3]))
        if not math.isfinite(det) or abs(det) <= 2.0 ** -20:
            return None
        i00, i01, i10, i11 = s[4] / det, -s[1] / det, -s[3] / det, s[0] / det
        i02 = float(-(d(i00) * d(s[2]) + d(i01) * d(s[5])))
        i12 = float(-(d(i10) * d(s[2]) + d(i11) * d(s[5])))
    return [i00, i01, i02, i10, i11, i12]


def stabilize(pair_params, width, height, radius, sigma=None, zoom=1.0):
    """disflow.stabilize_path(..., with_status=True): corrections float32 (N, 6),
    status u8 (N,), replaced."""
    if sigma is None:
        sigma = max(radius, 1) / 2.0
    C, bad = path(pair_params)
    S = smooth(C, radius, sigma)
    z = 1.0 / float(F32(zoom))
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    Z = [z, 0.0, cx * (1.0 - z), 0.0, z, cy * (1.0 - z)]
    out = np.zeros((len(C), 6), np.float32)
    status = np.zeros(len(C), np.uint8)
    for k, (c, s) in enumerate(zip(C, S)):
        inv = invert(s)
        if inv is None:
            continue
        with np.errstate(all="ignore"):
            m = [float(v) for v in _mul(_mul([np.float64(v) for v in c], [np.float64(v) for v in inv]),
                                        [np.float64(v) for v in Z])]
            q = np.array([m[2], m[0] - 1.0, m[1], m[5], m[3], m[4] - 1.0], np.float64).astype(np.float32)
        if np.isfinite(q).all():
            out[k] = q
            status[k] = 1
    return out, status, bad


def matrix(q):
    """The 3 x 3 float64 matrix of a model's six parameters."""
    q = np.asarray(q, np.float64)
    return np.array([[1 + q[1], q[2], q[0]], [q[4], 1 + q[5], q[3]], [0, 0, 1]])


def warp(image, params, border=warpref.REPLICATE):
    """disflow.warp_motion(..., return_valid=True): (dst, valid)."""
    image = np.asarray(image)
    p = np.asarray(params, np.float32)
    if p.ndim == 1:
        H, W = image.shape[:2]
        return warpref.warp(image, motionref.to_flow(p, W, H), 1.0, border)
    H, W = image.shape[1:3]
    out = [warpref.warp(i, motionref.to_flow(q, W, H), 1.0, border) for i, q in zip(image, p)]
    return np.stack([d for d, _ in out]), np.stack([m for _, m in out])


def routes(params, width, height, channels, border=warpref.REPLICATE):
    """(staged blocks, direct blocks, pixels of staged blocks that read global
    memory) of dis_warp_motion_u8's launch over the models (n, 6): the block's
    decision of k_warp_motion in the same float32 operations. Only the
    3-channel kernel stages; 1 and 4 channels run the direct form everywhere."""
    W, H, C = width, height, channels
    staged = direct = lane = 0
    one, two, zero = F32(1), F32(2), F32(0)
    xm, ym = F32(W - 1), F32(H - 1)
    for p in np.asarray(params, np.float32).reshape(-1, 6):
        finite = bool(np.isfinite(p).all())
        fl = motionref.to_flow(p, W, H)
        with np.errstate(all="ignore"):
            ok = (np.abs(fl[..., 0]) < F32(1e9)) & (np.abs(fl[..., 1]) < F32(1e9))
            px = np.arange(W, dtype=F32)[None, :] + fl[..., 0]
            py = np.arange(H, dtype=F32)[:, None] + fl[..., 1]
        inside = ok & (px >= zero) & (px <= xm) & (py >= zero) & (py <= ym)
        reads = ok & (inside | (border == warpref.REPLICATE))  # pixels that form tap indices
        cpx = np.minimum(np.maximum(px, zero), xm)
        cpy = np.minimum(np.maximum(py, zero), ym)
        for Y0 in range(0, H, TILE_H):
            for X0 in range(0, W, TILE_W):
                X1, Y1 = min(X0 + TILE_W - 1, W - 1), min(Y0 + TILE_H - 1, H - 1)
                cs = [(Y0, X0), (Y0, X1), (Y1, X0), (Y1, X1)]
                if C != 3 or not finite or not all(ok[c] for c in cs):
                    direct += 1
                    continue
                lox, hix = min(px[c] for c in cs), max(px[c] for c in cs)
                loy, hiy = min(py[c] for c in cs), max(py[c] for c in cs)
                bx0 = int(min(max(np.floor(lox) - one, zero), xm))
                bx1 = int(min(min(max(np.floor(hix), zero), xm) + two, xm))
                by0 = int(min(max(np.floor(loy) - one, zero), ym))
                by1 = int(min(min(max(np.floor(hiy), zero), ym) + two, ym))
                be, bo = (bx1 + 1) * C, (bx0 * C) & ~3
                pitch = ((be - bo + 3) >> 2) | 1
                if pitch * (by1 - by0 + 1) > STAGE_DWORDS:
                    direct += 1
                    continue
                staged += 1
                t = (slice(Y0, Y1 + 1), slice(X0, X1 + 1))
                with np.errstate(invalid="ignore"):
                    ix0 = np.floor(cpx[t]).astype(np.int64)
                    iy0 = np.floor(cpy[t]).astype(np.int64)
                ix1, iy1 = np.minimum(ix0 + 1, W - 1), np.minimum(iy0 + 1, H - 1)
                inbox = (ix0 >= bx0) & (ix1 <= bx1) & (iy0 >= by0) & (iy1 <= by1)
                lane += int((reads[t] & ~inbox).sum())
    return staged, direct, lane
