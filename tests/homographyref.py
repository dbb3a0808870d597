"""The homography family of include/dis_abi.h restated in numpy, operation for
operation: dis_flow_fit_homography (float64 sums in the contract's order --
slots of a chunk, adjacent pairs, chunks in turn -- and the 8 x 8 LDL^T solve
in Python floats, one rounding per operation), dis_homography_to_flow (float32),
dis_warp_homography_u8 (warpref.warp of that field) and
dis_homography_stabilize (Python floats). The GPU tests compare with it bit for
bit."""
import math

import numpy as np

import motionref
import warpref
from motionref import CHUNK, SLOTS, STEPS, NAN32, NAN16, chunks, trusted, ldl_solve
from stabref import weights

TERMS = 27
F32 = np.float32


def workspace_bytes(n, width, height):
    return n * (chunks(width, height) * TERMS + 16) * 8


def scale(width, height):
    """The smallest power of two >= max(W, H, 2) / 2."""
    m, s = max(width, height, 2), 1
    while 2 * s < m:
        s *= 2
    return s


def _coords(width, height):
    """(a, b): the centred coordinates scaled by 1 / s, per pixel, row-major."""
    s = float(scale(width, height))
    q = np.arange(width * height)
    a = ((q % width).astype(np.float64) - (width - 1) / 2.0) / s
    b = ((q // width).astype(np.float64) - (height - 1) / 2.0) / s
    return a, b


def _uv(flow, width, height):
    s = float(scale(width, height))
    f = np.asarray(flow).astype(np.float32)
    return f[..., 0].reshape(-1).astype(np.float64) / s, f[..., 1].reshape(-1).astype(np.float64) / s


def terms(flow):
    """(27, W*H): the terms of every pixel of one (H, W, 2) field."""
    H, W = np.asarray(flow).shape[:2]
    a, b = _coords(W, H)
    U, V = _uv(flow, W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        A, B = a + U, b + V
        aa, ab, bb = a * a, a * b, b * b
        aA, bA, aB, bB = a * A, b * A, a * B, b * B
        Q = A * A + B * B
        return np.stack([np.ones(W * H), a, b, aa, ab, bb,
                         aA, bA, aa * A, ab * A, bb * A,
                         aB, bB, aa * B, ab * B, bb * B,
                         aa * Q, ab * Q, bb * Q,
                         U, a * U, b * U, V, a * V, b * V,
                         aA * U + aB * V, bA * U + bB * V])


def sums(flow, member, T=None):
    """The 27 sums of one field over the pixels of `member` (H, W) bool, in the
    contract's order."""
    H, W = member.shape
    n = W * H
    T = terms(flow) if T is None else T
    T = np.where(member.reshape(-1)[None, :], T, 0.0)  # a select: no other pixel's vector enters a sum
    nch = chunks(W, H)
    P = np.zeros((TERMS, nch * CHUNK))
    P[:, :n] = T
    P = P.reshape(TERMS, nch, STEPS, SLOTS)
    acc = np.zeros((TERMS, nch, SLOTS))
    for k in range(STEPS):
        acc = acc + P[:, :, k, :]
    while acc.shape[2] > 1:
        acc = acc[:, :, 0::2] + acc[:, :, 1::2]
    acc = acc[:, :, 0]
    tot = np.zeros(TERMS)
    for c in range(nch):
        tot = tot + acc[:, c]
    return [float(t) for t in tot]


def normal_system(S):
    """(N 8 x 8 as lists, r) of the 27 sums."""
    N = [[0.0] * 8 for _ in range(8)]
    G = [[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]]
    for i in range(3):
        for j in range(3):
            N[i][j] = N[3 + i][3 + j] = G[i][j]
    c6 = [-S[6], -S[8], -S[9], -S[11], -S[13], -S[14]]
    c7 = [-S[7], -S[9], -S[10], -S[12], -S[14], -S[15]]
    for i in range(6):
        N[i][6] = N[6][i] = c6[i]
        N[i][7] = N[7][i] = c7[i]
    N[6][6], N[6][7], N[7][6], N[7][7] = S[16], S[17], S[17], S[18]
    r = [S[19], S[20], S[21], S[22], S[23], S[24], -S[25], -S[26]]
    return N, r


def corners(width, height):
    """(a, b) of the frame's four corners."""
    s = float(scale(width, height))
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    a0, a1 = (0.0 - cx) / s, (float(width - 1) - cx) / s
    b0, b1 = (0.0 - cy) / s, (float(height - 1) - cy) / s
    return [(a0, b0), (a1, b0), (a0, b1), (a1, b1)]


def accept(c, width, height):
    """The model tests after the solve: finite, d > 1/8 at the corners."""
    if c is None or not all(math.isfinite(v) for v in c):
        return False
    return all(1.0 + (c[6] * a + c[7] * b) > 0.125 for a, b in corners(width, height))


def solve(S, width, height):
    """The centred, scaled model (eight Python floats) of the sums, or None."""
    N, r = normal_system(S)
    out = ldl_solve(N, [r])
    if out is None or not accept(out[0], width, height):
        return None
    return out[0]


def agrees(flow, c, threshold):
    """(H, W) bool: d > 0 and the squared residual <= T2 / s^2 against the model
    c (None: nowhere)."""
    f = np.asarray(flow)
    H, W = f.shape[:2]
    if c is None:
        return np.zeros((H, W), bool)
    s = float(scale(W, H))
    a, b = _coords(W, H)
    U, V = _uv(f, W, H)
    t2s = (float(F32(threshold)) * float(F32(threshold))) / (s * s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = c[6] * a + c[7] * b
        d = 1.0 + g
        eU = (((c[0] + c[1] * a) + c[2] * b) - a * g) / d
        eV = (((c[3] + c[4] * a) + c[5] * b) - b * g) / d
        rU, rV = U - eU, V - eV
        return ((d > 0.0) & (rU * rU + rV * rV <= t2s)).reshape(H, W)


def to_frame(c, width, height):
    """The eight frame-coordinate parameters (Python floats) of a centred model."""
    s = float(scale(width, height))
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    ax, ay = cx / s, cy / s
    g00 = c[6] * ((0.0 - cx) / s) + c[7] * ((0.0 - cy) / s)
    w = 1.0 + g00
    return [((((s * c[0]) - c[1] * cx) - c[2] * cy) + cx * g00) / w,
            ((c[1] + ax * c[6]) - g00) / w,
            (c[2] + ax * c[7]) / w,
            ((((s * c[3]) - c[4] * cx) - c[5] * cy) + cy * g00) / w,
            (c[4] + ay * c[6]) / w,
            ((c[5] + ay * c[7]) - g00) / w,
            (c[6] / s) / w,
            (c[7] / s) / w]


def fit_one(flow, mask=None, iterations=3, threshold=1.0, history=None):
    """One (H, W, 2) field -> (params float32 (8,), info uint32 (4,), inliers u8
    (H, W), centred model or None)."""
    f = np.asarray(flow)
    H, W = f.shape[:2]
    tr = trusted(f, mask)
    T = terms(f)
    member, c, first, S = tr, None, 0, None
    for j in range(iterations + 1):
        S = sums(f, member, T)
        if j == 0:
            first = S[0]
        c = solve(S, W, H)
        if history is not None:
            history.append((member, c))
        member = tr & agrees(f, c, threshold)
    inl = member  # against the final model
    if c is None:
        params = np.full(8, NAN32, np.uint32).view(np.float32)
    else:
        with np.errstate(over="ignore"):
            params = np.array(to_frame(c, W, H), np.float64).astype(np.float32)
    info = np.array([0 if c is None else 1, int(first), int(S[0]), int(inl.sum())], np.uint32)
    return params, info, np.where(inl, 255, 0).astype(np.uint8), c


def fit(flow, mask=None, iterations=3, threshold=1.0):
    """disflow.fit_homography(..., return_info=True, return_inliers=True)."""
    f = np.asarray(flow)
    if f.ndim == 3:
        return fit_one(f, mask, iterations, threshold)[:3]
    r = [fit_one(f[k], None if mask is None else mask[k], iterations, threshold) for k in range(f.shape[0])]
    return np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.stack([a[2] for a in r])


def to_flow(params, width, height, out_dtype=np.float32):
    """disflow.homography_to_flow: float32 (8,) or (n, 8) -> (..., H, W, 2)."""
    p = np.asarray(params, np.float32)
    if p.ndim == 2:
        return np.stack([to_flow(q, width, height, out_dtype) for q in p])
    x = np.arange(width, dtype=np.float32)[None, :]
    y = np.arange(height, dtype=np.float32)[:, None]
    nan16 = np.full((height, width, 2), NAN16, np.uint16).view(np.float16)
    nan32 = np.full((height, width, 2), NAN32, np.uint32).view(np.float32)
    f16 = np.dtype(out_dtype) == np.float16
    if not np.isfinite(p).all():
        return nan16 if f16 else nan32
    out = np.empty((height, width, 2), np.float32)
    with np.errstate(all="ignore"):
        g = p[6] * x + p[7] * y
        d = F32(1.0) + g
        out[..., 0] = (((p[0] + p[1] * x) + p[2] * y) - x * g) / d
        out[..., 1] = (((p[3] + p[4] * x) + p[5] * y) - y * g) / d
        out = out.astype(out_dtype)
    ahead = np.broadcast_to((d > F32(0.0))[..., None], out.shape)
    return np.where(ahead, out, nan16 if f16 else nan32)


def warp(image, params, border=warpref.REPLICATE):
    """disflow.warp_homography(..., return_valid=True): (dst, valid)."""
    image = np.asarray(image)
    p = np.asarray(params, np.float32)
    if p.ndim == 1:
        H, W = image.shape[:2]
        return warpref.warp(image, to_flow(p, W, H), 1.0, border)
    H, W = image.shape[1:3]
    out = [warpref.warp(i, to_flow(q, W, H), 1.0, border) for i, q in zip(image, p)]
    return np.stack([d for d, _ in out]), np.stack([m for _, m in out])


def _mul3(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def _norm3(a):
    with np.errstate(all="ignore"):
        return [float(np.float64(v) / np.float64(a[8])) for v in a]


IDENTITY3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def path(pair_params):
    """(the matrices C_0 .. C_{N-1} as nine floats each, the replaced models)."""
    p = np.asarray(pair_params, np.float32).reshape(-1, 8)
    C, bad = [list(IDENTITY3)], 0
    for q in p:
        if np.isfinite(q).all():
            f = [float(v) for v in q]
            A = [1.0 + f[1], f[2], f[0], f[4], 1.0 + f[5], f[3], f[6], f[7], 1.0]
        else:
            A = list(IDENTITY3)
            bad += 1
        with np.errstate(all="ignore"):
            C.append(_norm3([float(v) for v in _mul3([np.float64(v) for v in A], [np.float64(v) for v in C[-1]])]))
    return C, bad


def smooth(C, radius, sigma):
    n = len(C)
    reach = min(radius, n - 1)
    g = weights(sigma, reach + 1)
    S = []
    for k in range(n):
        s, wsum = [np.float64(0.0)] * 9, np.float64(0.0)
        with np.errstate(all="ignore"):
            for j in range(max(0, k - reach), min(n - 1, k + reach) + 1):
                w = np.float64(g[abs(j - k)])
                for e in range(9):
                    s[e] = s[e] + w * np.float64(C[j][e])
                wsum = wsum + w
            S.append([float(v / wsum) for v in s])
    return S


def invert3(s):
    with np.errstate(all="ignore"):
        m = [np.float64(v) for v in s]
        k00, k01, k02 = m[4] * m[8] - m[5] * m[7], m[3] * m[8] - m[5] * m[6], m[3] * m[7] - m[4] * m[6]
        det = (m[0] * k00 - m[1] * k01) + m[2] * k02
        if not math.isfinite(det) or abs(det) <= 2.0 ** -20:
            return None
        adj = [k00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
               m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
               k02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
        return [float(v / det) for v in adj]


def stabilize(pair_params, width, height, radius, sigma=None, zoom=1.0):
    """disflow.stabilize_path_homography(..., with_status=True): corrections
    float32 (N, 8), status u8 (N,), replaced."""
    if sigma is None:
        sigma = max(radius, 1) / 2.0
    C, bad = path(pair_params)
    S = smooth(C, radius, sigma)
    z = 1.0 / float(F32(zoom))
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    Z = [z, 0.0, cx * (1.0 - z), 0.0, z, cy * (1.0 - z), 0.0, 0.0, 1.0]
    out = np.zeros((len(C), 8), np.float32)
    status = np.zeros(len(C), np.uint8)
    for k, (c, s) in enumerate(zip(C, S)):
        inv = invert3(s)
        if inv is None:
            continue
        with np.errstate(all="ignore"):
            d = np.float64
            m = _norm3([float(v) for v in _mul3(_mul3([d(v) for v in c], [d(v) for v in inv]), [d(v) for v in Z])])
            q = np.array([m[2], m[0] - 1.0, m[1], m[5], m[3], m[4] - 1.0, m[6], m[7]], np.float64).astype(np.float32)
        q[6:][q[6:] == 0] = 0.0
        if np.isfinite(q).all():
            out[k] = q
            status[k] = 1
    return out, status, bad


def matrix(q):
    """The 3 x 3 float64 matrix of a model's eight parameters."""
    q = np.asarray(q, np.float64)
    return np.array([[1 + q[1], q[2], q[0]], [q[4], 1 + q[5], q[3]], [q[6], q[7], 1]])


def params_of(M):
    """The eight parameters (float64) of a 3 x 3 matrix, normalised."""
    M = np.asarray(M, np.float64) / M[2][2]
    return np.array([M[0, 2], M[0, 0] - 1, M[0, 1], M[1, 2], M[1, 0], M[1, 1] - 1, M[2, 0], M[2, 1]])


def field64(q, width, height):
    """The float64 field of eight parameters (no order promised): the truth of a test."""
    q = np.asarray(q, np.float64)
    x = np.arange(width, dtype=np.float64)[None, :]
    y = np.arange(height, dtype=np.float64)[:, None]
    g = q[6] * x + q[7] * y
    return np.stack([(q[0] + q[1] * x + q[2] * y - x * g) / (1 + g), (q[3] + q[4] * x + q[5] * y - y * g) / (1 + g)], -1)
