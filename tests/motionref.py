"""dis_flow_fit_motion and dis_motion_to_flow (include/dis_abi.h) restated in
numpy, operation for operation: float64 sums in the fixed order of the
contract (slots of a chunk, adjacent pairs, chunks in turn), the LDL^T solve in
Python floats (IEEE doubles, one rounding per operation), float32 for the
synthesised field. The GPU tests compare with it bit for bit."""
import numpy as np

CHUNK, SLOTS, STEPS = 16384, 256, 64
NAN32 = np.uint32(0x7FC00000)
NAN16 = np.uint16(0x7E00)
TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
MODELS = {"translation": TRANSLATION, "similarity": SIMILARITY, "affine": AFFINE}
TOL = 2.0 ** -20


def chunks(width, height):
    return (width * height + CHUNK - 1) // CHUNK


def workspace_bytes(n, width, height):
    return n * (chunks(width, height) * 12 + 16) * 8


def trusted(flow, mask=None):
    """(H, W) bool: the test on the float32 values (float16 widens exactly)."""
    f = np.asarray(flow).astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(f[..., 0]) < np.float32(1e9)) & (np.abs(f[..., 1]) < np.float32(1e9))
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok


def _coords(width, height):
    q = np.arange(width * height)
    x = (q % width).astype(np.float64) - (width - 1) / 2.0
    y = (q // width).astype(np.float64) - (height - 1) / 2.0
    return x, y


def _uv(flow):
    f = np.asarray(flow).astype(np.float32)
    return f[..., 0].reshape(-1).astype(np.float64), f[..., 1].reshape(-1).astype(np.float64)


def sums(flow, member):
    """The twelve sums of one (H, W, 2) field over the pixels of `member` (H, W)
    bool, in the contract's order."""
    H, W = member.shape
    n = W * H
    x, y = _coords(W, H)
    u, v = _uv(flow)
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.stack([np.ones(n), x, y, x * x, x * y, y * y, u, x * u, y * u, v, x * v, y * v])
    T = np.where(member.reshape(-1)[None, :], T, 0.0)  # a select: no other pixel's vector enters a sum
    nch = chunks(W, H)
    P = np.zeros((12, nch * CHUNK))
    P[:, :n] = T
    P = P.reshape(12, nch, STEPS, SLOTS)
    acc = np.zeros((12, nch, SLOTS))
    for k in range(STEPS):
        acc = acc + P[:, :, k, :]
    while acc.shape[2] > 1:
        acc = acc[:, :, 0::2] + acc[:, :, 1::2]
    acc = acc[:, :, 0]
    tot = np.zeros(12)
    for c in range(nch):
        tot = tot + acc[:, c]
    return [float(t) for t in tot]


def ldl_solve(A, bs):
    """A x = b for each b of bs by LDL^T without pivoting; None when a pivot is
    not above 2^-20 of its diagonal element."""
    m = len(A)
    L = [[0.0] * m for _ in range(m)]
    d = [0.0] * m
    for j in range(m):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * d[k]
        if not dj > TOL * A[j][j]:
            return None
        d[j] = dj
        for i in range(j + 1, m):
            t = A[i][j]
            for k in range(j):
                t = t - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = t / dj
    out = []
    for b in bs:
        z = list(b)
        for i in range(m):
            for k in range(i):
                z[i] = z[i] - L[i][k] * z[k]
        for i in range(m):
            z[i] = z[i] / d[i]
        for i in reversed(range(m)):
            for k in range(i + 1, m):
                z[i] = z[i] - L[k][i] * z[k]
        out.append(z)
    return out


def solve(S, model):
    """The centred model (six Python floats) of the sums, or None."""
    S1, Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = S
    if model == AFFINE:
        r = ldl_solve([[S1, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]], [[Su, Sxu, Syu], [Sv, Sxv, Syv]])
        return None if r is None else r[0] + r[1]
    if model == SIMILARITY:
        q = Sxx + Syy
        r = ldl_solve([[S1, 0.0, Sx, -Sy], [0.0, S1, Sy, Sx], [Sx, Sy, q, 0.0], [-Sy, Sx, 0.0, q]],
                      [[Su, Sv, Sxu + Syv, Sxv - Syu]])
        if r is None:
            return None
        tx, ty, s, rr = r[0]
        return [tx, s, -rr, ty, rr, s]
    r = ldl_solve([[S1]], [[Su], [Sv]])
    return None if r is None else [r[0][0], 0.0, 0.0, r[1][0], 0.0, 0.0]


def agrees(flow, c, threshold):
    """(H, W) bool: r2 <= T2 against the centred model c (None: nowhere)."""
    f = np.asarray(flow)
    H, W = f.shape[:2]
    if c is None:
        return np.zeros((H, W), bool)
    x, y = _coords(W, H)
    u, v = _uv(f)
    t2 = float(np.float32(threshold)) * float(np.float32(threshold))
    with np.errstate(invalid="ignore", over="ignore"):
        ru = u - ((c[0] + c[1] * x) + c[2] * y)
        rv = v - ((c[3] + c[4] * x) + c[5] * y)
        return (ru * ru + rv * rv <= t2).reshape(H, W)


def fit_one(flow, mask=None, model=AFFINE, iterations=3, threshold=1.0, history=None):
    """One (H, W, 2) field -> (params float32 (6,), info uint32 (4,), inliers u8
    (H, W), centred model or None). info[3] counts the inliers; a call without an
    inlier plane reports 0 there. history (a list) receives each pass's
    (members, centred model)."""
    f = np.asarray(flow)
    H, W = f.shape[:2]
    tr = trusted(f, mask)
    member, c, first, S = tr, None, 0, None
    for j in range(iterations + 1):
        S = sums(f, member)
        if j == 0:
            first = S[0]
        c = solve(S, model)
        if history is not None:
            history.append((member, c))
        member = tr & agrees(f, c, threshold)
    inl = member  # against the final model
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    if c is None:
        params = np.full(6, NAN32, np.uint32).view(np.float32)
    else:
        p = [(c[0] - c[1] * cx) - c[2] * cy, c[1], c[2], (c[3] - c[4] * cx) - c[5] * cy, c[4], c[5]]
        with np.errstate(over="ignore"):
            params = np.array(p, np.float64).astype(np.float32)
    info = np.array([0 if c is None else 1, int(first), int(S[0]), int(inl.sum())], np.uint32)
    return params, info, np.where(inl, 255, 0).astype(np.uint8), c


def fit(flow, mask=None, model="affine", iterations=3, threshold=1.0):
    """disflow.fit_motion(..., return_info=True, return_inliers=True): (H, W, 2) or
    (n, H, W, 2) -> params, info, inliers."""
    f = np.asarray(flow)
    mdl = MODELS.get(model, model)
    if f.ndim == 3:
        return fit_one(f, mask, mdl, iterations, threshold)[:3]
    r = [fit_one(f[k], None if mask is None else mask[k], mdl, iterations, threshold) for k in range(f.shape[0])]
    return np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.stack([a[2] for a in r])


def to_flow(params, width, height, out_dtype=np.float32):
    """disflow.motion_to_flow: float32 (6,) or (n, 6) -> (..., H, W, 2)."""
    p = np.asarray(params, np.float32)
    if p.ndim == 2:
        return np.stack([to_flow(q, width, height, out_dtype) for q in p])
    x = np.arange(width, dtype=np.float32)[None, :]
    y = np.arange(height, dtype=np.float32)[:, None]
    out = np.empty((height, width, 2), np.float32)
    if np.isfinite(p).all():
        with np.errstate(over="ignore", invalid="ignore"):
            out[..., 0] = (p[0] + p[1] * x) + p[2] * y
            out[..., 1] = (p[3] + p[4] * x) + p[5] * y
        out = out.astype(out_dtype)
        return out
    if np.dtype(out_dtype) == np.float16:
        return np.full((height, width, 2), NAN16, np.uint16).view(np.float16)
    return np.full((height, width, 2), NAN32, np.uint32).view(np.float32)
