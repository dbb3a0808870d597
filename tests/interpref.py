"""numpy float32 restatement of the frame interpolation (csrc/dis_interp.hip,
dis_flow_interp_u8 in include/dis_abi.h): whole arrays, np.float32 throughout
(never float64), one separately rounded operation per numpy call, in the
kernels' order -- so the results agree bit for bit. The sampler is
tests/warpref.py's; the splat is np.minimum.at on a uint64 key array, whose
result, like the kernel's atomicMin, does not depend on the order of arrival.

Also the two-layer scene with known flows that the quality check and the GPU
tests share (two_layer_scene)."""
import numpy as np

F32 = np.float32
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _valid(u, v):
    with np.errstate(invalid="ignore"):
        return (np.abs(u) < F32(1e9)) & (np.abs(v) < F32(1e9))  # False for NaN


def _sample(img, u, v, k):
    """dis_flow_warp_u8's steps 2-5 (replicate) on img (H, W, C) u8 with valid
    vectors (u, v) and scale k: the unrounded sums (H, W, C) and `inside`."""
    H, W, C = img.shape
    k = F32(k)
    x = np.arange(W, dtype=F32)[None, :]
    y = np.arange(H, dtype=F32)[:, None]
    xm, ym, zero, one = F32(W - 1), F32(H - 1), F32(0), F32(1)
    su = k * u
    sv = k * v
    px = x + su
    py = y + sv
    assert px.dtype == F32 and py.dtype == F32
    inside = (px >= zero) & (px <= xm) & (py >= zero) & (py <= ym)
    px = np.minimum(np.maximum(px, zero), xm)
    py = np.minimum(np.maximum(py, zero), ym)
    x0 = np.floor(px)
    y0 = np.floor(py)
    a = px - x0
    b = py - y0
    ix0 = x0.astype(np.int64)
    iy0 = y0.astype(np.int64)
    assert ix0.min() >= 0 and ix0.max() <= W - 1 and iy0.min() >= 0 and iy0.max() <= H - 1
    ix1 = np.minimum(ix0 + 1, W - 1)
    iy1 = np.minimum(iy0 + 1, H - 1)
    ia, ib = one - a, one - b
    w00, w01, w10, w11 = ia * ib, a * ib, ia * b, a * b
    s = np.empty((H, W, C), F32)
    for c in range(C):
        P = img[..., c].astype(F32)
        s[..., c] = ((w00 * P[iy0, ix0] + w01 * P[iy0, ix1]) + w10 * P[iy1, ix0]) + w11 * P[iy1, ix1]
    return s, inside


def interp(I0, I1, fw, t, bw=None, details=False):
    """(dst u8, fill u8, count) of the frame at time t between I0 and I1, images
    (H, W), (H, W, C), (n, H, W) or (n, H, W, C) as warpref.warp takes them, fw
    and bw (may be None) (H, W, 2) or (n, H, W, 2), float32 or float16 (widened
    exactly). count (..., H, W) is the number of splat candidates of every target.
    details (one image only): a fourth value, the (target, source) index pairs
    of all candidates as two int64 arrays."""
    I0, I1, fw = np.asarray(I0), np.asarray(I1), np.asarray(fw)
    assert I0.dtype == np.uint8 and I1.dtype == np.uint8 and I0.shape == I1.shape
    assert fw.dtype in (np.float32, np.float16) and fw.shape[-1] == 2
    if bw is not None:
        bw = np.asarray(bw)
        assert bw.dtype == fw.dtype and bw.shape == fw.shape
    H, W = fw.shape[-3:-1]
    if fw.ndim == 4 or (I0.ndim == 3 and I0.shape[:2] != (H, W)):
        assert not details
        f4 = fw if fw.ndim == 4 else fw[None]
        b4 = [None] * len(f4) if bw is None else (bw if bw.ndim == 4 else bw[None])
        assert len(I0) == len(f4)
        out = [interp(a, b, f, t, g) for a, b, f, g in zip(I0, I1, f4, b4)]
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]).reshape(fw.shape[:-1]),
                np.stack([o[2] for o in out]).reshape(fw.shape[:-1]))
    A, B = I0.reshape(H, W, -1), I1.reshape(H, W, -1)
    C = A.shape[2]
    fl = fw.astype(F32)  # exact for float16
    t = F32(t)
    assert F32(0) <= t <= F32(1)
    tb = F32(1) - t
    zero = F32(0)
    x = np.arange(W, dtype=F32)[None, :]
    y = np.arange(H, dtype=F32)[:, None]
    xm, ym = F32(W - 1), F32(H - 1)
    u, v = fl[..., 0], fl[..., 1]
    ok = _valid(u, v)
    us, vs = np.where(ok, u, zero), np.where(ok, v, zero)  # an invalid vector is read as (0, 0)

    # 1. splat
    s1, in1 = _sample(B, us, vs, 1.0)  # (1 * u is u)
    part = ok & in1
    cost = np.abs(A[..., 0].astype(F32) - s1[..., 0])
    for c in range(1, C):
        cost = cost + np.abs(A[..., c].astype(F32) - s1[..., c])
    assert cost.dtype == F32 and (cost[part] >= 0).all()
    index = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    key = (np.ascontiguousarray(cost).view(np.uint32).astype(np.uint64) << np.uint64(32)) | index
    tu = t * us
    tv = t * vs
    tx = x + tu
    ty = y + tv
    assert tx.dtype == F32 and ty.dtype == F32
    fx = (np.floor(tx), np.ceil(tx))
    fy = (np.floor(ty), np.ceil(ty))
    keys = np.full(H * W, NOKEY, np.uint64)
    count = np.zeros(H * W, np.int64)
    pairs_q, pairs_s = [], []
    for j in range(2):
        for k in range(2):
            m = part & (fx[k] >= zero) & (fx[k] <= xm) & (fy[j] >= zero) & (fy[j] <= ym)
            if j:
                m = m & (fy[1] != fy[0])
            if k:
                m = m & (fx[1] != fx[0])
            q = fy[j][m].astype(np.int64) * W + fx[k][m].astype(np.int64)
            assert q.size == 0 or (q.min() >= 0 and q.max() < H * W)
            np.minimum.at(keys, q, key[m])
            np.add.at(count, q, 1)
            pairs_q.append(q)
            pairs_s.append(index[m].astype(np.int64))

    # 2. blend
    K = keys.reshape(H, W)
    hit = K != NOKEY
    src = np.where(hit, K & np.uint64(0xFFFFFFFF), np.uint64(0)).astype(np.int64)
    wu = np.where(hit, u.reshape(-1)[src], us)  # a hole: the pixel's own vector, sanitised
    wv = np.where(hit, v.reshape(-1)[src], vs)
    assert _valid(wu, wv).all()
    s0, in0 = _sample(A, wu, wv, -t)
    s1, in1 = _sample(B, wu, wv, tb)
    m1 = np.zeros((H, W), bool)
    if bw is not None:
        bl = bw.astype(F32)
        bu, bv = bl[..., 0], bl[..., 1]
        bok = _valid(bu, bv)
        sb, inb = _sample(B, np.where(bok, bu, zero), np.where(bok, bv, zero), -tb)
        m1 = ~hit & bok & inb
    dst = np.empty((H, W, C), np.uint8)
    for c in range(C):
        p0 = tb * s0[..., c]
        p1 = t * s1[..., c]
        both = p0 + p1
        assert both.dtype == F32
        r = np.where(in0 == in1, both, np.where(in0, s0[..., c], s1[..., c]))
        if bw is not None:
            r = np.where(m1, sb[..., c], r)
        dst[..., c] = np.minimum(np.maximum(np.rint(r), zero), F32(255)).astype(np.uint8)
    fill = np.where(hit, 0, np.where(m1, 1, 2)).astype(np.uint8)
    out = (dst.reshape(I0.shape), fill, count.reshape(H, W))
    if details:
        out += ((np.concatenate(pairs_q), np.concatenate(pairs_s)),)
    return out


def contested_with_different_vectors(fw, pairs):
    """Number of targets with more than one candidate whose candidates do not
    all carry the same vector (pairs: interp(..., details=True)[3])."""
    q, s = pairs
    vec = np.asarray(fw).astype(F32).reshape(-1, 2)[s]
    order = np.argsort(q, kind="stable")
    q, vec = q[order], vec[order]
    first = np.r_[True, q[1:] != q[:-1]]
    group = np.cumsum(first) - 1
    lead = vec[np.flatnonzero(first)][group]  # each candidate's group leader's vector
    differs = np.zeros(group[-1] + 1 if len(group) else 0, bool)
    np.logical_or.at(differs, group, (vec != lead).any(axis=1))
    return int(differs.sum())


# ---------------------------------------------------------------------------
# the two-layer scene: a textured rectangle moving by (12, 4) over a textured
# background moving by (-2, 0), 64 x 48, one channel
# ---------------------------------------------------------------------------
SCENE_W, SCENE_H = 64, 48
_RX, _RY, _RW, _RH = 20, 14, 18, 14
_FG, _BG = (12.0, 4.0), (-2.0, 0.0)


def scene_frame(t):
    """The scene at time t (float64 rendering, rounded and clipped to u8) and
    the mask of the rectangle's pixels."""
    x = np.arange(SCENE_W, dtype=np.float64)[None, :]
    y = np.arange(SCENE_H, dtype=np.float64)[:, None]
    img = 110.0 + 40.0 * np.sin((x - _BG[0] * t) / 5.0) * np.cos((y - _BG[1] * t) / 6.0)
    ox, oy = x - (_RX + _FG[0] * t), y - (_RY + _FG[1] * t)
    rect = (ox >= 0) & (ox < _RW) & (oy >= 0) & (oy < _RH)
    img = np.where(rect, 200.0 + 30.0 * np.sin(ox / 2.0) * np.sin(oy / 3.0), img)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), rect


def two_layer_scene():
    """(I0, I1, fw, bw): the scene at t = 0 and t = 1 and its analytic float32
    flows, I0 -> I1 on I0's pixels and I1 -> I0 on I1's."""
    I0, r0 = scene_frame(0.0)
    I1, r1 = scene_frame(1.0)
    fw = np.where(r0[..., None], np.array(_FG, F32), np.array(_BG, F32)).astype(F32)
    bw = np.where(r1[..., None], -np.array(_FG, F32), -np.array(_BG, F32)).astype(F32)
    return I0, I1, fw, bw
