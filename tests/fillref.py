"""numpy float32 restatement of the push-pull fill of untrusted flow vectors
(csrc/dis_fill.hip; dis_flow_fill in include/dis_abi.h): whole arrays,
np.float32 throughout (never float64), one separately rounded operation per
numpy call, in the kernels' order -- so the results agree bit for bit."""
import numpy as np

F32 = np.float32

NAN32 = np.uint32(0x7fc00000)  # the canonical quiet NaN of an empty field
NAN16 = np.uint16(0x7e00)

# k[c], c = the number of trusted children; k[3] is the float next above 1/3
K = np.array([0, 0x3f800000, 0x3f000000, 0x3eaaaaab, 0x3e800000], np.uint32).view(F32)
QUARTER = F32(0.25)


def level_sizes(W, H):
    """[(W_0, H_0), ..., (1, 1)]: W_{l+1} = (W_l + 1) // 2, H likewise."""
    out = [(W, H)]
    while out[-1] != (1, 1):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def workspace_cells(W, H):
    """Cells of levels 1..L of one W x H field."""
    return sum(w * h for w, h in level_sizes(W, H)[1:])


def trusted(flow, mask=None):
    """ok_0 of (..., 2) vectors: |u| < 1e9 and |v| < 1e9 (False for NaN), and a
    nonzero mask byte when a mask is given."""
    f = np.asarray(flow).astype(F32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(f[..., 0]) < F32(1e9)) & (np.abs(f[..., 1]) < F32(1e9))
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    return ok


def pull(v, ok):
    """Level l (v: (H, W, 2) float32, ok: (H, W) bool) -> level l+1 (m, ok)."""
    H, W = ok.shape
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    vp = np.zeros((2 * H1, 2 * W1, 2), F32)
    okp = np.zeros((2 * H1, 2 * W1), bool)
    vp[:H, :W] = np.where(ok[..., None], v, F32(0))  # an untrusted vector never enters arithmetic
    okp[:H, :W] = ok
    cv = [vp[0::2, 0::2], vp[0::2, 1::2], vp[1::2, 0::2], vp[1::2, 1::2]]  # c00, c01, c10, c11
    co = [okp[0::2, 0::2], okp[0::2, 1::2], okp[1::2, 0::2], okp[1::2, 1::2]]
    c = co[0].astype(np.int64) + co[1] + co[2] + co[3]
    f = np.where(co[0][..., None], cv[0], np.where(co[1][..., None], cv[1], np.where(co[2][..., None], cv[2], cv[3])))
    d = [np.where(o[..., None], x - f, F32(0)) for x, o in zip(cv, co)]
    m = f + ((d[0] + d[1]) + (d[2] + d[3])) * K[c][..., None]
    assert m.dtype == F32
    return m, c > 0


def push(g1, W, H):
    """r of every cell of a W x H level from the complete level above it."""
    H1, W1 = g1.shape[:2]
    x, y = np.arange(W), np.arange(H)
    px, py = x >> 1, y >> 1
    qx = np.clip(px + np.where(x & 1, 1, -1), 0, W1 - 1)
    qy = np.clip(py + np.where(y & 1, 1, -1), 0, H1 - 1)
    P, Q = g1[py[:, None], px[None, :]], g1[py[:, None], qx[None, :]]
    R, S = g1[qy[:, None], px[None, :]], g1[qy[:, None], qx[None, :]]
    h0 = P + QUARTER * (Q - P)
    h1 = R + QUARTER * (S - R)
    r = h0 + QUARTER * (h1 - h0)
    assert r.dtype == F32
    return r


def fill(flow, mask=None, out_dtype=np.float32):
    """(out, level) of an (H, W, 2) field or an (n, H, W, 2) stack, float32 or
    float16 (widened exactly); mask: u8 (..., H, W) or None. out has out_dtype
    (float32 or float16), level is u8."""
    flow = np.asarray(flow)
    assert flow.dtype in (np.float32, np.float16) and flow.shape[-1] == 2
    out_dtype = np.dtype(out_dtype)
    assert out_dtype in (np.float32, np.float16)
    if flow.ndim == 4:
        res = [fill(flow[k], None if mask is None else mask[k], out_dtype) for k in range(len(flow))]
        return np.stack([o for o, _ in res]), np.stack([lv for _, lv in res])
    H, W = flow.shape[:2]
    ok0 = trusted(flow, mask)
    v0 = flow.astype(F32)
    ms, oks = [v0], [ok0]
    while oks[-1].shape != (1, 1):
        m, ok = pull(ms[-1], oks[-1])
        ms.append(m)
        oks.append(ok)
    L = len(ms) - 1
    if not oks[L][0, 0]:
        bits = NAN32 if out_dtype == np.float32 else NAN16
        return np.full((H, W, 2), bits).view(out_dtype), np.full((H, W), 255, np.uint8)
    g, lev = ms[L], np.full((1, 1), L, np.int64)
    for l in range(L - 1, -1, -1):
        h, w = oks[l].shape
        r = push(g, w, h)
        g = np.where(oks[l][..., None], ms[l], r)
        lev = np.where(oks[l], l, lev[(np.arange(h) >> 1)[:, None], (np.arange(w) >> 1)[None, :]])
    with np.errstate(over="ignore"):
        # a trusted pixel: its input vector in out_dtype (equal formats: the same bits)
        out = np.where(ok0[..., None], flow.astype(out_dtype), g.astype(out_dtype))
    assert out.dtype == out_dtype
    return out, lev.astype(np.uint8)
