"""NumPy restatement of the 4:2:0 conversions (csrc/dis_yuv.hip,
dis_yuv420_to_frames_u8 and dis_frames_to_yuv420_u8), with layout helpers.

Arithmetic: integers only, in signed 32 bits (every magnitude stays below
2^25), `>>` the floor shift. One row of TABLE per (matrix,
range); with c = yy*(Y - yoff) + 8192, u = Cb - 128, v = Cr - 128:

    R = clamp((c + rv*v) >> 14)   G = clamp((c + gu*u + gv*v) >> 14)   B = clamp((c + bu*u) >> 14)

for the four pixels of a 2 x 2 block (nearest chroma; gray is clamp(c >> 14)), and

    Y  = yoff + ((ky . (R,G,B) + 8192) >> 14)                          per pixel
    Cb = clamp((kcb . (sR,sG,sB) + (128 << 16) + (1 << 15)) >> 16)      per block, Cr likewise

over the block's sums (sR, sG, sB): the average and the conversion round once.

Derivation (derive(), with rationals). A standard gives Kr and Kb (BT.601:
299/1000 and 114/1000; BT.709: 2126/10000 and 722/10000), Kg = 1 - Kr - Kb, and
    Y' = Kr R + Kg G + Kb B,   Pb = (B - Y') / (2 (1 - Kb)),   Pr = (R - Y') / (2 (1 - Kr)),
so R = Y' + 2(1 - Kr) Pr, B = Y' + 2(1 - Kb) Pb and
G = Y' - (2 (1 - Kb) Kb / Kg) Pb - (2 (1 - Kr) Kr / Kg) Pr. Full range carries Y'
as 0..255 and Pb, Pr as +-127.5 around 128 (the JFIF convention: scales 1 and
1); limited range carries Y' as 16 + 219/255 of it and chroma as 224/255 of it.
Each coefficient is the real one times 2^14, rounded to nearest:
    yy = 255/219 (limited) or 1;  rv = 2(1 - Kr) / cs;  bu = 2(1 - Kb) / cs;
    gu = -2(1 - Kb) Kb / Kg / cs;  gv = -2(1 - Kr) Kr / Kg / cs      (cs = 224/255 or 1)
    ky = ys (Kr, Kg, Kb)                                             (ys = 219/255 or 1)
    kcb = cs (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb));  kcr = cs (1 - Kr, -Kg, -Kb) / (2 (1 - Kr))
and then the green entry of ky, kcb and kcr is replaced by what makes the row
sum to round(ys * 2^14) (16384 or 14071) or to 0: gray then gives Y exactly and
Cb = Cr = 128 exactly."""
from fractions import Fraction

import numpy as np

import lumaref

MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
ROWS = [(m, r) for m in MATRICES for r in RANGES]

# (matrix, range) -> yoff, yy, rv, gu, gv, bu, ky, kcb, kcr
TABLE = {
    ("bt601", "full"): (0, 16384, 22970, -5638, -11700, 29032,
                        (4899, 9617, 1868), (-2765, -5427, 8192), (8192, -6860, -1332)),
    ("bt601", "limited"): (16, 19077, 26149, -6419, -13320, 33050,
                           (4207, 8260, 1604), (-2428, -4768, 7196), (7196, -6026, -1170)),
    ("bt709", "full"): (0, 16384, 25802, -3069, -7670, 30402,
                        (3483, 11718, 1183), (-1877, -6315, 8192), (8192, -7441, -751)),
    ("bt709", "limited"): (16, 19077, 29372, -3494, -8731, 34610,
                           (2991, 10064, 1016), (-1649, -5547, 7196), (7196, -6536, -660)),
}

_K = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}


def _nearest(q):
    """The integer nearest to the rational q (halves away from zero; none occurs)."""
    n = (abs(q) * 2 + 1) // 2
    return int(n if q >= 0 else -n)


def derive(matrix, range_):
    """The row of TABLE from the standard's Kr, Kb with rationals (docstring)."""
    kr, kb = _K[matrix]
    kg = 1 - kr - kb
    ys, cs = (Fraction(219, 255), Fraction(224, 255)) if range_ == "limited" else (Fraction(1), Fraction(1))
    one = 1 << 14
    yoff = 16 if range_ == "limited" else 0
    yy = _nearest(one / ys)
    rv = _nearest(one * 2 * (1 - kr) / cs)
    bu = _nearest(one * 2 * (1 - kb) / cs)
    gu = _nearest(-one * 2 * (1 - kb) * kb / kg / cs)
    gv = _nearest(-one * 2 * (1 - kr) * kr / kg / cs)
    ky = [_nearest(one * ys * k) for k in (kr, kg, kb)]
    ky[1] = _nearest(one * ys) - ky[0] - ky[2]
    kcb = [_nearest(one * cs * k / (2 * (1 - kb))) for k in (-kr, -kg, 1 - kb)]
    kcb[1] = -kcb[0] - kcb[2]
    kcr = [_nearest(one * cs * k / (2 * (1 - kr))) for k in (1 - kr, -kg, -kb)]
    kcr[1] = -kcr[0] - kcr[2]
    return (yoff, yy, rv, gu, gv, bu, tuple(ky), tuple(kcb), tuple(kcr))


def _clamp(v):
    return np.clip(v, 0, 255)


def yuv_to_rgb(y, cb, cr, matrix, range_, clamp=True):
    """The to-frames formula on arrays (or scalars) of samples -> (R, G, B) int32
    (clamp=False: the values before the clamp)."""
    yoff, yy, rv, gu, gv, bu = TABLE[(matrix, range_)][:6]
    y, u, v = np.asarray(y, np.int32), np.asarray(cb, np.int32) - 128, np.asarray(cr, np.int32) - 128
    c = yy * (y - yoff) + 8192
    r, g, b = (c + rv * v) >> 14, (c + gu * u + gv * v) >> 14, (c + bu * u) >> 14
    return (_clamp(r), _clamp(g), _clamp(b)) if clamp else (r, g, b)


def y_to_gray(y, matrix, range_):
    yoff, yy = TABLE[(matrix, range_)][:2]
    return _clamp((yy * (np.asarray(y, np.int32) - yoff) + 8192) >> 14)


def rgb_to_y(r, g, b, matrix, range_):
    yoff, ky = TABLE[(matrix, range_)][0], TABLE[(matrix, range_)][6]
    r, g, b = (np.asarray(v, np.int32) for v in (r, g, b))
    return yoff + ((ky[0] * r + ky[1] * g + ky[2] * b + 8192) >> 14)


def sums_to_chroma(sr, sg, sb, matrix, range_, clamp=True):
    """(Cb, Cr) of a block's sums (each 0..1020); clamp=False: before the clamp."""
    kcb, kcr = TABLE[(matrix, range_)][7:9]
    sr, sg, sb = (np.asarray(v, np.int32) for v in (sr, sg, sb))
    out = []
    for k in (kcb, kcr):
        v = (k[0] * sr + k[1] * sg + k[2] * sb + (128 << 16) + (1 << 15)) >> 16
        out.append(_clamp(v) if clamp else v)
    return tuple(out)


def _rgb_planes(frames, fmt):
    a = np.asarray(frames)
    assert a.dtype == np.uint8
    _, C, order = lumaref.FORMATS[fmt]
    if order is None:
        return a, a, a
    assert a.shape[-1] == C, (a.shape, fmt)
    return a[..., order[0]], a[..., order[1]], a[..., order[2]]


def to_yuv420(frames, fmt, matrix, range_):
    """(..., H, W[, C]) u8 frames of format `fmt` (even H, W) -> the planes
    (Y (..., H, W), Cb (..., H/2, W/2), Cr) as u8."""
    r, g, b = _rgb_planes(frames, fmt)
    H, W = r.shape[-2:]
    assert H % 2 == 0 and W % 2 == 0
    y = rgb_to_y(r, g, b, matrix, range_).astype(np.uint8)

    def block_sums(p):
        p = p.astype(np.int32)
        return p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]
    cb, cr = sums_to_chroma(block_sums(r), block_sums(g), block_sums(b), matrix, range_)
    return y, cb.astype(np.uint8), cr.astype(np.uint8)


def to_frames(y, cb, cr, fmt, matrix, range_, alpha=255):
    """The planes (Y (..., H, W), Cb and Cr (..., H/2, W/2); None for "gray")
    -> (..., H, W[, C]) u8 frames of format `fmt`."""
    y = np.asarray(y)
    _, C, order = lumaref.FORMATS[fmt]
    if order is None:
        return y_to_gray(y, matrix, range_).astype(np.uint8)
    up = lambda p: np.repeat(np.repeat(np.asarray(p), 2, axis=-2), 2, axis=-1)  # noqa: E731
    rgb = yuv_to_rgb(y, up(cb), up(cr), matrix, range_)
    out = np.empty(y.shape + (C,), np.uint8)
    for k in range(3):
        out[..., order[k]] = rgb[k]
    if C == 4:
        out[..., 3] = alpha
    return out


# ---------------------------------------------------------------------------
# layouts: where the planes of a surface lie in a flat buffer
# ---------------------------------------------------------------------------
LAYOUTS = ("nv12", "nv21", "i420", "yv12")


def surface_layout(layout, W, H, y_stride=0, gap=0):
    """One image's planes in one buffer, as the ABI's arguments (offsets from
    the buffer's first byte): dict(y, cb, cr, c_step, y_stride, c_stride, bytes).
    y_stride 0 = W; planar chroma rows are y_stride // 2 apart; `gap` bytes lie
    between the planes. `bytes` is a whole image (the distance to the next)."""
    ys = y_stride or W
    if layout in ("nv12", "nv21"):
        c0 = ys * H + gap
        c1, step, cs, size = c0 + 1, 2, ys, c0 + ys * (H // 2) + gap
    else:
        cs = ys // 2
        c0 = ys * H + gap
        c1, step = c0 + cs * (H // 2) + gap, 1
        size = c1 + cs * (H // 2) + gap
    cb, cr = (c1, c0) if layout in ("nv21", "yv12") else (c0, c1)
    return dict(y=0, cb=cb, cr=cr, c_step=step, y_stride=ys, c_stride=cs, bytes=size)


def place(buf, base, lay, image_stride, y, cb, cr):
    """Write the planes (n, H, W) / (n, H/2, W/2) into the flat u8 buffer."""
    n, H, W = y.shape
    for i in range(n):
        o = base + i * image_stride
        for r in range(H):
            buf[o + lay["y"] + r * lay["y_stride"]:][:W] = y[i, r]
        for name, p in (("cb", cb), ("cr", cr)):
            for r in range(H // 2):
                s = o + lay[name] + r * lay["c_stride"]
                buf[s:s + (W // 2 - 1) * lay["c_step"] + 1:lay["c_step"]] = p[i, r]
    return buf
