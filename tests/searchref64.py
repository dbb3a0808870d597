"""One PatchGrid level in float64, with a trace -- tests only.

The tolerance mode (DIS_PRECISION_FMA) is the one kernel family not held bit
for bit to the oracle; tests/test_gpu_fma_levels.py checks it level by level
against this module instead: every level gets the GPU's own, exactly known
start, so after a few updates of a smooth map the comparison is at rounding
scale and not at the scale of the iteration's chaos (outlier-reset flips).

``search(planes..., init, mode="f64")`` has the semantics of
``pyref.search_level`` / ``oracle/dis_oracle.c`` (grid geometry, Sobel template
gradients from the padded planes, the Hessian with the ``det == 0``
regularisation, the start from a per-patch init, the bilinear warp with the
``ceil(p + 1e-5f)`` tap base (Q8), mean normalisation, the solve, the outlier /
out-of-bounds reset, ``it + 1`` updates), vectorised over the patches, in plain
float64: dot products and a pivoted 2 x 2 solve, no summation order imitated.
Besides ``u`` it returns, per patch,

``S``        the first-order rounding scale of the result, summed over the
             updates actually run:
                 |H^-1|_inf * sum_i (|gx_i| + |gy_i|) (|r_i| + |mean r|)
               + cond_inf(H) * |d|_inf
             (the right-hand sides' error carried through the solve, and the
             Hessian's own rounding). ``rho(u', trace)`` is the normalised error
             |u' - u64|_inf / (2^-24 S); where S = 0 (flat patch, b = 0, or no
             update run) u' must equal u64 exactly.
``fragile``  the float64 trajectory came within DELTA = 1e-3 px of a decision
             (the outlier threshold on the distance from the start, one of the
             four bounds, on the start or an updated position); or a sample
             coordinate's fraction lay within 2e-5 of an integer without being
             one (below it: the Q8 quirk, where tap base and weights disagree;
             above it: a float32 run a rounding away sits in that zone); or the
             float32 and float64 determinants fall on different sides of
             ``det == 0``; or the start is out of bounds in one precision only.
             Fragile patches are left out of the rho statistics and counted.

``mode="f32"`` is the same search in float32 in the reference's order (Eigen's
reduction, every operation rounded once). With no mutation it equals
``pyref.search_level`` bit for bit (tests/test_search64_host.py pins that on
the whole case matrix); with a ``mutation`` it is wrong in one way a kernel
could be wrong, for the sensitivity test; with a ``style`` it restates the
rounding steps of the tolerance mode (centred gradients, contracted products,
reciprocal pivots, the 2-lanes-per-patch summation order) on top of the
reference order. The yardstick of the acceptance function is
``pyref.search_level`` itself, never the code under test; the full
2-lanes-per-patch restatement (``FMA_LPP2``) is the second member of the
yardstick set, having reproduced on the CPU the one excess over K that kernel
showed on the GPU (tests/test_search64_host.py).

numpy >= 2 (NEP 50): float32 op Python-scalar stays float32.
"""
import math

import numpy as np

f32 = np.float32
f64 = np.float64

K = 4            # candidate's max / median rho over the yardstick's
DELTA = 1e-3     # px: distance from a decision that makes a patch fragile
FRAC_EPS = 2e-5  # a sample coordinate's fraction this close to an integer: fragile
FRAGILE_CAP = 0.01
U24 = 2.0 ** -24

MUTATIONS = ("drop_tap", "swap_w1_w2", "grad_shift", "mean56", "no_mean", "recip_wrong_row")


def grid(W, H, st):
    npw = int(math.ceil(f32(W) / f32(st)))
    nph = int(math.ceil(f32(H) / f32(st)))
    return npw, nph, (W - (npw - 1) * st) // 2, (H - (nph - 1) * st) // 2


def patch_refs(W, H, st):
    """Integer reference points (rx, ry) of every patch, patch-id order gx * nph + gy."""
    npw, nph, offw, offh = grid(W, H, st)
    gx, gy = np.divmod(np.arange(npw * nph), nph)
    return gx * st + offw, gy * st + offh


def start_from_dense(dense, W, H, st):
    """The level's per-patch init from the dense field of the level above (or a
    warm start's coarse init plane): 2 * dense[ry >> 1, rx >> 1], float32."""
    rx, ry = patch_refs(W, H, st)
    return (np.asarray(dense, f32)[ry >> 1, rx >> 1] * f32(2)).astype(f32)


def _eigen_sum(x):
    """Eigen 3.3 SSE redux order over the last axis (64 values), float32."""
    p0, p1 = x[:, 0:4], x[:, 4:8]
    for i in range(8, x.shape[1], 8):
        p0 = p0 + x[:, i:i + 4]
        p1 = p1 + x[:, i + 4:i + 8]
    p0 = p0 + p1
    return (p0[:, 0] + p0[:, 2]) + (p0[:, 1] + p0[:, 3])


def _fma(x, y, acc):
    """x * y + acc rounded once to float32, exactly: the product is exact in
    float64, the float64 sum is rounded to odd (TwoSum gives its error), so
    the second rounding to float32 cannot double-round."""
    p = np.asarray(x, f64) * np.asarray(y, f64)
    p, a = np.broadcast_arrays(p, np.asarray(acc, f64))
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)
    s = np.ascontiguousarray(s)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def _eigen_dot(g, r, fma=False):
    """sum(g * r) over the last axis in Eigen's order; fma: each product
    contracted into the accumulation (the first of each chain is a plain product)."""
    if not fma:
        return _eigen_sum(g * r)
    p0, p1 = g[:, 0:4] * r[:, 0:4], g[:, 4:8] * r[:, 4:8]
    for i in range(8, g.shape[1], 8):
        p0 = _fma(g[:, i:i + 4], r[:, i:i + 4], p0)
        p1 = _fma(g[:, i + 4:i + 8], r[:, i + 4:i + 8], p1)
    p0 = p0 + p1
    return (p0[:, 0] + p0[:, 2]) + (p0[:, 1] + p0[:, 3])


def _column_chains(g, r, fma):
    """Per pixel column c (8 of them, the patch row-major): the chain over the
    rows j of g[j, c] * r[j, c] (r None: of g[j, c]), as k_search8<2> keeps
    them: 4 columns per lane."""
    G = g.reshape(len(g), 8, 8)
    if r is None:
        a = G[:, 0]
        for j in range(1, 8):
            a = a + G[:, j]
        return a
    R = r.reshape(len(r), 8, 8)
    a = G[:, 0] * R[:, 0]
    for j in range(1, 8):
        a = _fma(G[:, j], R[:, j], a) if fma else a + G[:, j] * R[:, j]
    return a


def _lpp2_dot(g, r, fma, split=False):
    """The 2-lanes-per-patch orders of dis_search8.hip: patch_dot<2> / patch_sum<2>
    pair column ci with ci + 4 across the two lanes first; the tolerance mode's
    iterate_split (split) sums each lane's 4 columns, then the two lanes."""
    a = _column_chains(g, r, fma)
    if split:
        return ((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])) + ((a[:, 4] + a[:, 5]) + (a[:, 6] + a[:, 7]))
    c = a[:, 0:4] + a[:, 4:8]
    return (c[:, 0] + c[:, 2]) + (c[:, 1] + c[:, 3])


def _lu_solve(h00, h01, h10, h11, b0, b1, wrong_row=False, recip=False, fma=False):
    """PartialPivLU of the 2 x 2 system, elementwise in the arrays' own type.
    recip: the pivots' rounded reciprocals multiplied in (tolerance mode)."""
    sw = np.abs(h10) > np.abs(h00)
    a00, a10 = np.where(sw, h10, h00), np.where(sw, h00, h10)
    a01, a11 = np.where(sw, h11, h01), np.where(sw, h01, h11)
    c0, c1 = np.where(sw, b1, b0), np.where(sw, b0, b1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        l10 = np.where(a00 != 0, a10 / np.where(a00 != 0, a00, 1), a10)
        a11 = a11 - l10 * a01
        c1 = c1 - l10 * c0
        if recip:
            c1 = c1 * (a11.dtype.type(1) / a11)
            c0 = _fma(-c1, a01, c0) if fma else c0 - c1 * a01
            c0 = c0 * (a00.dtype.type(1) / a00)
        elif wrong_row:  # mutation: the pivots' reciprocals on each other's rows
            c1 = c1 / a00
            c0 = c0 - c1 * a01
            c0 = c0 / a11
        else:
            c1 = c1 / a11
            c0 = c0 - c1 * a01
            c0 = c0 / a00
    return c0, c1


class Trace:
    """What search(mode="f64") returns besides u (all per patch)."""

    def __init__(self, u, S, fragile, updates):
        self.u, self.S, self.fragile, self.updates = u, S, fragile, updates

    @property
    def fragile_share(self):
        return float(self.fragile.mean())


STYLES = ("centred", "fma", "recip", "lpp2")
# k_search8<2, kFma> restated step by step (the second member of the yardstick set)
FMA_LPP2 = STYLES


def search(dxp, dyp, I1p, pad, W, H, ps, st, it, norm, init, mode="f64", mutation=None, style=()):
    """One level over the oracle's padded planes. init: (N, 2) float32 per-patch
    start (None: zero). mode "f64": -> Trace; mode "f32": -> u (N, 2) float32.
    style (mode "f32"): rounding steps of the tolerance mode restated on top of
    the reference order -- "centred": sum((g - mean g) r) with gradients centred
    once per patch instead of sum(g (r - mean r)) (the Hessian keeps the raw
    gradients); "fma": warp and dot products contracted; "recip": the solve
    multiplies by the pivots' rounded reciprocals; "lpp2": the sums in the order
    of the 2-lanes-per-patch kernel (with the other three: k_search8<2, kFma>)."""
    assert mode in ("f64", "f32") and (mutation is None or (mode == "f32" and mutation in MUTATIONS))
    assert all(x in STYLES for x in style) and (not style or (mode == "f32" and mutation is None))
    centred, fma, recip, lpp2 = (x in style for x in STYLES)
    # Q8: from |p| >= 256 the float32 epsilon of ceil(p + 1e-5f) is a no-op, another tap rule
    assert max(W, H) + ps < 256 and ps == 8 and pad >= ps
    T = f64 if mode == "f64" else f32
    hp = ps // 2
    N = grid(W, H, st)[0] * grid(W, H, st)[1]
    irx, iry = patch_refs(W, H, st)
    ar = np.arange(ps)
    rows = (iry + pad - hp)[:, None, None] + ar[None, :, None]
    cols = (irx + pad - hp)[:, None, None] + ar[None, None, :]
    if mutation == "grad_shift":
        cols = cols + 1
    gdx32 = dxp[rows, cols].reshape(N, -1)
    gdy32 = dyp[rows, cols].reshape(N, -1)
    dot = (lambda g, r: _lpp2_dot(g, r, fma)) if lpp2 else (lambda g, r: _eigen_dot(g, r, fma))
    h32 = [dot(gdx32, gdx32), dot(gdx32, gdy32), dot(gdy32, gdy32)]
    sing32 = h32[0] * h32[2] - h32[1] * h32[1] == 0
    if mode == "f32":
        gdx, gdy = gdx32, gdy32
        h00, h01, h11 = h32
        sing = sing32
        h00 = np.where(sing, (h00.astype(f64) + 1e-10).astype(f32), h00)
        h11 = np.where(sing, (h11.astype(f64) + 1e-10).astype(f32), h11)
        if centred and norm:
            psum = (lambda g: _lpp2_dot(g, None, False)) if lpp2 else _eigen_sum
            gdx = gdx - (psum(gdx) * f32(1.0 / 64))[:, None]
            gdy = gdy - (psum(gdy) * f32(1.0 / 64))[:, None]
    else:
        gdx, gdy = gdx32.astype(f64), gdy32.astype(f64)
        h00, h01, h11 = (gdx * gdx).sum(1), (gdx * gdy).sum(1), (gdy * gdy).sum(1)
        sing = h00 * h11 - h01 * h01 == 0
        h00 = np.where(sing, h00 + 1e-10, h00)
        h11 = np.where(sing, h11 + 1e-10, h11)
    I1 = I1p.astype(T)
    iu = np.zeros((N, 2), f32) if init is None else np.ascontiguousarray(init, f32).reshape(N, 2)
    rx, ry = irx.astype(T), iry.astype(T)
    thr = T(ps) / T(2)
    lb, ubw, ubh = -T(ps) / T(2), T(W + ps // 2 - 2), T(H + ps // 2 - 2)
    eps = T(f32(1e-5))
    one = T(1)

    def oob(x, y):
        return (x < lb) | (y < lb) | (x > ubw) | (y > ubh)

    def near_bound(x, y):
        return np.minimum.reduce([np.abs(x - lb), np.abs(y - lb), np.abs(x - ubw), np.abs(y - ubh)]) < DELTA

    def near_integer(x):
        fr = x - np.floor(x)
        return ((fr > 0) & (fr < FRAC_EPS)) | (fr > 1 - FRAC_EPS)

    def warp(x, y):
        l, k = np.floor(x), np.floor(y)
        a, b = (x - l)[:, None, None], (y - k)[:, None, None]
        w0, w1, w2, w3 = (one - a) * (one - b), a * (one - b), b * (one - a), a * b
        if mutation == "swap_w1_w2":
            w1, w2 = w2, w1
        X = np.ceil(x + eps).astype(np.int64) + pad
        Y = np.ceil(y + eps).astype(np.int64) + pad
        r_ = (Y - hp)[:, None, None] + ar[None, :, None]
        c_ = (X - hp)[:, None, None] + ar[None, None, :]
        A, B, Cc, D = I1[r_, c_], I1[r_, c_ - 1], I1[r_ - 1, c_], I1[r_ - 1, c_ - 1]
        if fma:
            r = _fma(w0, D, _fma(w1, Cc, _fma(w2, B, w3 * A))).reshape(len(x), -1)
        else:
            r = (((w3 * A + w2 * B) + w1 * Cc) + w0 * D).reshape(len(x), -1)
        if mutation == "drop_tap":
            r[:, 27] = 0
        mean = np.zeros(len(x), T)
        if norm and mutation != "no_mean" and not centred:
            if mode == "f64":
                mean = r.mean(1)
            elif mutation == "mean56":  # one of the 8 lanes' columns missing from the sum
                mean = _eigen_sum(np.where(np.arange(ps * ps) % ps == 3, f32(0), r)) / f32(ps * ps)
            else:
                mean = _eigen_sum(r) / f32(ps * ps)
            r = r - mean[:, None]
        return r, mean

    u = iu.astype(T)
    sx, sy = rx + u[:, 0], ry + u[:, 1]
    alive = ~oob(sx, sy)
    S = np.zeros(N)
    updates = np.zeros(N, np.int64)
    fragile = np.zeros(N, bool)
    if mode == "f64":
        sx32, sy32 = irx.astype(f32) + iu[:, 0], iry.astype(f32) + iu[:, 1]
        oob32 = (sx32 < f32(lb)) | (sy32 < f32(lb)) | (sx32 > f32(ubw)) | (sy32 > f32(ubh))
        fragile |= (oob32 == alive) | near_bound(sx, sy) | (sing != sing32)
        det = h00 * h11 - h01 * h01
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            hinv = np.maximum(np.abs(h11) + np.abs(h01), np.abs(h01) + np.abs(h00)) / np.abs(det)
        cond = hinv * np.maximum(np.abs(h00) + np.abs(h01), np.abs(h01) + np.abs(h11))
        gabs = np.abs(gdx) + np.abs(gdy)
    qx, qy = sx.copy(), sy.copy()
    for counter in range(1, it + 2):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        r, mean = warp(qx[idx], qy[idx])
        if mode == "f64":
            b0, b1 = (gdx[idx] * r).sum(1), (gdy[idx] * r).sum(1)
        else:
            if lpp2:
                b0, b1 = _lpp2_dot(gdx[idx], r, fma, fma), _lpp2_dot(gdy[idx], r, fma, fma)
            else:
                b0, b1 = _eigen_dot(gdx[idx], r, fma), _eigen_dot(gdy[idx], r, fma)
        d0, d1 = _lu_solve(h00[idx], h01[idx], h01[idx], h11[idx], b0, b1, mutation == "recip_wrong_row", recip, fma)
        with np.errstate(invalid="ignore", over="ignore"):
            u[idx, 0] = u[idx, 0] - d0
            u[idx, 1] = u[idx, 1] - d1
            nx, ny = rx[idx] + u[idx, 0], ry[idx] + u[idx, 1]
            ex, ey = sx[idx] - nx, sy[idx] - ny
            nrm = np.sqrt(ex * ex + ey * ey)
            bad = (nrm > thr) | oob(nx, ny) | (nrm != nrm)
        if mode == "f64":
            fragile[idx] |= near_integer(qx[idx]) | near_integer(qy[idx])
            fragile[idx] |= (np.abs(nrm - thr) < DELTA) | near_bound(nx, ny)
            S[idx] += hinv[idx] * (gabs[idx] * (np.abs(r) + np.abs(mean)[:, None])).sum(1)
            S[idx] += cond[idx] * np.maximum(np.abs(d0), np.abs(d1))
            updates[idx] += 1
        qx[idx], qy[idx] = nx, ny
        u[idx[bad]] = iu[idx[bad]].astype(T)
        alive[idx[bad]] = False
    if mode == "f32":
        return u
    return Trace(u, S, fragile, updates)


def rho(u, tr):
    """Normalised error of a result u (N, 2) against a Trace: (rho over the
    patches with S > 0, NaN elsewhere; mask of patches with S == 0 where u is
    not exactly the float64 result)."""
    err = np.abs(np.asarray(u, f64).reshape(-1, 2) - tr.u).max(1)
    flat = ~(tr.S > 0)  # S = 0, or not finite (cannot happen with a regularised H)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(flat, np.nan, err / (U24 * tr.S))
    return out, flat & (err != 0)


class Verdict:
    """max_y / med_y: the bound's yardstick figures (the larger over the
    yardstick set); max_y0 / med_y0: pyref.search_level's alone."""

    def __init__(self, ok, why, max_c, med_c, max_y, med_y, max_y0, med_y0, fragile_share, inexact_flat):
        self.ok, self.why = ok, why
        self.max_c, self.med_c, self.max_y, self.med_y = max_c, med_c, max_y, med_y
        self.max_y0, self.med_y0 = max_y0, med_y0
        self.fragile_share, self.inexact_flat = fragile_share, inexact_flat

    @staticmethod
    def _ratio(c, y):
        return c / y if y > 0 else (0.0 if c == 0 else np.inf)

    @property
    def max_ratio(self):  # over pyref.search_level
        return self._ratio(self.max_c, self.max_y0)

    @property
    def med_ratio(self):
        return self._ratio(self.med_c, self.med_y0)

    def __str__(self):
        return (f"rho max {self.max_c:.3g} (pyref {self.max_y0:.3g}, x{self.max_ratio:.2f}; set {self.max_y:.3g}) "
                f"median {self.med_c:.3g} (pyref {self.med_y0:.3g}, x{self.med_ratio:.2f}; set {self.med_y:.3g}) "
                f"fragile {self.fragile_share:.3%} flat-but-moved {self.inexact_flat}"
                + ("" if self.ok else f" REJECTED: {self.why}"))


def accept(u_cand, u_yards, tr, k=K):
    """The acceptance function: on the level's non-fragile patches,
    max rho_cand <= k max rho_yard and median rho_cand <= k median rho_yard,
    the fragile share <= 1 % of the level's patches, and u_cand exactly the
    float64 result wherever S = 0. u_yards: the yardstick's result, or a list
    of them (the yardstick set: pyref.search_level's first; the bound takes the
    larger max and the larger median over the set). -> Verdict."""
    if isinstance(u_yards, np.ndarray):
        u_yards = [u_yards]
    rc, flat_bad_c = rho(u_cand, tr)
    rys = [rho(u, tr)[0] for u in u_yards]
    keep = ~tr.fragile & ~np.isnan(rys[0])
    why = []
    bad_flat = int((flat_bad_c & ~tr.fragile).sum())
    if bad_flat:
        why.append(f"{bad_flat} patches with S = 0 are not exactly the float64 result")
    if tr.fragile_share > FRAGILE_CAP:
        why.append(f"fragile share {tr.fragile_share:.2%} > {FRAGILE_CAP:.0%}")
    if not keep.any():
        mc = dc = my = dy = my0 = dy0 = 0.0
    else:
        c = rc[keep]
        mc, dc = float(c.max()), float(np.median(c))
        maxs = [float(y[keep].max()) for y in rys]
        meds = [float(np.median(y[keep])) for y in rys]
        my, dy, my0, dy0 = max(maxs), max(meds), maxs[0], meds[0]
        if not np.isfinite(c).all():
            why.append("candidate not finite")
        if not mc <= k * my:
            why.append(f"max rho {mc:.3g} > {k} x {my:.3g}")
        if not dc <= k * dy:
            why.append(f"median rho {dc:.3g} > {k} x {dy:.3g}")
    return Verdict(not why, "; ".join(why), mc, dc, my, dy, my0, dy0, tr.fragile_share, bad_flat)
