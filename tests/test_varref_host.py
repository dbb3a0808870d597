"""CPU tests of the variational refinement's two restatements: the C oracle
(dis_oracle_var_refine, the specification of csrc/dis_varref.hip) against the
vectorised numpy one (pyref.var_refine), bit for bit, at every refined level
shape of the tile-edge matrix (tests/varref_cases.py); two known answers that
depend on neither; and the geometry of the matrix itself."""
import numpy as np
import pytest

import pyref
import varref_cases as vc

f32 = np.float32


def _bitexact(got, exp, what):
    got = np.ascontiguousarray(got, f32)
    exp = np.ascontiguousarray(exp, f32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got.view(np.uint32) != exp.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("shape", vc.all_level_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_var_refine_oracle_matches_numpy(oracle, shape):
    w, h = shape
    I0, I1 = vc.level_pair(w, h)
    for kind in vc.FLOWS:
        flow = vc.level_flow(w, h, kind)
        for fp in vc.VR:
            got = oracle.var_refine(I0, I1, flow, fp)
            _bitexact(got, pyref.var_refine(I0, I1, flow, fp), f"{w}x{h} {kind} fp {fp}")
            assert np.isfinite(got).all()
            assert not np.array_equal(got, flow), "the refinement left the flow as it was"


def test_the_far_flows_leave_the_frame_on_every_side():
    for w, h in vc.all_level_shapes():
        f = vc.level_flow(w, h, "far")
        yy, xx = np.mgrid[0:h, 0:w]
        X, Y = xx + f[..., 0], yy + f[..., 1]
        assert X.min() < -1 and X.max() > w and Y.min() < -1 and Y.max() > h, (w, h)
        assert np.abs(f).max() <= 20
        hv = vc.level_flow(w, h, "halves")
        assert np.array_equal(hv * 2, np.round(hv * 2))
        if w * h >= 64:
            assert (hv == np.round(hv)).any() and (hv != np.round(hv)).any()
        c = vc.level_flow(w, h, "const")
        assert (c == c[0, 0]).all()


@pytest.mark.parametrize("shape", [(3, 2), (9, 7), (33, 31), (109, 47)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_images_and_zero_flow_stay_zero(oracle, shape):
    # Iz, Ixz, Iyz and the smoothness term all vanish: B1 = B2 = 0 exactly, so
    # every SOR update is 0 whatever the weights are
    w, h = shape
    I0 = vc.level_pair(w, h)[0]
    zero = np.zeros((h, w, 2), f32)
    for fp in vc.VR:
        for refine in (oracle.var_refine, pyref.var_refine):
            out = refine(I0, I0, zero, fp)
            assert not out.any(), (refine.__module__, fp)


@pytest.mark.parametrize("a,b", [(3, -2), (-5, 1), (0, 4)])
def test_five_tap_derivative_of_a_plane_is_its_slope(a, b):
    # ((p(-2) - 8 p(-1)) + 8 p(1)) - p(2) of a*x + b*y along x is 12 a: every
    # intermediate is an integer below 2^24, and 12 a / 12 divides exactly
    w, h = 19, 11
    yy, xx = np.mgrid[0:h, 0:w]
    plane = (a * xx + b * yy + 40).astype(f32)
    dx, dy = pyref.d5(plane, 1), pyref.d5(plane, 0)
    assert dx.dtype == f32 and dy.dtype == f32
    assert (dx[:, 2:-2] == a).all() and (dy[2:-2, :] == b).all()
    # replicate border: the first column's taps are p0, p0, p1, p2 -> 6 a / 12;
    # the last column's p(n-3), p(n-2), p(n-1), p(n-1) -> the same
    assert (dx[:, 0] == a / 2).all() and (dx[:, -1] == a / 2).all()
    assert (dy[0, :] == b / 2).all() and (dy[-1, :] == b / 2).all()


# ---------------------------------------------------------------------------
# the matrix reaches what it is there for (constants of csrc/dis_varref.hip)
# ---------------------------------------------------------------------------
LIN_TILE = 32              # k_vr_lin: kLW = kLH
SOR_W, SOR_H = 108, 46     # k_vr_sor output tile: kSTW x kSTH
HALO_X, HALO_Y = 10, 9     # kSHX, kSHY: the region is 128 x 64
XCDS = 8                   # xcd_tile()


def _sor_tiles(w, h):
    return -(-w // SOR_W), -(-h // SOR_H)


def _interior_tiles(w, h):
    """Tiles that take sor_tile<true>: xs >= 1 && xs + 128 <= W - 1 && ys >= 1 && ys + 64 <= H - 1."""
    nx, ny = _sor_tiles(w, h)
    n = 0
    for by in range(ny):
        for bx in range(nx):
            xs, ys = bx * SOR_W - HALO_X, by * SOR_H - HALO_Y
            n += (xs >= 1 and xs + SOR_W + 2 * HALO_X <= w - 1 and ys >= 1 and ys + SOR_H + 2 * HALO_Y <= h - 1)
    return n


def test_the_matrix_reaches_every_path():
    shapes = {c.name: vc.level_shapes(c) for c in vc.MATRIX}
    flat = [s for ss in shapes.values() for s in ss]
    # with C = F = 0 the frame is the refined level
    for c in vc.MATRIX:
        if c.C == 0:
            assert shapes[c.name] == [(c.W, c.H)]
    assert shapes["tiny"] == [(24, 16), (12, 8), (6, 4), (3, 2)]
    assert shapes["ragged-c3"] == [(208, 152), (104, 76), (52, 38), (26, 19)]
    assert shapes["c2f1-b2"] == [(80, 60), (40, 30)]
    # the first level with a border-free SOR tile, and its neighbour with none
    assert _interior_tiles(227, 102) == 1 and (227, 102) in flat
    assert _interior_tiles(226, 101) == 0 and (226, 101) in flat
    # ... and the two shapes that miss it in one dimension only (an off-by-one in
    # either upper bound of the condition turns exactly one of them interior)
    assert _interior_tiles(227, 101) == 0 and (227, 101) in flat
    assert _interior_tiles(226, 102) == 0 and (226, 102) in flat
    assert _interior_tiles(227, 101 + 1) == 1 and _interior_tiles(226 + 1, 102) == 1
    assert [s for s in flat if _interior_tiles(*s)] == [(227, 102), (325, 139), (325, 139)]
    assert _interior_tiles(325, 139) == 1
    # tile counts (blocks of one k_vr_sor launch: tiles x pairs) around the XCD remap
    blocks = {c.name: _sor_tiles(*shapes[c.name][0])[0] * _sor_tiles(*shapes[c.name][0])[1] * c.batch
              for c in vc.MATRIX}
    assert blocks["9-tiles"] == 9 and blocks["18-tiles"] == 18      # tails of 1 and 2
    assert blocks["16-tiles"] == 16 and blocks["48-tiles"] == 48    # no tail
    assert any(n % XCDS == 0 for n in blocks.values())
    assert any(n >= 9 and n % XCDS for n in blocks.values())
    assert any(n < XCDS for n in blocks.values())
    assert blocks["sor-107x45"] == 1 and blocks["sor-108x46"] == 1 and blocks["sor-109x47"] == 4
    # pixel pairs per lane: odd widths leave half a pair outside the image
    assert any(w & 1 for w, _ in flat) and any(not w & 1 for w, _ in flat)
    # narrower than the 5-tap derivative in both dimensions
    assert any(w < 5 and h < 5 for w, h in flat)
    # k_vr_lin's tile edge -1, 0, +1 in both dimensions
    for edge in (LIN_TILE - 1, LIN_TILE, LIN_TILE + 1):
        assert any(w == edge for w, _ in flat) and any(h == edge for _, h in flat)
    assert (2 * LIN_TILE + 1, LIN_TILE + 1) in flat
    # the batches: synth and steps only; every case runs both refinement counts
    assert [c.name for c in vc.MATRIX if c.batch > 1] == ["18-tiles", "48-tiles", "c2f1-b2"]
    assert vc.VR == (1, 3)


def test_the_inputs_do_what_they_are_there_for(oracle):
    # on the oracle, one shape: `steps` drives the refined flow out of the frame,
    # `same` is moved by the refinement, `flat` stays exactly zero
    case = vc.BY_NAME["sor-109x47"]
    got = {}
    for kind in vc.INPUTS:
        I0, I1 = vc.frames(case, kind)
        assert not I0.flags.writeable and I0.shape == (1, case.H, case.W)
        refined = vc.oracle_levels(case, kind, 0, 3)[2][0]
        plain = vc.oracle_levels(case, kind, 0, 0)[2][0]
        got[kind] = (refined, plain)
    refined, plain = got["steps"]
    yy, xx = np.mgrid[0:case.H, 0:case.W]
    X, Y = xx + refined[..., 0], yy + refined[..., 1]
    assert X.min() < 0 or X.max() > case.W - 1 or Y.min() < 0 or Y.max() > case.H - 1
    assert set(np.unique(vc.frames(case, "steps")[0])) == {0, 255}
    assert np.array_equal(np.roll(vc.frames(case, "steps")[0][0], (-3, 2), (0, 1)), vc.frames(case, "steps")[1][0])
    refined, plain = got["same"]
    assert np.abs(refined - plain).max() > 0.1
    refined, plain = got["flat"]
    assert not refined.any() and not plain.any()
    refined, plain = got["synth"]
    assert not np.array_equal(refined, plain)
