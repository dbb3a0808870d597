"""Tolerance mode (DIS_PRECISION_FMA), level by level, at rounding scale.

In tolerance mode only the search kernels differ from the exact pipeline: the
kFma instantiations of k_search8<LPP> / k_search8_fb<LPP> (iterate,
iterate_split, patch_dot, warp_patch, the centred gradients of search_block).
Everything around them -- pyramid, the fused densification that starts a
level, k_densify, k_vr_*, k_output / the upsample -- is the exact code. So for
every case and lane layout:

* the surroundings are held bit for bit: the image and gradient dumps to the
  oracle's pyramid, each level's dense dump to the exact densification (and
  refinement) of the GPU's OWN patch dump of that level, the returned flow to
  the oracle's upsample of the finest dense dump -- no exclusions;
* each level's search is checked on its own: tests/searchref64.py (float64)
  and the yardstick set -- pyref.search_level (reference-order float32) and
  the float32 restatement of the 2-lanes-per-patch tolerance arithmetic, which
  joined after reproducing on the CPU the one excess over K the GPU showed
  (tests/test_search64_host.py) -- run from the start the GPU's
  level really had: 2 * dense(l + 1)[ry >> 1, rx >> 1] of the exact
  densification of the GPU's u_{l+1} (the refined dump under refinement; the
  caller's init plane at a warm coarsest level; zero at a cold one).
  searchref64.accept (K = 4 over the yardstick on max and median rho, fragile
  share <= 1 %) judges the GPU's u_l; the figures are printed. On top of
  that every layout must equal the float32 restatement of its own arithmetic
  bit for bit (searchref64 styles: centred gradients, contracted products,
  reciprocal pivots; the 1 / 4 / 8-lane kernels sum in Eigen's order, the
  2-lane kernel in iterate_split's) -- a wrong lane, weight or mean cannot
  hide in any tolerance then;
* the FMA kernels really ran: some patch differs from the exact mode's dump,
  and variant 9 lists fallback blocks.

Which kernel a case reaches (patch size 8; tile_layout of dis_search8.hip
restated: grid step -> LDS tile stride per lanes-per-patch layout, and the
LPP-2 half-wave layout). Restated, not read from the library, which exports
neither search8_tile_stride nor search8_tile_quad: fma_cases.tile_layout is
the restatement, fma_cases.TILE_TABLE this table, and
tests/test_search64_host.py holds the two together on the CPU.

    steps (overlap)      LPP 1   LPP 2        LPP 4   LPP 8
    1 (0.8)              100     72 (4 x 4)   68      72
    2 (0.75)             98      66 (2 x 8)   66      68
    3 (0.625)            100     72 (4 x 4)   68      72
    4 (0.5)              97      65 (2 x 8)   65      66
    5 (0.375)            100     72 (4 x 4)   68      72
    6 (0.25)             98      66 (2 x 8)   66      68
    7 (0.125)            100     72 (4 x 4)   68      72
    8 (0.0)              LPP 2   65 (2 x 8)   65      65

Variants 3 / 2 / 4 / 5 force 2 / 4 / 8 / 1 lanes per patch, 9 is LPP 2 with
most blocks through the fallback list (k_search8_fb<2, kFma>), 0 picks per
level (8 lanes here: every level is below kLpp8MaxPatches). These are all
eight grid steps patch size 8 can have, so together this is every kFma
instantiation launch_search8_t<false, true> can launch, each at every step
that reaches it: launch_ts only specialises LPP 2 and 8, over strides 65 /
66 / 68 / 72, which are the only strides the table gives those two layouts
at any step, so its run-time-stride default is unreachable at patch size 8
(steps 5 to 7 reach the 72, 66 / 68 and 72 instantiations that steps 1 to 3
reach, at wider I0 regions). Paper mode, other patch sizes and the
wave-per-patch kernel always run the exact kernels and are bit-exact
elsewhere (tests/test_gpu_parity.py, tests/test_gpu_grid_steps.py).
"""
import numpy as np
import pytest

import fma_cases as fc
import initref
import pyref
import searchref64 as s64

pytestmark = pytest.mark.gpu

VARIANTS = {0: "auto", 3: "LPP2", 2: "LPP4", 4: "LPP8", 5: "LPP1", 9: "LPP2-fallback"}
FALLBACK_CASES = ("shift-it0", "shift-it3", "bigshift", "scene31", "shift-step5")
PARAMS = [(c, v) for c in fc.CASES for v in VARIANTS if v != 9 or c.name in FALLBACK_CASES]
MEDIAN_RHO_SANITY = 10.0  # tests/test_search64_host.py

_exact = {}


def _bitexact(got, exp, what):
    got = np.ascontiguousarray(got, np.float32)
    exp = np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got.view(np.uint32) != exp.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _engine(d, case, fma, variant):
    p = d.Params(coarsest_scale=case.C, finest_scale=case.F, patch_size=fc.PS, iterations=case.it,
                 patch_overlap=case.ov, patch_normalization=case.norm, var_refine_iters=case.vr)
    eng = d.DenseInverseSearch(p, case.W, case.H, max_batch=case.batch)
    eng.set_precision(d.PRECISION_FMA if fma else d.PRECISION_EXACT)
    eng.set_variant(variant)
    eng.set_debug(True)
    if case.batch > 1:
        eng.set_concurrency(2)
    I0, I1 = fc.frames(case)
    if case.warm:
        flow = eng.calc_batch(I0, I1, init=fc.warm_plane(case), init_kind="coarse")
    else:
        flow = eng.calc_batch(I0, I1)
    return eng, flow


def _patch_dumps(d, eng, case):
    return {(k, l): eng.debug_dump(d.STAGE_PATCH_U, l, k).reshape(-1, 2)
            for k in range(case.batch) for l in range(case.F, case.C + 1)}


def _exact_dumps(d, case):
    if case.name not in _exact:
        eng, _ = _engine(d, case, False, 0)
        _exact[case.name] = _patch_dumps(d, eng, case)
        eng.close()
    return _exact[case.name]


@pytest.mark.parametrize("case,variant", PARAMS, ids=lambda x: VARIANTS[x] if isinstance(x, int) else repr(x))
def test_fma_search_level_by_level(disflow_mod, oracle, case, variant):
    d = disflow_mod
    eng, flow = _engine(d, case, True, variant)
    st, C, F = fc.steps(case), case.C, case.F
    u_gpu = _patch_dumps(d, eng, case)
    pl, pt = oracle.padded_size(case.W, case.H, C)[2:]
    rejected = []
    # 2 lanes per patch (iterate_split's order): asked for, or LPP 1 not fitting its tile at grid step 8
    lpp2 = variant in (3, 9) or (variant == 5 and st == 8)
    for k in range(case.batch):
        Wp, Hp, P0, PX, PY, P1, py0, py1 = fc.pyramids(case, k)
        # --- the exact surroundings, bit for bit
        for l in range(C + 1):
            _bitexact(eng.debug_dump(d.STAGE_IMG0, l, k).reshape(py0[l][0].shape), py0[l][0], f"img0 l{l} pair {k}")
            _bitexact(eng.debug_dump(d.STAGE_IMG1, l, k).reshape(py1[l][0].shape), py1[l][0], f"img1 l{l} pair {k}")
        dense = {}
        for l in range(F, C + 1):
            w, h = Wp >> l, Hp >> l
            _bitexact(eng.debug_dump(d.STAGE_DX0, l, k).reshape(h, w), py0[l][1], f"dx l{l} pair {k}")
            _bitexact(eng.debug_dump(d.STAGE_DY0, l, k).reshape(h, w), py0[l][2], f"dy l{l} pair {k}")
            exp = pyref.densify(u_gpu[k, l], s64.grid(w, h, st), w, h, fc.PS, st)
            if case.vr:
                exp = oracle.var_refine(py0[l][0], py1[l][0], exp, case.vr)
            dense[l] = eng.debug_dump(d.STAGE_DENSE, l, k).reshape(h, w, 2)
            _bitexact(dense[l], exp, f"dense l{l} pair {k}")
        _bitexact(flow[k], oracle.upsample_crop(dense[F], Wp, Hp, F, pl, pt, case.W, case.H), f"flow pair {k}")
        # --- the search, level by level, from the start the GPU's level had
        for l in range(C, F - 1, -1):
            w, h = Wp >> l, Hp >> l
            if l < C:
                init = s64.start_from_dense(dense[l + 1], w, h, st)
            elif case.warm:
                init = s64.start_from_dense(initref.sanitize(fc.warm_plane(case)[k]), w, h, st)
            else:
                init = None
            tr, ys = fc.level_check(case, k, l, init)
            v = s64.accept(u_gpu[k, l], ys, tr)
            restated = fc.fma_restatement(case, k, l, init, lpp2)
            same = (u_gpu[k, l].view(np.uint32) == restated.view(np.uint32)).all(1)
            print(f"FMA-LEVEL {case.name} {VARIANTS[variant]} pair {k} level {l} patches {len(same)}: {v}; "
                  f"{int((~same).sum())} patches differ from the restated {'LPP-2' if lpp2 else 'Eigen-order'} arithmetic")
            assert v.med_y0 <= MEDIAN_RHO_SANITY, "the float64 search does not track the yardstick"
            if not v.ok:
                rejected.append(f"pair {k} level {l}: {v}")
            if not same.all():  # every kFma kernel is its restatement, bit for bit
                rejected.append(f"pair {k} level {l}: {int((~same).sum())} patches differ from the restated arithmetic")
    # --- the FMA kernels ran
    exact = _exact_dumps(d, case)
    assert any(not np.array_equal(u_gpu[key].view(np.uint32), exact[key].view(np.uint32)) for key in u_gpu), \
        "FMA mode ran the exact kernels"
    if variant == 9:
        assert sum(eng.fallback_blocks(l) for l in range(F, C + 1)) > 0, "variant 9 listed no fallback block"
    eng.close()
    assert not rejected, "\n".join(rejected)
