"""CPU tests of the level-by-level tolerance check's own machinery
(tests/searchref64.py, tests/fma_cases.py): the float64 level search against
the reference-order float32 one on the whole case matrix, the sensitivity of
the acceptance function to six ways a kernel could be wrong, the oracle's
own CPU rounding variants (oracle/Makefile `variants`) as candidates, and the
CPU reproduction of the one excess over K the GPU showed.

Every level starts from the exact pipeline's dense field of the level above
(fma_cases.oracle_starts). The figures are printed (pytest -s shows them)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fma_cases as fc
import oracle_binding as ob
import pyref
import searchref64 as s64

# a first-order scale with a worst-case constant of about log2(64) + the solve's
# few roundings: the yardstick's median rho above this would mean the float64
# search is not the function the float32 one computes, and every ratio vacuous
MEDIAN_RHO_SANITY = 10.0


def _levels(case):
    for k in range(case.batch):
        starts = fc.oracle_starts(case, k)
        for l in range(case.C, case.F - 1, -1):
            yield k, l, starts[l]


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_float64_against_f32(case):
    for k, l, init in _levels(case):
        tr, ys = fc.level_check(case, k, l, init)
        uy = ys[0]
        r, flat_moved = s64.rho(uy, tr)
        v = s64.accept(uy, uy, tr)
        print(f"{case.name} pair {k} level {l}: {len(uy)} patches, {tr.updates.mean():.2f} updates, "
              f"f32 rho max {v.max_y:.3g} median {v.med_y:.3g}, fragile {tr.fragile_share:.3%}, "
              f"S = 0 on {int((~(tr.S > 0)).sum())}")
        assert np.isfinite(r[tr.S > 0]).all()
        assert tr.fragile_share <= s64.FRAGILE_CAP
        assert not (flat_moved & ~tr.fragile).any(), "S = 0 but the float32 result is not the float64 one"
        assert v.ok, str(v)
        assert v.med_y <= MEDIAN_RHO_SANITY
        # the vectorised float32 search (the base of the mutations below) is pyref, bit for bit
        u32 = fc.reference(case, k, l, init, "f32")
        assert np.array_equal(u32.view(np.uint32), uy.view(np.uint32))


def test_tile_layout_table_for_every_grid_step():
    """The kernel table in tests/test_gpu_fma_levels.py (fma_cases.TILE_TABLE) against the
    Python restatement of tile_layout, for every grid step patch size 8 can have; every
    step is the step of some case, and launch_ts holds every stride 2 and 8 lanes per
    patch can get as a template constant (its run-time-stride default is never taken)."""
    assert {fc.steps(c) for c in fc.CASES} == set(range(1, 9)) == set(fc.TILE_TABLE)
    for st, (s1, s2, quad, s4, s8) in fc.TILE_TABLE.items():
        assert fc.lpp1_fits(st) == (s1 is not None), st
        if s1 is not None:
            assert fc.tile_layout(st, 1) == (s1, 0), st
        assert fc.tile_layout(st, 2) == (s2, quad), st
        assert fc.tile_layout(st, 4) == (s4, 0), st
        assert fc.tile_layout(st, 8) == (s8, 0), st
        assert s2 in fc.LAUNCH_TS_STRIDES and s8 in fc.LAUNCH_TS_STRIDES, st


@pytest.mark.parametrize("mutation", s64.MUTATIONS)
def test_acceptance_rejects_mutation(mutation):
    rejected = {}
    for case in fc.CASES:
        for k, l, init in _levels(case):
            tr, ys = fc.level_check(case, k, l, init)
            v = s64.accept(fc.reference(case, k, l, init, "f32", mutation), ys, tr)
            if not v.ok and v.max_c >= 10 * s64.K * v.max_y:
                rejected.setdefault(case.name, []).append((l, v.max_ratio, v.med_c))
            if mutation == "drop_tap" and case.name.startswith("shift"):
                assert v.med_c >= 700, (case.name, l, str(v))
    for name, rows in rejected.items():
        print(f"{mutation} {name}: " + ", ".join(f"level {l} max rho x{mr:.3g} median rho {md:.3g}" for l, mr, md in rows))
    assert len(rejected) >= 3, rejected


def _variant_lib(name):
    path = os.path.join(ob.ORACLE_DIR, f"libdis_oracle_{name}.so")
    src = os.path.join(ob.ORACLE_DIR, "dis_oracle.c")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", ob.ORACLE_DIR, "variants"])
    L = ctypes.CDLL(path)
    for fn, f in list(vars(ob.lib).items()):  # every prototype the binding declared (tools/tolerance.py)
        if fn.startswith("dis_oracle_"):
            getattr(L, fn).argtypes = f.argtypes
            getattr(L, fn).restype = f.restype
    return L


@pytest.mark.parametrize("case", [c for c in fc.CASES if not c.warm], ids=repr)
@pytest.mark.parametrize("variant", ["seqsum", "avxsum", "fma"])
def test_oracle_rounding_variants_accepted(variant, case, monkeypatch):
    """The oracle built with another reduction order (sequential; Eigen with
    AVX packets) or with FMA contraction, at the coarsest level: the start is
    zero there, so the variant's level-C search is level-isolated as it stands.
    The acceptance function must take all of them with K = 4.

    Measured against pyref.search_level alone: fma max rho x0.56 to x1.55, and
    two cases above K: seqsum shift-it0 level 2 max rho 1.09 against 0.197
    (x5.5, median x3.9), avxsum scene32-raw level 3 max rho 2.62 against 0.504
    (x5.2) -- levels of 35 patches whose zero start makes pyref's warp exact
    (integer positions), so its own max rho is unusually small. Against the
    yardstick set (searchref64.accept; the restated 2-lanes-per-patch tolerance
    arithmetic is its second member, see the last test) every case passes,
    those two at x3.4 and x3.7 of the set's max."""
    L = _variant_lib(variant)
    for k in range(case.batch):
        Wp, Hp, P0, PX, PY, P1, _, _ = fc.pyramids(case, k)
        C = case.C
        tr, ys = fc.level_check(case, k, C, None)
        with monkeypatch.context() as m:
            m.setattr(ob, "lib", L)
            _, us, _ = ob.flow_from_pyramids(P0, PX, PY, P1, fc.PS, Wp, Hp, C, C, case.it, fc.PS, case.ov,
                                             case.norm, capture=True)
        v = s64.accept(us[C], ys, tr)
        print(f"{variant} {case.name} pair {k} level {C}: {v}")
        assert v.ok, str(v)


def test_lpp2_restatement_reproduces_the_gpu_excess():
    """Why the yardstick set has a second member. On an MI355X the
    2-lanes-per-patch tolerance kernel (variants 3 and 9) gave, on bigshift
    pair 1 level 1 from its own level-2 result, max rho 3.11 against pyref's
    0.771 (x4.03 > K; median x1.22). searchref64's float32 restatement of that
    kernel's arithmetic (centred gradients, contracted products, reciprocal
    pivots, its summation order), cascaded on the CPU from the zero start of
    level 2, reproduces exactly those figures: the excess is rounding, not a
    wrong operand, and the restatement joins the yardstick set."""
    case, k = fc.BY_NAME["bigshift"], 1
    st = fc.steps(case)
    Wp, Hp = fc.pyramids(case, k)[:2]
    tr2, ys2 = fc.level_check(case, k, 2, None)
    dense = pyref.densify(ys2[1], s64.grid(Wp >> 2, Hp >> 2, st), Wp >> 2, Hp >> 2, fc.PS, st)
    init = s64.start_from_dense(dense, Wp >> 1, Hp >> 1, st)
    tr, ys = fc.level_check(case, k, 1, init)
    v = s64.accept(ys[1], ys[0], tr)
    print(f"restated k_search8<2, kFma>, bigshift pair 1 level 1 against pyref alone: {v}")
    assert not v.ok and v.max_c > s64.K * v.max_y0
    assert abs(v.max_c - 3.11) < 0.01 and abs(v.max_y0 - 0.771) < 0.001  # the GPU's figures
