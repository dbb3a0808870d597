"""Variational refinement on the GPU, level by level, bit for bit, at the
shapes where k_vr_d0 / k_vr_lin / k_vr_sor (csrc/dis_varref.hip) change path
(tests/varref_cases.py; tests/test_varref_host.py checks that the matrix
reaches them).

The recipe is test_gpu_fma_levels.py's with the precision left exact: for
every case, input and refinement count, every level's dense dump must equal the
oracle's refinement of the densification of the GPU's OWN patch dump of that
level -- so a mismatch names the level and names refinement, not the search --
and around it the pyramid planes, the patch displacements and the returned
flow must equal the oracle's. With C = F = 0 the frame is the refined level,
which is how each tile-edge shape is reached.

Inputs: value noise (synth), a 0 / 255 block pattern whose refined flow leaves
the frame (steps), identical random frames (same) and constant frames (flat:
zero flow, refinement has nothing to move).
"""
import numpy as np
import pytest

import pyref
import varref_cases as vc

pytestmark = pytest.mark.gpu


def _bitexact(got, exp, what):
    got = np.ascontiguousarray(got, np.float32)
    exp = np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got.view(np.uint32) != exp.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _params(d, case, vr):
    return d.Params(coarsest_scale=case.C, finest_scale=case.F, patch_size=vc.PS, iterations=vc.IT,
                    patch_overlap=vc.OV, patch_normalization=vc.NORM, var_refine_iters=vr)


@pytest.mark.parametrize("vr", vc.VR, ids=lambda v: f"vr{v}")
@pytest.mark.parametrize("case", vc.MATRIX, ids=repr)
def test_refinement_level_by_level(disflow_mod, oracle, case, vr):
    d = disflow_mod
    C, F = case.C, case.F
    st = oracle.steps(vc.PS, vc.OV)
    Wp, Hp, pl, pt = oracle.padded_size(case.W, case.H, C)
    p = _params(d, case, vr)
    eng = d.DenseInverseSearch(p, case.W, case.H, max_batch=case.batch)
    eng.set_debug(True)
    if case.batch > 1:
        eng.set_concurrency(2)
    try:
        for kind in vc.inputs_of(case):
            I0, I1 = vc.frames(case, kind)
            flow = eng.calc_batch(I0, I1)
            moved = False
            for k in range(case.batch):
                what = f"{case.name} {kind} vr {vr} pair {k}"
                py0, py1 = vc.pyramids(case, kind, k)[6:]
                flowF, us, ds = vc.oracle_levels(case, kind, k, vr)
                for l in range(C + 1):
                    shape = py0[l][0].shape
                    _bitexact(eng.debug_dump(d.STAGE_IMG0, l, k).reshape(shape), py0[l][0], f"{what}: img0 l{l}")
                    _bitexact(eng.debug_dump(d.STAGE_IMG1, l, k).reshape(shape), py1[l][0], f"{what}: img1 l{l}")
                dense = {}
                for l in range(C, F - 1, -1):  # coarse to fine: the first mismatch is the cause
                    w, h = Wp >> l, Hp >> l
                    _bitexact(eng.debug_dump(d.STAGE_DX0, l, k).reshape(h, w), py0[l][1], f"{what}: dx l{l}")
                    _bitexact(eng.debug_dump(d.STAGE_DY0, l, k).reshape(h, w), py0[l][2], f"{what}: dy l{l}")
                    u = eng.debug_dump(d.STAGE_PATCH_U, l, k).reshape(-1, 2)
                    plain = pyref.densify(u, oracle.grid(w, h, st), w, h, vc.PS, st)
                    dense[l] = eng.debug_dump(d.STAGE_DENSE, l, k).reshape(h, w, 2)
                    _bitexact(dense[l], oracle.var_refine(py0[l][0], py1[l][0], plain, vr), f"{what}: dense l{l}")
                    _bitexact(u, us[l], f"{what}: patch u l{l}")
                    _bitexact(dense[l], ds[l], f"{what}: dense l{l} against the oracle's scale loop")
                    moved = moved or not np.array_equal(dense[l].view(np.uint32), plain.view(np.uint32))
                _bitexact(dense[F], flowF, f"{what}: finest dense")
                _bitexact(flow[k], oracle.upsample_crop(dense[F], Wp, Hp, F, pl, pt, case.W, case.H), f"{what}: flow")
                _bitexact(flow[k], oracle.calc_from_params(I0[k], I1[k], p), f"{what}: flow against calc")
            if kind == "flat":
                assert not flow.any(), f"{case.name} flat vr {vr}: constant frames gave a flow"
            else:
                assert moved, f"{case.name} {kind} vr {vr}: no level's dense dump differs from its densification"
    finally:
        eng.close()


def test_refinement_graphs_across_a_call_sequence(disflow_mod, oracle):
    """The refinement launches of a (direction, sub-batch, level) are replayed as
    a graph keyed by (pairs, first pair): batch sizes, eager timing and the
    stream count change between calls on one engine, and every result is the
    oracle's."""
    d = disflow_mod
    case = vc.Case("sequence", 217, 93, 0, 0, 3)
    p = _params(d, case, 3)
    I0, I1 = vc.frames(case, "synth")
    exp = np.stack([oracle.calc_from_params(I0[k], I1[k], p) for k in range(3)])
    assert not np.array_equal(exp[0], exp[1]) and not np.array_equal(exp[1], exp[2])
    eng = d.DenseInverseSearch(p, case.W, case.H, max_batch=3)
    try:
        eng.set_concurrency(2)
        _bitexact(eng.calc_batch(I0, I1), exp, "n = 3 on 2 streams")
        _bitexact(eng.calc_batch(I0[:1], I1[:1]), exp[:1], "n = 1")
        _bitexact(eng.calc_batch(I0[:2], I1[:2]), exp[:2], "n = 2")
        eng.set_kernel_timing(True)
        _bitexact(eng.calc_batch(I0, I1), exp, "n = 3, kernel timing (eager)")
        n_lin, n_sor = eng.kernel_time(d.KERNEL_VR_LIN)[0], eng.kernel_time(d.KERNEL_VR_SOR)[0]
        assert n_lin == n_sor and n_lin > 0 and n_lin % 3 == 0, (n_lin, n_sor)  # timed launches: the eager path ran
        eng.set_kernel_timing(False)
        _bitexact(eng.calc_batch(I0, I1), exp, "n = 3 after kernel timing")
        eng.set_concurrency(1)
        _bitexact(eng.calc_batch(I0, I1), exp, "n = 3 on 1 stream")
    finally:
        eng.close()
