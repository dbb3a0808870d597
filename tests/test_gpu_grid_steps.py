"""GPU parity at every patch-grid step: the HIP path against the CPU oracle,
float32 bit patterns, tolerance 0 (as tests/test_gpu_parity.py), at the grid
steps the rest of the suite never visits.

steps = max(1, floor(patch_size * (1 - patch_overlap))) selects much of the
kernel code: the covering coarse-patch ranges (floordiv_r by the step), the I0
region and LDS tile stride of k_search8<LPP>, the K = ceil(8 / steps)
instantiation of k_output, the patch stage of k_densify. The other files run
patch size 8 at steps 1, 2, 3, 4 and 8 (paper mode: 2, 3, 4) and the generic
sizes at steps 2 to 4. Here:

* patch size 8 at steps 5, 6 and 7, every kernel variant, both modes, half
  output, batches, refinement, the compat path, stage dumps;
* paper mode at steps 1 (up to 8 x 8 covering patches: the general vote loop,
  k_densify's paper branch) and 8 (one covering patch per pixel);
* the generic kernels (patch sizes 2 to 16, 12 and 14 among them) from step 1
  to step = patch size.

Every case names the step it is there for and asserts oracle.steps() gives it
before anything runs. tests/test_oracle.py pins the oracle itself to the numpy
restatement at these steps."""
import numpy as np
import pytest

import test_gpu_f16 as half
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

_bitexact = parity._assert_bitexact

# patch size 8: step -> overlap (exact in binary)
PS8_OVERLAP = {1: 0.875, 5: 0.375, 6: 0.25, 7: 0.125, 8: 0.0}
# set_variant: 0 auto, 3 / 2 / 4 / 5 = 2 / 4 / 8 / 1 lanes per patch, 6 one wave per patch,
# 9 = 2 lanes per patch with most blocks through the fallback list, 1 the generic kernels
REF_VARIANTS = ((0, "auto"), (3, "LPP2"), (2, "LPP4"), (4, "LPP8"), (5, "LPP1"), (6, "wave"), (9, "LPP2-fallback"),
                (1, "generic"))
PAPER_VARIANTS = ((0, "auto"), (1, "generic"), (3, "LPP2"), (2, "LPP4"), (4, "LPP8"), (5, "LPP1"),
                  (9, "LPP2-fallback"))  # paper mode has no wave-per-patch form (tests/test_gpu_parity.py)

_frames_cache = {}
_oracle_cache = {}


def _params(d, C, F, ps, it, overlap, norm=1, step=None, oracle=None, **kw):
    if step is not None:
        assert oracle.steps(ps, overlap) == step, (ps, overlap, step)
    return d.Params(coarsest_scale=C, finest_scale=F, patch_size=ps, iterations=it, patch_overlap=overlap,
                    patch_normalization=norm, **kw)


def _frames(d, W, H, kind, seed=0):
    """A related pair, or two unrelated frames (erratic coarse flow: spread
    blocks, the global-read paths); computed once, read-only."""
    key = (W, H, kind, seed)
    if key not in _frames_cache:
        s = 3 * W + H + 10 * seed
        if kind == "related":
            I0, I1 = d.synth_pair(s, W, H)
        else:
            I0, _ = d.synth_pair(s + 1, W, H)
            _, I1 = d.synth_pair(s + 2, W, H)
            I1 = np.ascontiguousarray(I1[::-1])
        I0.setflags(write=False)
        I1.setflags(write=False)
        _frames_cache[key] = (I0, I1)
    return _frames_cache[key]


def _oracle_flow(oracle, I0, I1, p, key):
    """The oracle's flow, once per (frames, knobs), shared and left unchanged."""
    k = (key, tuple(sorted(vars(p).items())))
    if k not in _oracle_cache:
        out = oracle.calc_from_params(I0, I1, p)
        out.setflags(write=False)
        _oracle_cache[k] = out
    return _oracle_cache[k]


def _levels(p):
    return range(p.finest_scale, p.coarsest_scale + 1)


def _run_variants(d, oracle, p, W, H, variants, what):
    eng = d.DenseInverseSearch(p, W, H)
    # variant 9 caps the usable tile at 24 pixels: at steps 5 to 7 any block of two patches is wider
    want_fallback = oracle.steps(p.patch_size, p.patch_overlap) in (5, 6, 7)
    for kind in ("related", "unrelated"):
        I0, I1 = _frames(d, W, H, kind)
        exp = _oracle_flow(oracle, I0, I1, p, (W, H, kind, 0))
        assert np.abs(exp).max() > 0.25, "a flow of zeros would prove nothing"
        for variant, name in variants:
            eng.set_variant(variant)
            _bitexact(eng.calc(I0, I1), exp, f"{what} {name} {kind}")
            if variant == 9 and kind == "related" and p.patch_size == 8 and want_fallback:
                listed = [eng.fallback_blocks(l) for l in _levels(p)]
                assert sum(listed) > 0, f"{what}: variant 9 listed no fallback block {listed}"
    eng.close()


# --- patch size 8, steps 5, 6, 7 ---------------------------------------------------------------

PS8_SHAPES = {
    # name: (W, H, C, F, iterations, normalisation, steps it runs at)
    "ragged-F0": (203, 151, 3, 0, 6, 1, (5, 6, 7)),   # levels 208 x 152 .. 26 x 19: partial 8 x 8 patch blocks
    "F1": (160, 120, 3, 1, 6, 1, (5, 6, 7)),          # k_output<true, 2>, the F == 1 interior-tile rows
    "F2": (200, 136, 3, 2, 6, 1, (6,)),
    "F1-raw": (160, 120, 3, 1, 6, 0, (5, 6, 7)),      # no normalisation
    "ragged-F0-it0": (203, 151, 3, 0, 0, 1, (7,)),    # iterations 0: one update
}
PS8_CASES = [(step, name) for name, c in PS8_SHAPES.items() for step in c[6]]


def _partial_blocks(oracle, Wp, Hp, C, F, st):
    """Levels whose patch grid has >= 2 blocks of 8 x 8 patches on both axes, the last ones partial."""
    out = []
    for l in range(F, C + 1):
        npw, nph, _, _ = oracle.grid(Wp >> l, Hp >> l, st)
        if npw > 8 and nph > 8 and npw % 8 and nph % 8:
            out.append((l, npw, nph))
    return out


@pytest.mark.parametrize("paper", [0, 1], ids=["reference", "paper"])
@pytest.mark.parametrize("step,shape", PS8_CASES, ids=[f"step{s}-{n}" for s, n in PS8_CASES])
def test_ps8_steps_5_6_7_every_variant(disflow_mod, oracle, step, shape, paper):
    # k_search8<LPP> (I0 region (bgx1 - bgx0) * st + 10 wide, tile strides of tile_layout at
    # this step), k_search8_fb, k_search_wave, k_search_generic<8>, and k_output<UPS, 2> at a
    # step that is not 4; related frames and unrelated ones
    W, H, C, F, it, norm, _ = PS8_SHAPES[shape]
    p = _params(disflow_mod, C, F, 8, it, PS8_OVERLAP[step], norm, step=step, oracle=oracle, paper_mode=paper)
    if shape.startswith("ragged"):
        Wp, Hp = oracle.padded_size(W, H, C)[:2]
        assert (Wp, Hp) == (208, 152)
        assert _partial_blocks(oracle, Wp, Hp, C, F, step), "no level with several, partial patch blocks"
    _run_variants(disflow_mod, oracle, p, W, H, PAPER_VARIANTS if paper else REF_VARIANTS,
                  f"ps 8 step {step} {shape} paper {paper}")


HALF_CASES = [(5, "ragged-F0", 3), (5, "F1", 4), (6, "ragged-F0", 4), (6, "F1", 0), (6, "F2", 3),
              (7, "ragged-F0", 0), (7, "F1", 3)]


@pytest.mark.parametrize("step,shape,variant", HALF_CASES, ids=[f"step{s}-{n}" for s, n, _ in HALF_CASES])
def test_ps8_steps_5_6_7_half_output(disflow_mod, oracle, step, shape, variant):
    # the __half2 instantiations of k_output<., 2>: the oracle's flow narrowed as tests/test_gpu_f16.py does
    W, H, C, F, it, norm, _ = PS8_SHAPES[shape]
    p = _params(disflow_mod, C, F, 8, it, PS8_OVERLAP[step], norm, step=step, oracle=oracle, paper_mode=0)
    I0, I1 = _frames(disflow_mod, W, H, "related")
    eng = disflow_mod.DenseInverseSearch(p, W, H, flow_dtype=np.float16)
    eng.set_variant(variant)
    got = eng.calc(I0, I1)
    eng.close()
    assert got.dtype == np.float16 and got.shape == (H, W, 2)
    half._assert_bits(got, half.narrow(_oracle_flow(oracle, I0, I1, p, (W, H, "related", 0))), f"step {step} {shape}")


def test_ps8_step_5_batch_of_three_on_two_streams(disflow_mod, oracle):
    W, H = 160, 120
    p = _params(disflow_mod, 3, 1, 8, 6, PS8_OVERLAP[5], step=5, oracle=oracle)
    pairs = [_frames(disflow_mod, W, H, "related", seed=k) for k in range(3)]
    I0 = np.stack([a for a, _ in pairs])
    I1 = np.stack([b for _, b in pairs])
    eng = disflow_mod.DenseInverseSearch(p, W, H, max_batch=3)
    eng.set_concurrency(2)
    got = eng.calc_batch(I0, I1)
    eng.close()
    for k in range(3):
        _bitexact(got[k], _oracle_flow(oracle, I0[k], I1[k], p, (W, H, "related", k)), f"step 5 pair {k}")


@pytest.mark.parametrize("paper", [0, 1], ids=["reference", "paper"])
def test_ps8_step_6_with_refinement(disflow_mod, oracle, paper):
    # refinement on: every level's dense field is materialised by k_densify at patch size 8
    # and step 6, and the search initialises from dense_coarse
    W, H = 160, 120
    p = _params(disflow_mod, 3, 1, 8, 6, PS8_OVERLAP[6], step=6, oracle=oracle, var_refine_iters=2, paper_mode=paper)
    I0, I1 = _frames(disflow_mod, W, H, "related")
    exp = _oracle_flow(oracle, I0, I1, p, (W, H, "related", 0))
    eng = disflow_mod.DenseInverseSearch(p, W, H)
    for variant, name in ((0, "auto"), (3, "LPP2"), (1, "generic")) + (() if paper else ((6, "wave"),)):
        eng.set_variant(variant)
        _bitexact(eng.calc(I0, I1), exp, f"step 6 refined {name} paper {paper}")
    eng.close()


@pytest.mark.parametrize("step", [5, 6, 7])
def test_ps8_steps_5_6_7_compat_constructor_path(disflow_mod, oracle, step):
    # caller-built physical planes: the kPhys kernels, which do not stage the I0 region
    W, H, C, F, it, ps = 160, 128, 3, 1, 6, 8
    ov = PS8_OVERLAP[step]
    assert oracle.steps(ps, ov) == step
    I0, I1 = _frames(disflow_mod, W, H, "related")
    Wp, Hp, P0, PX, PY, P1, _, _ = oracle.build_pyramids(I0, I1, C, ps)
    exp = oracle.flow_from_pyramids(P0, PX, PY, P1, ps, Wp, Hp, C, F, it, ps, ov, 1)
    for _ in range(2):  # the second call reuses the cached workspace
        got = disflow_mod.optical_flow_from_pyramids(P0, PX, PY, P1, ps, Wp, Hp, C, F, it, ps, ov, True)
        _bitexact(got, exp, f"compat flow step {step}")


@pytest.mark.parametrize("paper", [0, 1], ids=["reference", "paper"])
@pytest.mark.parametrize("step", [5, 7])
def test_ps8_steps_5_7_stage_dumps(disflow_mod, oracle, step, paper):
    # names the level and the stage of a difference, not just the final flow
    W, H, C, F, it, norm, _ = PS8_SHAPES["ragged-F0"]
    ov = PS8_OVERLAP[step]
    p = _params(disflow_mod, C, F, 8, it, ov, norm, step=step, oracle=oracle, paper_mode=paper)
    I0, I1 = _frames(disflow_mod, W, H, "related")
    eng = disflow_mod.DenseInverseSearch(p, W, H)
    eng.set_debug(True)
    eng.calc(I0, I1)
    Wp, Hp, P0, PX, PY, P1, _, _ = oracle.build_pyramids(I0, I1, C, 8)
    _, us, ds = oracle.flow_from_pyramids(P0, PX, PY, P1, 8, Wp, Hp, C, F, it, 8, ov, norm, capture=True, paper=paper)
    S = disflow_mod
    for l in range(C, F - 1, -1):  # coarse to fine: the first difference is the cause
        _bitexact(eng.debug_dump(S.STAGE_PATCH_U, l).reshape(-1, 2), us[l], f"step {step} patch u level {l}")
        _bitexact(eng.debug_dump(S.STAGE_DENSE, l).reshape(ds[l].shape), ds[l], f"step {step} dense level {l}")
    eng.close()


# --- paper mode at steps 1 and 8 ---------------------------------------------------------------

PAPER_EDGE_SHAPES = [(96, 80, 3, 1), (96, 80, 3, 0), (200, 136, 3, 2)]
PAPER_EDGE_VARIANTS = ((0, "auto"), (3, "LPP2"), (4, "LPP8"), (5, "LPP1"), (9, "LPP2-fallback"), (1, "generic"))


def _coverage(oracle, w, h, ps, st):
    """Patches covering each pixel of a w x h level: footprints [ref - ps/2, ref + ps/2) counted in numpy."""
    npw, nph, offw, offh = oracle.grid(w, h, st)
    cx, cy = np.zeros(w, np.int64), np.zeros(h, np.int64)
    for g in range(npw):
        cx[max(g * st + offw - ps // 2, 0):min(g * st + offw + ps // 2, w)] += 1
    for g in range(nph):
        cy[max(g * st + offh - ps // 2, 0):min(g * st + offh + ps // 2, h)] += 1
    return cy[:, None] * cx[None, :]


@pytest.mark.parametrize("W,H,C,F", PAPER_EDGE_SHAPES, ids=[f"{w}x{h}-F{f}" for w, h, _, f in PAPER_EDGE_SHAPES])
@pytest.mark.parametrize("step", [1, 8])
def test_paper_mode_steps_1_and_8(disflow_mod, oracle, step, W, H, C, F):
    # step 1: a coarse pixel is covered by up to 8 x 8 coarse patches (the general vote
    # loop of the weighted coarse-to-fine init, not its n <= 2 kPV form), k_output does
    # not fit and k_densify's paper branch runs. Step 8: one covering patch per pixel
    # (n == 1; LPP 1 does not fit its tile and runs as LPP 2).
    p = _params(disflow_mod, C, F, 8, 4, PS8_OVERLAP[step], step=step, oracle=oracle, paper_mode=1)
    Wp, Hp = oracle.padded_size(W, H, C)[:2]
    for l in _levels(p):
        n = _coverage(oracle, Wp >> l, Hp >> l, 8, step)
        if step == 8:
            # footprints of step = patch size tile the level whatever its size (the grid is
            # centred: tests/test_oracle.py test_step_equal_to_patch_size_tiles_every_level),
            # so no pixel is left uncovered and every one has exactly one vote
            assert n.min() == 1 and n.max() == 1, (l, n.min(), n.max())
        elif (Wp >> l) >= 16 and (Hp >> l) >= 16:
            assert n.max() == 64 and n.min() >= 16, (l, n.min(), n.max())  # 8 x 8 inside, 4 x 4 in the corners
    _run_variants(disflow_mod, oracle, p, W, H, PAPER_EDGE_VARIANTS, f"paper step {step} {W}x{H} F {F}")


# --- generic kernels: patch size x step ---------------------------------------------------------

GENERIC_OVERLAP = {
    2: {1: 0.5, 2: 0.0},
    4: {1: 0.75, 3: 0.25, 4: 0.0},
    6: {1: 0.75, 5: 0.1, 6: 0.0},
    10: {1: 0.875, 7: 0.25, 9: 0.05, 10: 0.0},
    12: {1: 0.875, 4: 0.625, 9: 0.25, 12: 0.0},
    14: {1: 0.875, 7: 0.5, 13: 0.05, 14: 0.0},
    16: {1: 0.9375, 5: 0.6875, 15: 0.0625, 16: 0.0},
}
GENERIC_CASES = [(ps, st) for ps, steps in GENERIC_OVERLAP.items() for st in steps]
GENERIC_MIDDLE = {2: 1, 4: 3, 6: 5, 10: 7, 12: 9, 14: 7, 16: 5}  # the step of the no-normalisation and paper cases


def _generic_case(d, oracle, ps, step, W, H, C, F, it, norm=1, paper=0, kind="related", flow_dtype=np.float32):
    p = _params(d, C, F, ps, it, GENERIC_OVERLAP[ps][step], norm, step=step, oracle=oracle, paper_mode=paper)
    I0, I1 = _frames(d, W, H, kind)
    exp = _oracle_flow(oracle, I0, I1, p, (W, H, kind, 0))
    assert np.abs(exp).max() > 0.25
    eng = d.DenseInverseSearch(p, W, H, flow_dtype=flow_dtype)
    got = eng.calc(I0, I1)
    eng.close()
    what = f"ps {ps} step {step} {W}x{H} C {C} F {F} norm {norm} paper {paper} {kind}"
    if flow_dtype == np.float16:
        half._assert_bits(got, half.narrow(exp), what)
    else:
        _bitexact(got, exp, what)


@pytest.mark.parametrize("ps,step", GENERIC_CASES, ids=[f"ps{p}-step{s}" for p, s in GENERIC_CASES])
def test_generic_patch_size_by_step(disflow_mod, oracle, ps, step):
    # k_search_generic<PS>, k_densify (floordiv_r by steps up to 16; at patch size 16 and
    # step 1 its largest patch stage and 256 covering patches per pixel, the last entry of
    # c_densify_rcp) and k_upsample_crop. 160 x 120: at patch size 16 and step 16 level 0
    # has 10 x 8 = 80 patches, more than one 64-lane block with a partial one.
    W, H, C, it = 160, 120, 2, 3
    if (ps, step) == (16, 16):
        assert oracle.grid(W, H, 16)[:2] == (10, 8)
    if (ps, step) == (16, 1):
        n = _coverage(oracle, W, H, 16, 1)
        # pixel x is covered by the patches at x - 7 .. x + 8: all 16 exist for x in [7, W - 9]
        assert n.max() == 256 and (n[7:H - 8, 7:W - 8] == 256).all()  # interior pixels: c_densify_rcp.r[256]
    for F in (0, 1):
        _generic_case(disflow_mod, oracle, ps, step, W, H, C, F, it)
        _generic_case(disflow_mod, oracle, ps, step, W, H, C, F, it, kind="unrelated")
    if step == GENERIC_MIDDLE[ps]:
        _generic_case(disflow_mod, oracle, ps, step, W, H, C, 1, it, norm=0)
    if step in (GENERIC_MIDDLE[ps], ps):
        for F in (0, 1):
            _generic_case(disflow_mod, oracle, ps, step, W, H, C, F, it, paper=1)
    if ps in (12, 16):  # k_upsample_crop<__half2>
        for F in (0, 1):
            _generic_case(disflow_mod, oracle, ps, step, W, H, C, F, it, flow_dtype=np.float16)


@pytest.mark.parametrize("ps,step", [(12, 9), (16, 1)], ids=["ps12-step9", "ps16-step1"])
def test_generic_patch_size_ragged(disflow_mod, oracle, ps, step):
    W, H, C, it = 203, 151, 3, 3
    for F in (0, 1):
        _generic_case(disflow_mod, oracle, ps, step, W, H, C, F, it)
