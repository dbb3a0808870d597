"""GPU tests of the f16 flow format (dis_set_flow_format, dis_flow_convert;
include/dis_abi.h): the one narrowing function on every rounding boundary, each
flow writer (k_output's three store sites, k_upsample_crop) against the oracle's
flow narrowed, the f16 readers (warm start), the host pipeline, the graph
cache, the error paths and the C++ facade.

Flows are compared as 16-bit patterns (view(np.uint16)); where a NaN is
expected, NaN-ness is compared instead of bits. `narrow` is numpy's
astype(float16): round to nearest even, subnormals kept, |v| >= 65520 -> inf."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fbref
import initref
import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")
f16, f32 = np.float16, np.float32


def narrow(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, f32).astype(f16)


def _assert_bits(got, exp, what):
    """Same dtype, shape and bit patterns; NaNs match NaNs of any payload."""
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.dtype == e.dtype, f"{what}: dtype {g.dtype} vs {e.dtype}"
    assert g.shape == e.shape, f"{what}: shape {g.shape} vs {e.shape}"
    u = {2: np.uint16, 4: np.uint32, 1: np.uint8}[g.dtype.itemsize]
    bad = g.view(u) != e.view(u)
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(e))
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ; first at {list(idx)} "
                             f"got {g[idx]!r} ({int(g.view(u)[idx]):#x}) exp {e[idx]!r} ({int(e.view(u)[idx]):#x})")


def _params(S, C, F, **kw):
    kw.setdefault("iterations", 8)
    return S.Params(coarsest_scale=C, finest_scale=F, **kw)


def _pairs(S, seed, W, H, n):
    ps = [S.synth_pair(seed + k, W, H) for k in range(n)]
    return np.stack([a for a, _ in ps]), np.stack([b for _, b in ps])


_oracle_cache = {}


def oracle_flow(oracle, I0, I1, p):
    """The oracle's float flow of one pair, computed once per (frames, knobs) and never changed."""
    key = (I0.tobytes(), I1.tobytes(), I0.shape, tuple(sorted(vars(p).items())))
    if key not in _oracle_cache:
        out = oracle.calc_from_params(I0, I1, p)
        out.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


# ---------------------------------------------------------------------------
# 1. the conversion, exhaustively
# ---------------------------------------------------------------------------
def _narrowing_inputs():
    """f32 inputs around every rounding boundary of binary16: for each pair of
    adjacent finite halves the midpoint (a tie), its f32 neighbours on both
    sides and the two halves themselves, both signs; the subnormal range and
    below; +-0; the overflow boundary; inf and NaN."""
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(f16).astype(f32)  # +0 .. 65504, ascending
    lo, hi = h[:-1], h[1:]
    mid = (lo + hi) * f32(0.5)  # exact: 12 significant bits
    assert np.all((mid > lo) & (mid < hi))
    pos = np.concatenate([lo, hi, mid, np.nextafter(mid, f32(-np.inf)), np.nextafter(mid, f32(np.inf))])
    tiny = f32(2.0) ** np.arange(-30, -13).astype(f32)  # 2^-24 is the smallest subnormal half, 2^-25 ties to 0
    tiny = np.concatenate([tiny, np.nextafter(tiny, f32(0)), np.nextafter(tiny, f32(1)), tiny * f32(1.5),
                           np.array([1e-45, 1e-40, 1.1754944e-38, 5.9604645e-08, 2.9802322e-08, 2.9802326e-08], f32)])
    top = np.array([65504.0, 65519.996, 65520.0, 65536.0, 1e9, 3.4028235e38], f32)
    assert top[1] < f32(65520.0)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], f32)
    special = np.concatenate([special, np.array([0x7f800001, 0xffc12345], np.uint32).view(f32)])  # NaN payloads
    body = np.concatenate([pos, tiny, top])
    return np.concatenate([body, -body, special]).astype(f32)


def test_widening_is_exact_for_every_bit_pattern(disflow_mod):
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(f16)
    _assert_bits(disflow_mod.flow_convert(allh, f32), allh.astype(f32), "f16 -> f32, host pointers")
    _assert_bits(disflow_mod.flow_convert(allh, f16), allh, "f16 -> f16 copies")


def test_narrowing_matches_numpy_on_every_rounding_boundary_host(disflow_mod):
    x = _narrowing_inputs()
    assert x.size > 300000
    got = disflow_mod.flow_convert(x, f16)
    assert got.dtype == f16 and got.shape == x.shape
    _assert_bits(got, narrow(x), "f32 -> f16, host pointers")
    # (the cases the contract names, spelled out)
    one = disflow_mod.flow_convert(np.array([65519.996, 65520.0, -65520.0, 1e9, 2.0 ** -25, 2.0 ** -24, -0.0], f32), f16)
    assert one.view(np.uint16).tolist() == [0x7bff, 0x7c00, 0xfc00, 0x7c00, 0x0000, 0x0001, 0x8000]
    _assert_bits(disflow_mod.flow_convert(x, f32), x, "f32 -> f32 copies")


@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 1), (1, 0), (3, 1)],
                         ids=["aligned", "both-offset-one-value", "source-offset", "offsets-3-1"])
def test_conversion_on_device_pointers(disflow_mod, src_off, dst_off):
    # (1, 1): both buffers one value past an aligned base -- the kernel peels a
    # head and runs its vector body; (1, 0) and (3, 1): no common alignment, so
    # every value goes through the scalar path. Sentinels guard both ends.
    import torch
    S = disflow_mod
    x = _narrowing_inputs()
    n = x.size
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    src = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    src[src_off:src_off + n] = torch.from_numpy(x).to(dev)
    dst = torch.full((n + 8,), 7.0, dtype=torch.float16, device=dev)
    torch.cuda.synchronize()
    S.flow_convert_device(src[src_off:].data_ptr(), f32, dst[dst_off:].data_ptr(), f16, n, stream=s.cuda_stream)
    s.synchronize()
    out = dst.cpu().numpy()
    _assert_bits(out[dst_off:dst_off + n], narrow(x), "f32 -> f16, device pointers")
    assert (out[:dst_off] == 7).all() and (out[dst_off + n:] == 7).all(), "wrote outside the destination"
    # ... and back: every bit pattern, widened
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(f16)
    hsrc = torch.zeros(65536 + 8, dtype=torch.float16, device=dev)
    hsrc[dst_off:dst_off + 65536] = torch.from_numpy(allh).to(dev)
    wide = torch.full((65536 + 8,), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    S.flow_convert_device(hsrc[dst_off:].data_ptr(), f16, wide[src_off:].data_ptr(), f32, 65536, stream=s.cuda_stream)
    s.synchronize()
    w = wide.cpu().numpy()
    _assert_bits(w[src_off:src_off + 65536], allh.astype(f32), "f16 -> f32, device pointers")
    assert (w[:src_off] == 7).all() and (w[src_off + 65536:] == 7).all(), "wrote outside the destination"


# ---------------------------------------------------------------------------
# 2. k_output against the oracle
# ---------------------------------------------------------------------------
# F = 1 interior-tile path (out_rows_f1): an output tile is 64 x 64 pixels at
# F >= 1 (kOutTW x kOutTH, csrc/dis_output.hip) and takes that path when it
# lies inside W x H, none of its taps is clamped and the base allows the
# two-pixel stores. The kernel has one instantiation per parity of
# (pad_top - 1, pad_left - 1). Geometry (make_geometry, restated by
# initref.padded_size) pads to a multiple of 2^C and puts pad / 2 on the left /
# top; with C = 2 a size of 132 has pad 0 and 66 has pad 2 -> pad_left 1, so
# {66, 132}^2 covers the four parities. They are the smallest even sizes that
# do and still hold an interior tile and ragged border tiles: with pad 0 tile 0
# fails `ox + pad_left >= 1`, so the interior tile is tile 1 and the size must
# exceed 128 + 2; with pad_left 1 it is tile 0 and the size must exceed 64.
# _interior_tiles restates the kernel's condition; the test asserts all this.
F1_SIZES = [(66, 66), (132, 66), (66, 132), (132, 132)]


def _interior_tiles(W, H, C):
    Wp, Hp, pl, pt = initref.padded_size(W, H, C)
    wF, hF = Wp // 2, Hp // 2
    xmax = next((d for d in range(Wp) if max(int(np.floor((d + 0.5) * 0.5 - 0.5)), 0) + 1 >= wF), Wp)
    tiles = []
    for oy in range(0, H, 64):
        for ox in range(0, W, 64):
            xh, yh = ox + 63 + pl, oy + 63 + pt
            if (ox + 64 <= W and oy + 64 <= H and ox + pl >= 1 and oy + pt >= 1 and ((xh - 1) >> 1) + 1 <= wF - 1 and
                    ((yh - 1) >> 1) + 1 <= hF - 1 and xh < xmax):
                tiles.append((ox, oy))
    return tiles, ((pt - 1) & 1, (pl - 1) & 1)


def test_f1_sizes_cover_the_four_parities_with_interior_and_ragged_tiles():
    seen = set()
    for W, H in F1_SIZES:
        tiles, parity = _interior_tiles(W, H, 2)
        assert tiles and W % 64 and H % 64 and W % 2 == 0, (W, H, tiles)
        seen.add(parity)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


OUTPUT_CASES = {
    **{f"F1-{W}x{H}": (W, H, 2, 1, {}) for W, H in F1_SIZES},
    "F0-131x37-odd-width": (131, 37, 2, 0, {}),  # W odd: one 4-byte store per pixel; ragged tile rows
    "F2-96x80": (96, 80, 3, 2, {}),
    "paper-F1-132x66": (132, 66, 2, 1, dict(paper_mode=1)),
}


@pytest.mark.parametrize("case", sorted(OUTPUT_CASES))
def test_output_kernel_equals_narrowed_oracle(disflow_mod, oracle, case):
    S = disflow_mod
    W, H, C, F, kw = OUTPUT_CASES[case]
    p = _params(S, C, F, **kw)
    I0, I1 = S.synth_pair(500 + W + H, W, H)
    eng = S.DenseInverseSearch(p, W, H, flow_dtype=f16)
    got = eng.calc(I0, I1)
    eng.close()
    assert got.dtype == f16 and got.shape == (H, W, 2)
    exp = oracle_flow(oracle, I0, I1, p)
    assert np.abs(exp).max() > 0.5, "a flow of zeros would prove nothing"
    _assert_bits(got, narrow(exp), case)


def test_output_to_a_4_byte_aligned_pointer(disflow_mod, oracle):
    # 4-byte but not 8-byte aligned: the per-pixel store path on a size whose
    # aligned run takes the two-pixel stores and the interior-tile path
    import torch
    S = disflow_mod
    W, H = 132, 66
    p = _params(S, 2, 1)
    I0, I1 = S.synth_pair(500 + W + H, W, H)
    dev = torch.device("cuda:0")
    d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
    buf = torch.full((4 + H * W * 2 + 4,), 7.0, dtype=torch.float16, device=dev)
    out = buf[2:]
    assert out.data_ptr() % 8 == 4
    eng = S.DenseInverseSearch(p, W, H, flow_dtype=f16)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.calc_device(1, d0.data_ptr(), d1.data_ptr(), out.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    eng.close()
    b = buf.cpu().numpy()
    _assert_bits(b[2:2 + H * W * 2].reshape(H, W, 2), narrow(oracle_flow(oracle, I0, I1, p)), "misaligned output")
    assert (b[:2] == 7).all() and (b[2 + H * W * 2:] == 7).all(), "wrote outside the flow"


def test_batch_of_three_on_two_streams(disflow_mod, oracle):
    # sub-batch k's output offset is counted in halves
    S = disflow_mod
    W, H, n = 66, 66, 3
    p = _params(S, 2, 1)
    I0, I1 = _pairs(S, 40, W, H, n)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, flow_dtype=f16)
    eng.set_concurrency(2)
    got = eng.calc_batch(I0, I1)
    eng.close()
    assert got.dtype == f16
    for k in range(n):
        _assert_bits(got[k], narrow(oracle_flow(oracle, I0[k], I1[k], p)), f"pair {k}")


# ---------------------------------------------------------------------------
# 3. k_upsample_crop (generic patch sizes, refinement)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F,kw", [(0, dict(patch_size=4)), (1, dict(patch_size=4)), (1, dict(var_refine_iters=2))],
                         ids=["ps4-F0", "ps4-F1", "refine-F1"])
def test_upsample_crop_equals_narrowed_oracle(disflow_mod, oracle, F, kw):
    S = disflow_mod
    W, H = 64, 48
    p = _params(S, 2, F, **kw)
    I0, I1 = scenes.scene_pair(11, W, H)
    eng = S.DenseInverseSearch(p, W, H, flow_dtype=f16)
    got = eng.calc(I0, I1)
    eng.close()
    exp = oracle_flow(oracle, I0, I1, p)
    assert np.abs(exp).max() > 0.25
    _assert_bits(got, narrow(exp), f"F {F} {kw}")


# ---------------------------------------------------------------------------
# 4. flat frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,C,F", [(132, 66, 2, 1), (131, 37, 2, 0)])
def test_flat_frames_give_positive_zero_halves(disflow_mod, W, H, C, F):
    S = disflow_mod
    flat = np.full((H, W), 128, np.uint8)
    eng = S.DenseInverseSearch(_params(S, C, F), W, H, flow_dtype=f16)
    got = eng.calc(flat, flat)
    eng.close()
    assert got.dtype == f16 and not got.view(np.uint16).any()


# ---------------------------------------------------------------------------
# 5. bidirectional
# ---------------------------------------------------------------------------
def test_bidir_equals_narrowed_oracle_and_masks_from_widened_flows(disflow_mod, oracle):
    S = disflow_mod
    W, H = 160, 120
    p = _params(S, 3, 1, iterations=12)
    a, b = scenes.scene_pair(3, W, H)
    eng = S.DenseInverseSearch(p, W, H, flow_dtype=f16)
    fw, bw, mfw, mbw = eng.calc_bidir_batch(a[None], b[None], consistency=True)
    one_fw, one_bw = eng.calc_bidir(a, b)
    eng.close()
    assert fw.dtype == f16 and bw.dtype == f16
    _assert_bits(fw[0], narrow(oracle_flow(oracle, a, b, p)), "forward")
    _assert_bits(bw[0], narrow(oracle_flow(oracle, b, a, p)), "backward")
    _assert_bits(one_fw, fw[0], "calc_bidir forward")
    _assert_bits(one_bw, bw[0], "calc_bidir backward")
    wfw, wbw = fw.astype(f32), bw.astype(f32)
    _assert_bits(mfw[0], fbref.check(wfw[0], wbw[0])[0], "forward mask")
    _assert_bits(mbw[0], fbref.check(wbw[0], wfw[0])[0], "backward mask")
    assert set(np.unique(mfw)) == {0, 255}


# ---------------------------------------------------------------------------
# 6. warm start
# ---------------------------------------------------------------------------
WW, WH, WC = 72, 40, 2


def _warm_setup(S):
    p = _params(S, WC, 0, iterations=6, patch_overlap=0.5)
    frames = [scenes.scene_pair(20 + k, WW, WH) for k in range(2)]
    e16 = S.DenseInverseSearch(p, WW, WH, flow_dtype=f16)
    e32 = S.DenseInverseSearch(p, WW, WH)
    h = e16.calc(*frames[0])
    return p, frames, e16, e32, h


def test_flow_to_init_reads_halves(disflow_mod):
    S = disflow_mod
    p, frames, e16, e32, h = _warm_setup(S)
    _assert_bits(e16.flow_to_init(h), initref.flow_to_init(h.astype(f32), WC), "flow_to_init of an f16 flow")
    # a corner of inf / NaN halves: sanitised to 0 after the widening
    bad = h.copy()
    bad[:3, :3] = np.array([np.inf, np.nan], f16)
    bad[3, 0] = np.array([-np.inf, 65504.0], f16)
    _assert_bits(e16.flow_to_init(bad), initref.flow_to_init(bad.astype(f32), WC), "with inf / NaN halves")
    e16.close()
    e32.close()


def test_warm_start_from_an_f16_flow(disflow_mod):
    S = disflow_mod
    p, frames, e16, e32, h = _warm_setup(S)
    I0, I1 = frames[1]
    cold = e16.calc(I0, I1)
    for name, init in (("previous output", h), ("with inf / NaN", None)):
        if init is None:
            init = h.copy()
            init[:3, :3] = np.array([np.inf, np.nan], f16)
        got = e16.calc(I0, I1, init=init)
        assert got.dtype == f16
        _assert_bits(got, narrow(e32.calc(I0, I1, init=init.astype(f32))), f"warm start, {name}")
    assert not np.array_equal(e16.calc(I0, I1, init=h).view(np.uint16), cold.view(np.uint16)), "the init had no effect"
    e16.close()
    e32.close()


def test_warm_start_in_place_on_the_device(disflow_mod):
    # flow in, flow out: the f16 output buffer of the previous pair is the init
    import torch
    S = disflow_mod
    p, frames, e16, e32, h = _warm_setup(S)
    I0, I1 = frames[1]
    dev = torch.device("cuda:0")
    d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
    buf = torch.from_numpy(h.copy()).to(dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    e16.calc_device(1, d0.data_ptr(), d1.data_ptr(), buf.data_ptr(), stream=s.cuda_stream, init_ptr=buf.data_ptr())
    s.synchronize()
    _assert_bits(buf.cpu().numpy(), narrow(e32.calc(I0, I1, init=h.astype(f32))), "init == flow")
    e16.close()
    e32.close()


def test_track_yields_float16_chained_calls(disflow_mod):
    S = disflow_mod
    p = _params(S, WC, 0, iterations=6, patch_overlap=0.5)
    seq = [scenes.scene_pair(20, WW, WH)[0], *[scenes.scene_pair(20 + k, WW, WH)[1] for k in range(3)]]
    e16 = S.DenseInverseSearch(p, WW, WH, flow_dtype=f16)
    got = list(e16.track(seq))
    prev = None
    for k, g in enumerate(got):
        assert g.dtype == f16
        prev = e16.calc(seq[k], seq[k + 1], init=prev)
        _assert_bits(g, prev, f"track pair {k}")
    assert len(got) == 3
    e16.close()


# ---------------------------------------------------------------------------
# 7. host pipeline
# ---------------------------------------------------------------------------
class _Pinned:
    """A numpy view of dis_host_alloc'd (page-locked) memory."""

    def __init__(self, S, shape, dtype):
        self.L = S.lib()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.p = ctypes.c_void_p()
        S._check(self.L.dis_host_alloc(nbytes, ctypes.byref(self.p)))
        buf = (ctypes.c_char * nbytes).from_address(self.p.value)
        self.a = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        self.a = None
        self.L.dis_host_free(self.p)


def test_host_pipeline_three_chunks(disflow_mod, oracle):
    import torch
    S = disflow_mod
    W, H, n = 132, 66, 5
    p = _params(S, 2, 1)
    I0, I1 = _pairs(S, 70, W, H, n)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, flow_dtype=f16)
    # the device path's result
    d0, d1 = torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda()
    out = torch.zeros((n, H, W, 2), dtype=torch.float16, device="cuda")
    st = torch.cuda.current_stream()
    eng.calc_device(n, d0.data_ptr(), d1.data_ptr(), out.data_ptr(), st.cuda_stream)
    st.synchronize()
    exp = out.cpu().numpy()
    _assert_bits(exp[0], narrow(oracle_flow(oracle, I0[0], I1[0], p)), "device path, pair 0")
    eng.set_host_pipeline(2)  # chunks of 2, 2 and 1 pairs
    got = eng.calc_batch(I0, I1)
    _assert_bits(got, exp, "pageable buffers")
    info = eng.host_pipeline_info()
    assert info["chunk_pairs"] == 2 and info["last_chunks"] == 3 and info["last_direct_out"] == 0, info
    b0, b1, fo = _Pinned(S, I0.shape, np.uint8), _Pinned(S, I1.shape, np.uint8), _Pinned(S, (n, H, W, 2), f16)
    b0.a[:], b1.a[:] = I0, I1
    fo.a.view(np.uint16)[:] = 0x7e00
    eng.calc_batch_host(n, b0.a.ctypes.data, b1.a.ctypes.data, fo.a.ctypes.data)
    _assert_bits(fo.a.copy(), exp, "page-locked buffers")
    info = eng.host_pipeline_info()
    assert info["last_chunks"] == 3 and info["last_direct_in"] == 1 and info["last_direct_out"] == 1, info
    # a format change rebuilds the pipe: float flows through the same engine
    eng.set_flow_format(f32)
    back = eng.calc_batch(I0, I1)
    assert back.dtype == f32
    _assert_bits(back[n - 1], oracle_flow(oracle, I0[n - 1], I1[n - 1], p), "F32 after F16, last pair")
    assert eng.host_pipeline_info()["last_chunks"] == 3
    eng.close()
    for b in (b0, b1, fo):
        b.free()


def test_host_pipeline_auto_chunk_doubles(disflow_mod):
    # about 64 MB of flow per chunk: 1920 x 1080 float flows are 4 pairs, half flows 8
    S = disflow_mod
    W, H, n = 1920, 1080, 9
    p = S.preset_params(S.Preset.ULTRAFAST, W, H)
    I0, I1 = _pairs(S, 1, W, H, 1)
    I0, I1 = np.repeat(I0, n, 0), np.repeat(I1, n, 0)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, flow_dtype=f16)
    got = eng.calc_batch(I0, I1)
    info = eng.host_pipeline_info()
    assert info["chunk_pairs"] == 8 and info["last_chunks"] == 2, info
    _assert_bits(got[n - 1], got[0], "the last chunk's pair equals the first's")
    eng.set_flow_format(f32)
    eng.calc_batch(I0[:5], I1[:5])
    info = eng.host_pipeline_info()
    assert info["chunk_pairs"] == 4 and info["last_chunks"] == 2, info
    eng.close()


# ---------------------------------------------------------------------------
# 8. graph cache
# ---------------------------------------------------------------------------
def test_graph_cache_is_keyed_by_the_format(disflow_mod, oracle):
    # same device buffers in F32, F16, F32, two calls each (capture, replay):
    # a graph captured for one store type is never replayed for the other
    import torch
    S = disflow_mod
    W, H, n = 132, 66, 2
    p = _params(S, 2, 1)
    I0, I1 = _pairs(S, 70, W, H, n)
    exp32 = np.stack([oracle_flow(oracle, I0[k], I1[k], p) for k in range(n)])
    dev = torch.device("cuda:0")
    d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
    out = torch.zeros((n, H, W, 2), dtype=torch.float32, device=dev)
    half_view = out.view(torch.float16).reshape(-1)  # the same memory as halves
    nh = n * H * W * 2                               # the f16 extent, in halves
    eng = S.DenseInverseSearch(p, W, H, max_batch=n)
    eng.set_graphs(True)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for fmt in (f32, f16, f32):
        eng.set_flow_format(fmt)
        for rep in range(2):
            with torch.cuda.stream(s):
                out.fill_(-7.0)
            eng.calc_device(n, d0.data_ptr(), d1.data_ptr(), out.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            if fmt is f32:
                _assert_bits(out.cpu().numpy(), exp32, f"F32 call {rep}")
            else:
                hv = half_view.cpu().numpy()
                _assert_bits(hv[:nh].reshape(n, H, W, 2), narrow(exp32), f"F16 call {rep}")
                tail = out.cpu().numpy().reshape(-1)[nh // 2:]
                assert (tail == -7.0).all(), "an F16 call wrote past the f16 extent"
    eng.close()


# ---------------------------------------------------------------------------
# 9. errors, and the default
# ---------------------------------------------------------------------------
def test_errors(disflow_mod):
    import torch
    S = disflow_mod
    L = S.lib()
    W, H = 64, 48
    p = _params(S, 2, 0)
    eng = S.DenseInverseSearch(p, W, H)
    for bad in (2, -1, 16):
        assert L.dis_set_flow_format(eng._ctx, bad) == S.DIS_ERR_INVALID_ARGUMENT
        assert b"DIS_FLOW" in L.dis_last_error()
    assert L.dis_set_flow_format(None, 1) == S.DIS_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        eng.set_flow_format(np.float64)
    assert eng.flow_dtype == f32
    I0, I1 = S.synth_pair(9, W, H)
    z16, z32 = np.zeros((H, W, 2), f16), np.zeros((H, W, 2), f32)
    with pytest.raises(ValueError):
        eng.calc(I0, I1, init=z16)  # an f16 init on a float32 engine
    eng.set_flow_format(f16)
    with pytest.raises(ValueError):
        eng.calc(I0, I1, init=z32)  # a float32 fullres init on a float16 engine
    iw, ih = eng.init_plane_size()
    with pytest.raises(ValueError):
        eng.calc(I0, I1, init=np.zeros((ih, iw, 2), f16), init_kind="coarse")  # coarse planes stay float32
    with pytest.raises(ValueError):
        eng.flow_to_init(z32)
    assert eng.calc(I0, I1, init=np.zeros((ih, iw, 2), f32), init_kind="coarse").dtype == f16
    # a 2-byte aligned device flow pointer
    dev = torch.device("cuda:0")
    d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
    buf = torch.zeros(H * W * 2 + 8, dtype=torch.float16, device=dev)
    other = torch.zeros(H * W * 2 + 8, dtype=torch.float16, device=dev)
    odd, odd2 = buf[1:].data_ptr(), other[1:].data_ptr()
    assert odd % 4 == 2 and odd2 % 4 == 2
    for call in (lambda: eng.calc_device(1, d0.data_ptr(), d1.data_ptr(), odd),
                 lambda: eng.calc_device(1, d0.data_ptr(), d1.data_ptr(), buf.data_ptr(), init_ptr=odd2),
                 lambda: eng.calc_device(1, d0.data_ptr(), d1.data_ptr(), odd, init_ptr=other.data_ptr())):
        with pytest.raises(S.DisError) as e:
            call()
        assert e.value.status == S.DIS_ERR_INVALID_ARGUMENT and "4-byte" in str(e.value)
    two = torch.zeros(2 * H * W * 2 + 8, dtype=torch.float16, device=dev)
    with pytest.raises(S.DisError) as e:
        eng.calc_bidir_device(1, d0.data_ptr(), d1.data_ptr(), two.data_ptr(), two[H * W * 2 + 1:].data_ptr())
    assert e.value.status == S.DIS_ERR_INVALID_ARGUMENT
    # the two f16 outputs may be as close as one f16 flow, not one float flow
    eng.calc_bidir_device(1, d0.data_ptr(), d1.data_ptr(), two.data_ptr(), two[H * W * 2:].data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(S.DisError):
        eng.calc_bidir_device(1, d0.data_ptr(), d1.data_ptr(), two.data_ptr(), two[H * W * 2 - 2:].data_ptr())
    # dis_flow_convert
    x = torch.zeros(16, dtype=torch.float32, device=dev)
    y = torch.zeros(16, dtype=torch.float16, device=dev)
    with pytest.raises(S.DisError):
        S.flow_convert_device(x.data_ptr() + 2, f32, y.data_ptr(), f16, 4)
    with pytest.raises(S.DisError):
        S.flow_convert_device(x.data_ptr(), f32, y.data_ptr() + 1, f16, 4)
    eng.close()
    with pytest.raises(ValueError):
        S.DenseInverseSearch(p, W, H, flow_dtype=np.int16)


def test_default_engine_still_returns_float32_bit_exact(disflow_mod, oracle):
    # a guard only: the existing suite is the real check that F32 is unchanged
    S = disflow_mod
    W, H = 132, 66
    p = _params(S, 2, 1)
    I0, I1 = S.synth_pair(500 + W + H, W, H)
    eng = S.DenseInverseSearch(p, W, H)
    got = eng.calc(I0, I1)
    eng.close()
    assert got.dtype == f32 and eng.flow_dtype == f32
    _assert_bits(got, oracle_flow(oracle, I0, I1, p), "default format")


# ---------------------------------------------------------------------------
# 10. FMA precision
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("conc", [1, 2])
def test_fma_mode_f16_is_its_own_f32_narrowed(disflow_mod, conc):
    # FMA mode is not bit-pinned to the oracle (only within a tolerance of it),
    # so the statement available is: the F16 output equals narrow() of the same
    # engine's F32 output in the same mode, for the same n and concurrency
    S = disflow_mod
    W, H, n = 132, 66, 3
    p = _params(S, 2, 1)
    I0, I1 = _pairs(S, 70, W, H, n)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n)
    eng.set_precision(S.PRECISION_FMA)
    eng.set_concurrency(conc)
    wide = eng.calc_batch(I0, I1)
    eng.set_flow_format(f16)
    got = eng.calc_batch(I0, I1)
    eng.close()
    assert wide.dtype == f32 and got.dtype == f16
    _assert_bits(got, narrow(wide), f"FMA, concurrency {conc}")


# ---------------------------------------------------------------------------
# the C++ facade
# ---------------------------------------------------------------------------
def test_cpp_facade_f16(disflow_mod, oracle, tmp_path):
    S = disflow_mod
    W, H = 160, 120  # tests/cpp/test_f16.cpp: the MEDIUM preset on synth pair 7
    I0, I1 = S.synth_pair(7, W, H)
    ref = tmp_path / "oracle_flow.f32"
    oracle.calc_from_params(I0, I1, S.preset_params(S.Preset.MEDIUM, W, H)).tofile(str(ref))
    exe = str(tmp_path / "test_f16")
    lib_dir = os.path.join(PKG, "disflow")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_f16.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(ref)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
