"""GPU tests of flow composition and point advection (dis_flow_compose,
dis_flow_advect_points): the kernels against their numpy restatement
(tests/composeref.py) on host arrays and on device pointers in every layout
that selects another load / store form, in place, through
DenseInverseSearch.track(accumulate=True), end to end on a sequence whose
content moves by whole pixels, the C++ facade and the CLI's --accumulate.
Every comparison is bit for bit."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import composeref
import warpref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")

F32, F16 = np.float32, np.float16
_BITS = {np.dtype(F32): np.uint32, np.dtype(F16): np.uint16, np.dtype(np.uint8): np.uint8}


def _assert_same(got, exp, what):
    """Equal shapes, dtypes and bit patterns (NaN compares by its bits)."""
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    gb, eb = g.view(_BITS[g.dtype]), e.view(_BITS[e.dtype])
    bad = gb != eb
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ; first at {idx[0].tolist()} "
                             f"got {gb[tuple(idx[0])]:#x} exp {eb[tuple(idx[0])]:#x}")


# (W, H, n): a single pixel; an odd W with a short last lane and no vector form;
# every form on short rows; an odd W over many rows; every vector form; many rows
SHAPES = [(1, 1, 1), (5, 3, 2), (16, 4, 1), (67, 33, 3), (64, 8, 2), (160, 120, 2)]
TRIPLES = [(F32, F32, F32), (F16, F16, F32)]  # (a, b, out) at every shape
ALL_TRIPLES = list(itertools.product((F32, F16), repeat=3))  # at (67, 33, 3)
PLANES = list(itertools.product((False, True), repeat=2))  # (valid_a, mask_b) given or not
_inputs = {}
_expected = {}


def _name(t):
    return "/".join(np.dtype(d).name for d in t)


def triples_of(shape):
    return ALL_TRIPLES if shape == (67, 33, 3) else TRIPLES


def inputs(W, H, n):
    """Two stacks of flows uniform in +-6 px (border pixels leave the frame on
    their own) with a handful of NaN, +-1e9, 2e9 and +-inf vectors each, as
    float32 and narrowed to float16, and two byte planes with about a fifth of
    zeros (other bytes 1..255): made once, never changed."""
    key = (W, H, n)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * W + 10 * H + n)
        bad = [(np.nan, np.nan), (1e9, -1e9), (-1e9, 2.0), (np.inf, 0.5), (1.0, -np.inf), (0.0, np.nan), (2e9, 0.0)]
        fields = {}
        for name in ("a", "b"):
            flow = rng.uniform(-6, 6, (n, H, W, 2)).astype(F32)
            flat = flow.reshape(-1, 2)
            pos = rng.choice(flat.shape[0], size=min(len(bad), flat.shape[0] // 8), replace=False)
            for j, q in enumerate(pos):
                flat[q] = bad[j]
            with np.errstate(over="ignore"):
                flow16 = flow.astype(F16)  # (+-1e9 become +-inf: still invalid)
            fields[name] = {np.dtype(F32): flow, np.dtype(F16): flow16}
        planes = [np.where(rng.random((n, H, W)) < 0.2, 0, rng.integers(1, 256, (n, H, W))).astype(np.uint8)
                  for _ in range(2)]
        for arr in list(fields["a"].values()) + list(fields["b"].values()) + planes:
            arr.setflags(write=False)
        _inputs[key] = (fields["a"], fields["b"], planes[0], planes[1])
    return _inputs[key]


def expected(shape, triple, use_va, use_mb):
    """The restatement's (out, valid_out) of one case: computed once, never changed."""
    key = (shape, tuple(np.dtype(d) for d in triple), use_va, use_mb)
    if key not in _expected:
        a, b, va, mb = inputs(*shape)
        out, valid = composeref.compose(a[np.dtype(triple[0])], b[np.dtype(triple[1])], va if use_va else None,
                                        mb if use_mb else None, triple[2])
        out.setflags(write=False)
        valid.setflags(write=False)
        _expected[key] = (out, valid)
    return _expected[key]


# ---------------------------------------------------------------------------
# host arrays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compose_matches_restatement_host(disflow_mod, shape):
    a, b, va, mb = inputs(*shape)
    for triple in triples_of(shape):
        fa, fb = a[np.dtype(triple[0])], b[np.dtype(triple[1])]
        for use_va, use_mb in PLANES:
            what = f"{_name(triple)}, valid_a {use_va}, mask_b {use_mb}"
            out, valid = expected(shape, triple, use_va, use_mb)
            kw = dict(valid_a=va if use_va else None, mask_b=mb if use_mb else None, out_dtype=triple[2])
            got, got_valid = disflow_mod.flow_compose(fa, fb, with_valid=True, **kw)
            _assert_same(got, out, "out, " + what)
            _assert_same(got_valid, valid, "valid_out, " + what)
            _assert_same(disflow_mod.flow_compose(fa, fb, **kw), out, "out without valid_out, " + what)
    W, H, n = shape
    if W * H * n >= 1000:  # a kernel that ignores an argument cannot pass
        t = TRIPLES[0]
        sets = {p: expected(shape, t, *p)[1] == 255 for p in PLANES}
        assert sets[(False, False)].any() and not sets[(False, False)].all()
        assert sets[(False, False)].sum() > sets[(True, False)].sum() > sets[(True, True)].sum()
        assert sets[(False, False)].sum() > sets[(False, True)].sum() > sets[(True, True)].sum()
        assert not np.array_equal(expected(shape, TRIPLES[0], False, False)[0].view(np.uint32),
                                  expected(shape, TRIPLES[1], False, False)[0].view(np.uint32))
    # one field of a stack: the wrapper's (H, W, 2) form
    out, valid = expected(shape, TRIPLES[0], True, True)
    one, one_valid = disflow_mod.flow_compose(a[np.dtype(F32)][0], b[np.dtype(F32)][0], valid_a=va[0], mask_b=mb[0],
                                              with_valid=True)
    _assert_same(one, out[0], "one (H, W, 2) field")
    _assert_same(one_valid, valid[0], "one field's valid_out")


# ---------------------------------------------------------------------------
# device pointers
# ---------------------------------------------------------------------------
def _offset_tensor(torch, host, lead, fill=7):
    """`host` (a flat numpy array) on the device, `lead` elements into a fresh
    allocation (allocations are at least 256-byte aligned)."""
    t = torch.full((lead + host.size,), fill, dtype=torch.from_numpy(host[:1].copy()).dtype, device="cuda:0")[lead:]
    t.copy_(torch.from_numpy(host.copy()))
    return t


def _fresh(torch, count, dtype, lead, fill=9):
    tdt = {np.dtype(F32): torch.float32, np.dtype(F16): torch.float16, np.dtype(np.uint8): torch.uint8}[np.dtype(dtype)]
    return torch.full((lead + count,), fill, dtype=tdt, device="cuda:0")[lead:]


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compose_matches_restatement_device(disflow_mod, shape, layout):
    # device pointers (torch tensors) on a caller's stream. aligned: every vector
    # form the shape allows; offset: the fields one (u,v) pair in and the byte
    # planes 1 byte in, so no vector form applies
    import torch
    W, H, n = shape
    a, b, va, mb = inputs(*shape)
    lead = 1 if layout == "offset" else 0
    px = n * H * W
    s = torch.cuda.Stream()
    ta = {d: _offset_tensor(torch, f.reshape(-1), 2 * lead, fill=0) for d, f in a.items()}
    tb = {d: _offset_tensor(torch, f.reshape(-1), 2 * lead, fill=0) for d, f in b.items()}
    tva, tmb = _offset_tensor(torch, va.reshape(-1), lead), _offset_tensor(torch, mb.reshape(-1), lead)
    assert tva.data_ptr() % 16 == lead and tmb.data_ptr() % 16 == lead
    for d in ta:
        assert ta[d].data_ptr() % 16 == 2 * lead * d.itemsize and tb[d].data_ptr() % 16 == 2 * lead * d.itemsize
    for triple in triples_of(shape):
        da, db, do = (np.dtype(d) for d in triple)
        for (use_va, use_mb), with_valid in itertools.product(PLANES, (True, False)):
            tout = _fresh(torch, 2 * px, do, 2 * lead)
            tvalid = _fresh(torch, px, np.uint8, lead)
            torch.cuda.synchronize()
            disflow_mod.flow_compose_device(ta[da].data_ptr(), da, tb[db].data_ptr(), db, n, W, H, tout.data_ptr(),
                                            out_dtype=do, valid_a_ptr=tva.data_ptr() if use_va else 0,
                                            mask_b_ptr=tmb.data_ptr() if use_mb else 0,
                                            valid_out_ptr=tvalid.data_ptr() if with_valid else 0, stream=s.cuda_stream)
            s.synchronize()
            out, valid = expected(shape, triple, use_va, use_mb)
            what = f"{_name(triple)}, valid_a {use_va}, mask_b {use_mb}"
            _assert_same(tout.cpu().numpy().reshape(n, H, W, 2), out, "out, " + what)
            if with_valid:
                _assert_same(tvalid.cpu().numpy().reshape(n, H, W), valid, "valid_out, " + what)
            else:
                assert bool((tvalid == 9).all()), "valid_out written though not asked for"
    # the inputs are as they were
    for d in ta:
        _assert_same(ta[d].cpu().numpy().reshape(n, H, W, 2), a[d], "a after the calls")
        _assert_same(tb[d].cpu().numpy().reshape(n, H, W, 2), b[d], "b after the calls")
    _assert_same(tva.cpu().numpy().reshape(n, H, W), va, "valid_a after the calls")
    _assert_same(tmb.cpu().numpy().reshape(n, H, W), mb, "mask_b after the calls")


def test_compose_rejects_misaligned_device_fields(disflow_mod):
    import torch
    f = [torch.zeros(64, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    p = [t.data_ptr() for t in f]
    for k in range(3):
        for dtype, off in ((F32, 4), (F16, 2)):
            q = list(p)
            q[k] += off
            dts = [F32, F32, F32]
            dts[k] = dtype
            with pytest.raises(disflow_mod.DisError) as e:
                disflow_mod.flow_compose_device(q[0], dts[0], q[1], dts[1], 1, 2, 2, q[2], out_dtype=dts[2])
            assert e.value.status == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    pts = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    for args in ((p[0] + 4, F32, pts.data_ptr(), p[1]), (p[0] + 2, F16, pts.data_ptr(), p[1]),
                 (p[0], F32, pts.data_ptr() + 4, p[1]), (p[0], F32, pts.data_ptr(), p[1] + 4)):
        with pytest.raises(disflow_mod.DisError) as e:
            disflow_mod.advect_points_device(args[0], args[1], 1, 2, 2, args[2], 3, args[3])
        assert e.value.status == disflow_mod.DIS_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------
# in place
# ---------------------------------------------------------------------------
def _fold(fields, dtypes):
    """The restatement's fold of a chain: acc_1 = field 0 as float32 with valid
    all 255, then acc_k = compose(acc_{k-1}, field k, valid_{k-1})."""
    acc = fields[0].astype(F32)
    valid = np.full(acc.shape[:-1], 255, np.uint8)
    for f, d in zip(fields[1:], dtypes[1:]):
        with np.errstate(over="ignore"):
            acc, valid = composeref.compose(acc, f.astype(d), valid, None, F32)
    return acc, valid


@pytest.mark.parametrize("shape", [(67, 33, 3), (64, 8, 2)], ids=lambda s: "x".join(map(str, s)))
def test_chain_of_four_fields_folds_in_place(disflow_mod, shape):
    # out == a and valid_out == valid_a on device pointers, the pair flows in
    # f32, f16, f32: one accumulator follows the chain (scalar and vector forms)
    import ctypes
    import torch
    W, H, n = shape
    rng = np.random.default_rng(77 + W)
    fields = [rng.uniform(-3, 3, (n, H, W, 2)).astype(F32) for _ in range(4)]
    fields[2][0, H // 2, W // 2] = np.nan
    dtypes = [F32, F32, F16, F32]
    exp, exp_valid = _fold(fields, dtypes)
    assert (exp_valid == 255).any() and (exp_valid == 0).any()
    tacc = torch.from_numpy(fields[0].copy()).to("cuda:0")
    tvalid = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for f, d in zip(fields[1:], dtypes[1:]):
        tf = torch.from_numpy(f.astype(d)).to("cuda:0")
        torch.cuda.synchronize()
        disflow_mod.flow_compose_device(tacc.data_ptr(), F32, tf.data_ptr(), d, n, W, H, tacc.data_ptr(),
                                        valid_a_ptr=tvalid.data_ptr(), valid_out_ptr=tvalid.data_ptr(),
                                        stream=s.cuda_stream)
        s.synchronize()
    _assert_same(tacc.cpu().numpy(), exp, "the accumulator")
    _assert_same(tvalid.cpu().numpy(), exp_valid, "its valid map")
    # and the same chain on host arrays through the C-ABI, out == a
    L = disflow_mod.lib()
    acc = fields[0].copy()
    valid = np.full((n, H, W), 255, np.uint8)
    for f, d in zip(fields[1:], dtypes[1:]):
        b = np.ascontiguousarray(f.astype(d))
        st = L.dis_flow_compose(acc.ctypes.data, 0, b.ctypes.data, 1 if d == F16 else 0, n, W, H, valid.ctypes.data,
                                None, acc.ctypes.data, 0, valid.ctypes.data, 0, None, 0)
        assert st == disflow_mod.DIS_OK, L.dis_last_error()
    assert isinstance(acc.ctypes.data, int) and ctypes.sizeof(ctypes.c_void_p) == 8
    _assert_same(acc, exp, "the host accumulator")
    _assert_same(valid, exp_valid, "its valid map")


W0, H0, MARGIN = 160, 120, 8


def moving_frames(disflow_mod, seed, moves):
    """Frames of W0 x H0 cut out of one value-noise image (disflow.synth_pair's
    first frame): frame k shows the content moved by moves[k] whole pixels."""
    big, _ = disflow_mod.synth_pair(seed, W0 + 2 * MARGIN, H0 + 2 * MARGIN)
    return [np.ascontiguousarray(big[MARGIN - dy:MARGIN - dy + H0, MARGIN - dx:MARGIN - dx + W0]) for dx, dy in moves]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_track_accumulate_equals_the_fold_of_its_flows(disflow_mod, dtype):
    frames = moving_frames(disflow_mod, 11, [(0, 0), (3, 1), (5, -1), (6, 1)])
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Params(3, 1, 8, 25, 0.625, 1), W0, H0, flow_dtype=dtype)
    got = list(eng.track(frames, accumulate=True))
    plain = list(eng.track(frames))
    eng.close()
    assert len(got) == 3 and len(plain) == 3
    acc, valid = None, None
    for k, (flow, gacc, gvalid) in enumerate(got):
        assert flow.dtype == dtype and flow.shape == (H0, W0, 2)
        _assert_same(flow, plain[k], f"pair {k}: the flow is the plain generator's")
        if k == 0:
            acc, valid = flow.astype(F32), np.full((H0, W0), 255, np.uint8)
        else:
            acc, valid = composeref.compose(acc, flow, valid, None, F32)
        _assert_same(gacc, acc, f"pair {k}: accumulated flow")
        _assert_same(gvalid, valid, f"pair {k}: valid map")
    assert (valid == 255).sum() > W0 * H0 // 2


# ---------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------
PW, PH, PN = 67, 33, 3
_points = {}


def points_of(count):
    """PN x count points uniform over [-2, W+1] x [-2, H+1], the first ones of
    each field replaced by NaN, infinite and exact-border points (another start
    in the list for each field, so that a single point per field meets three)."""
    if count not in _points:
        rng = np.random.default_rng(900 + count)
        pts = np.stack([rng.uniform(-2, PW + 1, (PN, count)), rng.uniform(-2, PH + 1, (PN, count))], -1).astype(F32)
        special = [(np.nan, 3.0), (0.0, 0.0), (PW - 1, PH - 1), (3.0, np.nan), (PW - 1, 0.0), (0.0, PH - 1),
                   (np.inf, 2.0), (2.0, -np.inf), (-0.0, 5.5), (PW - 1, 7.25), (np.nextafter(F32(PW - 1), F32(PW)), 4.0),
                   (12.5, np.nextafter(F32(0), F32(-1))), (12.0, 9.0)]
        for k in range(PN):
            for j in range(min(count, len(special))):
                pts[k, j] = special[(j + 4 * k) % len(special)]
        pts.setflags(write=False)
        _points[count] = pts
    return _points[count]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("count", [1, 63, 1000])
def test_advect_points_matches_restatement(disflow_mod, count, dtype):
    import torch
    flow = inputs(PW, PH, PN)[1][np.dtype(dtype)]
    pts = points_of(count)
    exp, exp_status = composeref.advect(pts, flow)
    if count >= 63:
        assert (exp_status == 255).any() and (exp_status == 0).any()
    # host arrays
    got, got_status = disflow_mod.advect_points(pts, flow, with_status=True)
    _assert_same(got, exp, "points_out")
    _assert_same(got_status, exp_status, "status")
    _assert_same(disflow_mod.advect_points(pts, flow), exp, "points_out without status")
    one, one_status = disflow_mod.advect_points(pts[1], flow[1], with_status=True)
    _assert_same(one, exp[1], "one field's points")
    _assert_same(one_status, exp_status[1], "one field's status")
    # host arrays in place, through the C-ABI
    L = disflow_mod.lib()
    fl = np.ascontiguousarray(flow)
    buf = pts.copy()
    st = L.dis_flow_advect_points(fl.ctypes.data, 1 if dtype == F16 else 0, PN, PW, PH, buf.ctypes.data, count,
                                  buf.ctypes.data, None, 0, None, 0)
    assert st == disflow_mod.DIS_OK, L.dis_last_error()
    _assert_same(buf, exp, "points_out == points on the host")
    # device pointers on a caller's stream, out of place and in place
    s = torch.cuda.Stream()
    tflow = torch.from_numpy(fl.copy()).to("cuda:0")
    tpts = torch.from_numpy(pts.copy()).to("cuda:0")
    tout = torch.full((PN, count, 2), 9.0, dtype=torch.float32, device="cuda:0")
    tstatus = torch.full((PN, count), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    disflow_mod.advect_points_device(tflow.data_ptr(), dtype, PN, PW, PH, tpts.data_ptr(), count, tout.data_ptr(),
                                     status_ptr=tstatus.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    _assert_same(tout.cpu().numpy(), exp, "device points_out")
    _assert_same(tstatus.cpu().numpy(), exp_status, "device status")
    _assert_same(tpts.cpu().numpy(), pts, "the points after the call")
    tstatus.fill_(9)
    torch.cuda.synchronize()
    disflow_mod.advect_points_device(tflow.data_ptr(), dtype, PN, PW, PH, tpts.data_ptr(), count, tpts.data_ptr(),
                                     stream=s.cuda_stream)
    s.synchronize()
    _assert_same(tpts.cpu().numpy(), exp, "device points_out == points")
    assert bool((tstatus == 9).all()), "status written though not asked for"


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_accumulated_flow_end_to_end(disflow_mod):
    # Value noise (synth_pair 11's first frame at 176 x 136) seen through a
    # 160 x 120 window: the content moves by (3, 1), then by (2, -2). MEDIUM's
    # knobs with coarsest scale 3. With the CPU oracle's flows (the engine's, bit
    # for bit) and the restatement: the composed field is valid on 18441 of
    # 19200 pixels (0.9605), its mean endpoint error against (5, -1) is 0.319 px
    # (the direct 0 -> 2 flow: 0.191 px), and warping frame 2 back by it brings
    # the mean |I - frame 0| over the valid pixels from 38.355 down to 3.243.
    f0, f1, f2 = moving_frames(disflow_mod, 11, [(0, 0), (3, 1), (5, -1)])
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Params(3, 1, 8, 25, 0.625, 1), W0, H0)
    fl1, fl2 = eng.calc(f0, f1), eng.calc(f1, f2)
    eng.close()
    acc, valid = disflow_mod.flow_compose(fl1, fl2, with_valid=True)
    exp, exp_valid = composeref.compose(fl1, fl2)
    _assert_same(acc, exp, "accumulated flow")
    _assert_same(valid, exp_valid, "valid map")
    m = valid == 255
    print(f"valid {m.mean():.4f} ({int(m.sum())} pixels)")
    assert m.sum() > W0 * H0 // 2
    warped = disflow_mod.flow_warp(f2, acc)  # (NaN vectors give 0; they are not among the valid pixels)
    _assert_same(warped, warpref.warp(f2, acc)[0], "frame 2 warped back")
    warped_err = np.abs(warped[m].astype(np.int32) - f0[m]).mean()
    plain_err = np.abs(f2[m].astype(np.int32) - f0[m]).mean()
    epe = np.sqrt(((acc[m] - F32([5, -1])) ** 2).sum(-1)).mean()
    print(f"mean |warp(frame 2, acc) - frame 0| {warped_err:.3f}, mean |frame 2 - frame 0| {plain_err:.3f}, "
          f"mean endpoint error {epe:.3f}")
    assert warped_err < plain_err, (warped_err, plain_err)


# ---------------------------------------------------------------------------
# the facade and the CLI
# ---------------------------------------------------------------------------
def test_cpp_facade_compose(tmp_path):
    # tests/cpp/test_compose.cpp: dis::flowCompose in its f32 form (plain, with
    # the planes, in place) and its half_bits form, and dis::advectPoints, on
    # the first two fields of the (67, 33, 3) case
    shape, n = (67, 33, 3), 2
    a, b, va, mb = inputs(*shape)
    a32, b32, b16 = a[np.dtype(F32)][:n], b[np.dtype(F32)][:n], b[np.dtype(F16)][:n]
    for name, arr in (("a.f32", a32), ("b.f32", b32), ("b.f16", b16), ("valid_a.u8", va[:n]), ("mask_b.u8", mb[:n])):
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
    expected(shape, (F32, F32, F32), False, False)[0][:n].tofile(str(tmp_path / "out_plain.f32"))
    gated = expected(shape, (F32, F32, F32), True, True)
    gated[0][:n].tofile(str(tmp_path / "out_gated.f32"))
    gated[1][:n].tofile(str(tmp_path / "valid_gated.u8"))
    half = expected(shape, (F32, F16, F32), False, False)
    half[0][:n].tofile(str(tmp_path / "out_half.f32"))
    half[1][:n].tofile(str(tmp_path / "valid_half.u8"))
    pts = points_of(63)[:n]
    moved, status = composeref.advect(pts, b32)
    np.ascontiguousarray(pts).tofile(str(tmp_path / "points.f32"))
    moved.tofile(str(tmp_path / "moved.f32"))
    status.tofile(str(tmp_path / "status.u8"))
    exe = str(tmp_path / "test_compose")
    lib_dir = os.path.join(PKG, "disflow")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_compose.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout


@pytest.mark.parametrize("extra", [[], ["--batch", "1"], ["--warm-start"], ["--bidir"]],
                         ids=["plain", "batch1", "warm-start", "bidir"])
def test_cli_accumulate_writes_the_composed_flow(disflow_mod, tmp_path, extra):
    import pngio
    cli = os.path.join(PKG, "disflow", "dis_flow")
    frames = moving_frames(disflow_mod, 11, [(0, 0), (3, 1), (5, -1)])
    d = tmp_path / "seq"
    d.mkdir()
    for k, f in enumerate(frames):
        pngio.write_gray8(str(d / f"frame_{k + 1:04d}.png"), f)
    args = [cli, "seq", "1", "3", "10", "8", "3", "1", "0.5", "1", "0", "--flo", "--accumulate"] + extra
    r = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    base = [str(tmp_path / f"OF_seq/frame_{k + 1:04d}") for k in range(2)]
    fl = [disflow_mod.read_flo(p + ".flo") for p in base]
    acc = [disflow_mod.read_flo(p + "_acc.flo") for p in base]
    _assert_same(acc[0], fl[0], "pair 0: the accumulated flow is the pair's")
    mask = None
    if "--bidir" in extra:
        mask = disflow_mod.flow_consistency(fl[1], disflow_mod.read_flo(base[1] + "_bw.flo"))
        assert (mask == 0).any() and (mask == 255).any()
    exp, exp_valid = disflow_mod.flow_compose(fl[0], fl[1], mask_b=mask, with_valid=True)
    _assert_same(acc[1], exp, "pair 1: the accumulated flow")
    _assert_same(exp, composeref.compose(fl[0], fl[1], None, mask)[0], "and the restatement's")
    assert (exp_valid == 255).sum() > W0 * H0 // 2 and np.isnan(acc[1][exp_valid == 0]).all()
    assert f"accumulate seq/frame_0002.png: {int((exp_valid == 255).sum())} of {W0 * H0} pixels" in r.stdout
