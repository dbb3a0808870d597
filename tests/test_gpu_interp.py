"""GPU tests of the frame interpolation (dis_flow_interp_u8): both kernels
against their numpy restatement (tests/interpref.py) on host arrays and on
device pointers in every layout that selects another load / store form, with a
workspace left dirty by the call before, DenseInverseSearch.interpolate, the
C++ facade and the CLI's --interp. Every comparison is bit for bit, of the
frame and of the fill map. Each input is first checked on the restatement to
reach the hard paths (contested targets, ties, every fill class, vectors that
leave the frame or are invalid), so that no test passes by avoiding them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import interpref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")

N = 3
TIMES = [0.0, 0.25, 1.0 / 3.0, 0.5, 1.0]
FLOW_DTYPES = [np.float32, np.float16]
CHANNELS = [1, 3, 4]
# scene: the two-layer scene, 64 x 48 (every vector form); ties: equal costs
# everywhere, 64 x 48; far: vectors up to +-40 px with invalid ones, 37 x 23
# (odd: every scalar form, a short last lane); row: 8 x 1 (one row, two lanes)
CASES = ["scene", "ties", "far", "row"]
SIZES = {"scene": (64, 48), "ties": (64, 48), "far": (37, 23), "row": (8, 1)}
_inputs = {}
_expected = {}


def _assert_same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    bad = g != e
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first at {idx[0].tolist()} "
                             f"got {g[tuple(idx[0])]!r} exp {e[tuple(idx[0])]!r}")


def _channels(gray, C):
    """(n, H, W) bytes -> (n, H, W, C): the further channels are fixed byte maps of the first."""
    maps = [gray, 255 - gray, (gray // 2) + 40, gray ^ 0x55]
    return np.ascontiguousarray(np.stack(maps[:C], axis=-1).astype(np.uint8))


def inputs(case, C):
    """(I0, I1, {dtype: (fw, bw)}) of N pairs: made once, never changed."""
    key = (case, C)
    if key in _inputs:
        return _inputs[key]
    W, H = SIZES[case]
    rng = np.random.default_rng(1000 * CASES.index(case) + 7)
    if case == "scene":
        a, b, fw1, bw1 = interpref.two_layer_scene()
        g0, g1 = np.stack([a] * N), np.stack([b] * N)
        fw = (fw1[None] + rng.normal(0, 0.3, (N, H, W, 2))).astype(np.float32)
        bw = (bw1[None] + rng.normal(0, 0.3, (N, H, W, 2))).astype(np.float32)
    elif case == "ties":
        # period-4 columns: I1(x + 4r, y) = I0(x, y) for every integer r, so every cost is exactly 0
        col = rng.integers(0, 256, (N, H, 4), dtype=np.uint8)
        g0 = np.ascontiguousarray(np.tile(col, (1, 1, W // 4)))
        g1 = g0.copy()
        fw = np.zeros((N, H, W, 2), np.float32)
        bw = np.zeros((N, H, W, 2), np.float32)
        fw[..., 0] = 4 * rng.integers(-2, 3, (N, H, W))
        bw[..., 0] = 4 * rng.integers(-2, 3, (N, H, W))
    else:
        g0 = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
        g1 = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
        amp = 40.0 if case == "far" else 3.0
        fw = rng.uniform(-amp, amp, (N, H, W, 2)).astype(np.float32)
        bw = rng.uniform(-amp, amp, (N, H, W, 2)).astype(np.float32)
        if case == "far":  # near vectors too, so that the frame is not all holes
            near = rng.random((N, H, W)) < 0.5
            fw[near] = rng.uniform(-3, 3, (int(near.sum()), 2)).astype(np.float32)
            bad = [(np.nan, np.nan), (1e9, -1e9), (-1e9, 2.0), (np.inf, 0.5), (1.0, -np.inf), (0.0, np.nan), (2e9, 0.0)]
            for f in (fw, bw):
                flat = f.reshape(-1, 2)
                pos = rng.choice(flat.shape[0], size=5 * len(bad), replace=False)
                for j, q in enumerate(pos):
                    flat[q] = bad[j % len(bad)]
    I0, I1 = _channels(g0, C), _channels(g1, C)
    with np.errstate(over="ignore"):
        flows = {np.float32: (fw, bw), np.float16: (fw.astype(np.float16), bw.astype(np.float16))}
    for a in (I0, I1) + flows[np.float32] + flows[np.float16]:
        a.setflags(write=False)
    _inputs[key] = (I0, I1, flows)
    return _inputs[key]


def expected(case, C, dtype, t, with_bw):
    """The restatement's (dst, fill, count) of one case: computed once, never changed."""
    key = (case, C, dtype, t, with_bw)
    if key not in _expected:
        I0, I1, flows = inputs(case, C)
        fw, bw = flows[dtype]
        out = interpref.interp(I0, I1, fw, t, bw if with_bw else None)
        for a in out:
            a.setflags(write=False)
        _expected[key] = out
    return _expected[key]


@pytest.mark.parametrize("dtype", FLOW_DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("C", CHANNELS)
def test_inputs_reach_the_hard_paths(C, dtype):
    # conditions on the restatement alone (they hold on any machine)
    for t in (0.25, 1.0 / 3.0, 0.5):
        dst, fill, count = expected("scene", C, dtype, t, True)
        for k in range(N):
            assert (count[k] > 1).sum() >= 100, (t, k, int((count[k] > 1).sum()))
            for cls in (0, 1, 2):
                assert (fill[k] == cls).sum() >= 10, (t, k, cls, int((fill[k] == cls).sum()))
        assert not np.array_equal(dst, expected("scene", C, dtype, t, False)[0])
    I0, I1, flows = inputs("ties", C)
    for t in (0.25, 0.5):
        for k in range(N):
            fw = flows[dtype][0][k]
            d, f, c, pairs = interpref.interp(I0[k], I1[k], fw, t, details=True)
            assert interpref.contested_with_different_vectors(fw, pairs) >= 100
    # far: many vectors leave the frame or are invalid, and the rest collide
    dst, fill, count = expected("far", C, dtype, 0.5, True)
    fw = flows_of("far", C, dtype)[0].astype(np.float32)
    with np.errstate(invalid="ignore"):
        assert (~(np.abs(fw) < 1e9).all(axis=-1)).sum() >= 20
    assert (count == 0).sum() >= 100 and (count > 1).sum() >= 100
    assert all((fill == cls).sum() >= 10 for cls in (0, 1, 2))


def flows_of(case, C, dtype):
    return inputs(case, C)[2][dtype]


@pytest.mark.parametrize("dtype", FLOW_DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("case", CASES)
def test_interp_matches_restatement_host(disflow_mod, case, C, dtype):
    I0, I1, flows = inputs(case, C)
    fw, bw = flows[dtype]
    for t in TIMES:
        for with_bw in (True, False):
            what = f"t {t}, {'bw' if with_bw else 'no bw'}"
            dst, fill, _ = expected(case, C, dtype, t, with_bw)
            got, got_fill = disflow_mod.flow_interp(I0, I1, fw, t, bw=bw if with_bw else None, return_fill=True)
            _assert_same(got, dst, "dst, " + what)
            _assert_same(got_fill, fill, "fill, " + what)
    # the endpoints, as the header promises
    _assert_same(disflow_mod.flow_interp(I0, I1, fw, 1.0, bw=bw), I1, "t = 1")
    _assert_same(disflow_mod.flow_interp(I0, I1, fw, 0.0), I0, "t = 0 without bw")
    # the other layouts of the wrapper: without the fill map, one pair of the stack, one channel without its axis
    dst, fill, _ = expected(case, C, dtype, 0.25, True)
    _assert_same(disflow_mod.flow_interp(I0, I1, fw, 0.25, bw=bw), dst, "dst without fill")
    one, one_fill = disflow_mod.flow_interp(I0[1], I1[1], fw[1], 0.25, bw=bw[1], return_fill=True)
    _assert_same(one, dst[1], "one (H, W, C) pair")
    _assert_same(one_fill, fill[1], "one pair's fill")
    if C == 1:
        _assert_same(disflow_mod.flow_interp(I0[..., 0], I1[..., 0], fw, 0.25, bw=bw), dst[..., 0], "(n, H, W) images")
        _assert_same(disflow_mod.flow_interp(I0[0, ..., 0], I1[0, ..., 0], fw[0], 0.25, bw=bw[0]), dst[0, ..., 0],
                     "one (H, W) pair")


def _offset_tensor(torch, host, lead, fill=7):
    """`host` (a flat numpy array) on the device, `lead` elements into a fresh
    allocation (allocations are at least 256-byte aligned)."""
    t = torch.full((lead + host.size,), fill, dtype=torch.from_numpy(host[:1].copy()).dtype, device="cuda:0")[lead:]
    t.copy_(torch.from_numpy(host.copy()))
    return t


def _padded(img, stride, image_stride, seed):
    n, H = img.shape[:2]
    row = img[0, 0].size
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, n * image_stride, dtype=np.uint8)  # the padding holds other bytes
    for k in range(n):
        rows = host[k * image_stride:k * image_stride + H * stride].reshape(H, stride)
        rows[:, :row] = img[k].reshape(H, row)
    return host


@pytest.mark.parametrize("layout", ["aligned", "offset", "padded"])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("case", CASES)
def test_interp_matches_restatement_device(disflow_mod, case, C, layout):
    # device pointers (torch tensors) on a caller's stream. aligned: every vector
    # form the shape allows; offset: flows one (u,v) pair in, the workspace one
    # key in, images, dst and fill 1 byte in, so no vector form applies; padded:
    # rows and images of both frames further apart than they are long. One
    # workspace serves every call of the test and starts as zeros: a call that
    # did not reset it would find every target taken by key 0.
    import torch
    W, H = SIZES[case]
    I0, I1, flows = inputs(case, C)
    lead = 1 if layout == "offset" else 0
    stride, image_stride = 0, 0
    h0, h1 = I0.reshape(-1), I1.reshape(-1)
    if layout == "padded":
        stride = W * C + 5
        image_stride = stride * H + 7
        h0, h1 = _padded(I0, stride, image_stride, 5), _padded(I1, stride, image_stride, 6)
    t0, t1 = _offset_tensor(torch, h0, lead), _offset_tensor(torch, h1, lead)
    px = N * H * W
    assert disflow_mod.flow_interp_workspace(N, W, H) == 8 * px
    tws = torch.zeros(lead + px, dtype=torch.int64, device="cuda:0")[lead:]
    assert tws.data_ptr() % 16 == 8 * lead and t0.data_ptr() % 16 == lead
    s = torch.cuda.Stream()
    for dtype in FLOW_DTYPES:
        fw, bw = flows[dtype]
        tfw = _offset_tensor(torch, fw.reshape(-1), 2 * lead, fill=0)
        tbw = _offset_tensor(torch, bw.reshape(-1), 2 * lead, fill=0)
        assert tfw.data_ptr() % 16 == lead * 2 * fw.itemsize
        for t, with_bw, with_fill in ((0.25, True, True), (0.5, False, True), (1.0 / 3.0, True, False),
                                      (0.0, True, True), (1.0, False, True)):
            tdst = torch.full((lead + px * C,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
            tfill = torch.full((lead + px,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
            torch.cuda.synchronize()
            disflow_mod.flow_interp_device(t0.data_ptr(), t1.data_ptr(), tfw.data_ptr(), dtype, N, W, H, C, t,
                                           tdst.data_ptr(), tws.data_ptr(), bw_ptr=tbw.data_ptr() if with_bw else 0,
                                           fill_ptr=tfill.data_ptr() if with_fill else 0, stride=stride,
                                           image_stride=image_stride, stream=s.cuda_stream)
            s.synchronize()
            dst, fill, _ = expected(case, C, dtype, t, with_bw)
            what = f"{np.dtype(dtype).name} flows, t {t}, {'bw' if with_bw else 'no bw'}"
            _assert_same(tdst.cpu().numpy().reshape(N, H, W, C), dst, "dst, " + what)
            if with_fill:
                _assert_same(tfill.cpu().numpy().reshape(N, H, W), fill, "fill, " + what)
            else:
                assert bool((tfill == 9).all()), "fill written though not asked for"


def test_dirty_workspace_and_host_path_against_device_path(disflow_mod):
    # two different calls into one workspace: the second finds the first one's
    # keys (and, before the first, a workspace of zeros) and must not see them
    import torch
    C = 1
    W, H = SIZES["scene"]
    px = N * H * W
    tws = torch.zeros(px, dtype=torch.int64, device="cuda:0")
    tdst = torch.empty(px * C, dtype=torch.uint8, device="cuda:0")
    tfill = torch.empty(px, dtype=torch.uint8, device="cuda:0")
    for case, t in (("ties", 0.5), ("scene", 0.25), ("ties", 0.25)):
        I0, I1, flows = inputs(case, C)
        fw, bw = flows[np.float32]
        dev = [torch.from_numpy(a.copy()).to("cuda:0") for a in (I0, I1, fw, bw)]
        disflow_mod.flow_interp_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), np.float32, N, W, H, C,
                                       t, tdst.data_ptr(), tws.data_ptr(), bw_ptr=dev[3].data_ptr(),
                                       fill_ptr=tfill.data_ptr())
        torch.cuda.synchronize()
        host, host_fill = disflow_mod.flow_interp(I0, I1, fw, t, bw=bw, return_fill=True)
        _assert_same(tdst.cpu().numpy().reshape(I0.shape), host, f"{case}: device against host path")
        _assert_same(tfill.cpu().numpy().reshape(N, H, W), host_fill, f"{case}: fill, device against host path")
        _assert_same(host, expected(case, C, np.float32, t, True)[0], f"{case}: against the restatement")
        keys = tws.cpu().numpy().view(np.uint64)
        assert ((keys == interpref.NOKEY) == (expected(case, C, np.float32, t, True)[2].reshape(-1) == 0)).all()


def test_interp_rejects_bad_device_pointers(disflow_mod):
    import torch
    f = torch.zeros(256, dtype=torch.float32, device="cuda:0")
    b = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    w = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    ok = dict(I0_ptr=b.data_ptr(), I1_ptr=b.data_ptr() + 16, fw_ptr=f.data_ptr(), flow_dtype=np.float32, n=1, width=2,
              height=2, channels=1, t=0.5, dst_ptr=b.data_ptr() + 32, workspace_ptr=w.data_ptr())
    disflow_mod.flow_interp_device(**ok)
    torch.cuda.synchronize()
    for over in (dict(workspace_ptr=0), dict(workspace_ptr=w.data_ptr() + 4), dict(fw_ptr=f.data_ptr() + 4),
                 dict(bw_ptr=f.data_ptr() + 68), dict(flow_dtype=np.float16, fw_ptr=f.data_ptr() + 2),
                 dict(dst_ptr=b.data_ptr() + 15), dict(fill_ptr=b.data_ptr() + 33),
                 dict(workspace_ptr=f.data_ptr())):
        with pytest.raises(disflow_mod.DisError) as e:
            disflow_mod.flow_interp_device(**dict(ok, **over))
        assert e.value.status == disflow_mod.DIS_ERR_INVALID_ARGUMENT, over


@pytest.mark.parametrize("dtype", FLOW_DTYPES, ids=["f32", "f16"])
def test_engine_interpolate(disflow_mod, dtype):
    # one calc_bidir, then one interpolation per time with the engine's flows as they are
    W, H = 160, 120
    I0, I1 = disflow_mod.synth_pair(7, W, H)
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Preset.MEDIUM, W, H, flow_dtype=dtype)
    fw, bw = eng.calc_bidir(I0, I1)
    ts = [0.25, 0.5, 0.75]
    frames = eng.interpolate(I0, I1, ts)
    pairs = eng.interpolate(I0, I1, ts[:1], return_fill=True)
    eng.close()
    assert fw.dtype == np.dtype(dtype) and len(frames) == 3
    for t, frame in zip(ts, frames):
        dst, fill, _ = interpref.interp(I0, I1, fw, t, bw)
        _assert_same(frame, dst, f"t {t}")
    _assert_same(pairs[0][0], frames[0], "return_fill: frame")
    _assert_same(pairs[0][1], interpref.interp(I0, I1, fw, ts[0], bw)[1], "return_fill: fill")
    # and the frames are closer to both neighbours than these are to each other
    mid = frames[1].astype(np.int32)
    assert np.abs(mid - I0).mean() < np.abs(I1.astype(np.int32) - I0).mean()
    assert np.abs(mid - I1).mean() < np.abs(I1.astype(np.int32) - I0).mean()


def test_cpp_facade_interp(tmp_path):
    # tests/cpp/test_interp.cpp: dis::flowInterp in its f32 form (bw, fill) and
    # its f16 form (no bw, no fill) on the far case with 3 channels at t = 0.25
    I0, I1, flows = inputs("far", 3)
    I0.tofile(str(tmp_path / "I0.u8"))
    I1.tofile(str(tmp_path / "I1.u8"))
    flows[np.float32][0].tofile(str(tmp_path / "fw.f32"))
    flows[np.float32][1].tofile(str(tmp_path / "bw.f32"))
    flows[np.float16][0].tofile(str(tmp_path / "fw.f16"))
    dst, fill, _ = expected("far", 3, np.float32, 0.25, True)
    dst.tofile(str(tmp_path / "dst_f32_bw.u8"))
    fill.tofile(str(tmp_path / "fill_f32_bw.u8"))
    expected("far", 3, np.float16, 0.25, False)[0].tofile(str(tmp_path / "dst_f16.u8"))
    exe = str(tmp_path / "test_interp")
    lib_dir = os.path.join(PKG, "disflow")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_interp.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout


@pytest.mark.parametrize("extra", [[], ["--bidir"]], ids=["plain", "bidir"])
def test_cli_interp_writes_the_frames_between(disflow_mod, tmp_path, extra):
    import pngio
    cli = os.path.join(PKG, "disflow", "dis_flow")
    png_tool = os.path.join(ROOT, "tests", "cpp", "png_tool")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "png_tool"])
    subprocess.check_call(["make", "-s", "-C", PKG])
    W, H = 160, 96
    a, b = disflow_mod.synth_pair(50, W, H)
    c, _ = disflow_mod.synth_pair(51, W, H)
    frames = [a, b, c]
    d = tmp_path / "seq"
    d.mkdir()
    for k, f in enumerate(frames):
        pngio.write_gray8(str(d / f"frame_{k + 1:04d}.png"), f)
    args = [cli, "seq", "1", "3", "10", "8", "3", "1", "0.5", "1", "0", "--flo", "--interp", "2"] + extra
    r = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in range(2):
        base = str(tmp_path / f"OF_seq/frame_{k + 1:04d}")
        fw = disflow_mod.read_flo(base + ".flo")
        bw = disflow_mod.read_flo(base + "_bw.flo") if extra else None
        for j in (1, 2):
            raw_path = str(tmp_path / "interp.raw")
            subprocess.run([png_tool, "gray", f"{base}_interp_{j}.png", raw_path], check=True)
            raw = open(raw_path, "rb").read()
            assert struct.unpack("<ii", raw[:8]) == (W, H)
            got = np.frombuffer(raw[8:], np.uint8).reshape(H, W)
            exp = disflow_mod.flow_interp(frames[k], frames[k + 1], fw, np.float32(j) / np.float32(3), bw=bw)
            _assert_same(got, exp, f"pair {k}: interp PNG {j}")
        assert not os.path.exists(f"{base}_interp_3.png")
