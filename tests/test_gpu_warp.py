"""GPU tests of the flow warp (dis_flow_warp_u8): the kernel against its numpy
restatement (tests/warpref.py) on host arrays and on device pointers in every
layout that selects another load / store form, an f16 engine's output straight
in, the end-to-end photometric gain, the C++ facade and the CLI's --warp.
Every comparison is bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import warpref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")


def _assert_same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    bad = g != e
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first at {idx[0].tolist()} "
                             f"got {g[tuple(idx[0])]!r} exp {e[tuple(idx[0])]!r}")


# (W, H, n, C): a single pixel; a short last lane and an odd W (no vector form);
# dword stores; many short rows; dword taps and 16-byte stores; the same with
# an odd W; many rows
SHAPES = [(1, 1, 1, 1), (5, 3, 2, 1), (16, 4, 1, 3), (67, 33, 3, 3), (64, 8, 2, 4), (67, 33, 2, 4), (160, 120, 2, 1)]
FLOW_DTYPES = [np.float32, np.float16]
BORDERS = [("replicate", warpref.REPLICATE), ("zero", warpref.ZERO)]
SCALES = [1.0, 0.5, -1.0]
_inputs = {}
_expected = {}


def inputs(W, H, n, C):
    """Images of random bytes and flows uniform in +-6 px (border pixels leave
    the frame on their own) with a handful of NaN, +-1e9 and +-inf vectors, as
    float32 and narrowed to float16: made once, never changed."""
    key = (W, H, n, C)
    if key not in _inputs:
        rng = np.random.default_rng(100000 * C + 1000 * W + 10 * H + n)
        img = rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)
        flow = rng.uniform(-6, 6, (n, H, W, 2)).astype(np.float32)
        bad = [(np.nan, np.nan), (1e9, -1e9), (-1e9, 2.0), (np.inf, 0.5), (1.0, -np.inf), (0.0, np.nan), (2e9, 0.0)]
        flat = flow.reshape(-1, 2)
        pos = rng.choice(flat.shape[0], size=min(len(bad), flat.shape[0] // 8), replace=False)
        for j, q in enumerate(pos):
            flat[q] = bad[j]
        with np.errstate(over="ignore"):
            flow16 = flow.astype(np.float16)  # (+-1e9 become +-inf: still invalid)
        for a in (img, flow, flow16):
            a.setflags(write=False)
        _inputs[key] = (img, {np.float32: flow, np.float16: flow16})
    return _inputs[key]


def expected(shape, dtype, border, scale):
    """The restatement's (dst, valid) of one case: computed once, never changed."""
    key = (shape, dtype, border, scale)
    if key not in _expected:
        img, flows = inputs(*shape)
        dst, valid = warpref.warp(img, flows[dtype], scale, border)
        dst.setflags(write=False)
        valid.setflags(write=False)
        _expected[key] = (dst, valid)
    return _expected[key]


@pytest.mark.parametrize("dtype", FLOW_DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_matches_restatement_host(disflow_mod, shape, dtype):
    img, flows = inputs(*shape)
    for bname, border in BORDERS:
        for scale in SCALES:
            what = f"{bname}, scale {scale}"
            dst, valid = expected(shape, dtype, border, scale)
            got, got_valid = disflow_mod.flow_warp(img, flows[dtype], scale=scale, border=bname, with_valid=True)
            _assert_same(got, dst, "dst, " + what)
            _assert_same(got_valid, valid, "valid, " + what)
            _assert_same(disflow_mod.flow_warp(img, flows[dtype], scale=scale, border=bname), dst,
                         "dst without valid, " + what)
    W, H, n, C = shape
    if W * H * n >= 1000:  # a kernel that ignores a mode cannot pass
        rep, valid = expected(shape, dtype, warpref.REPLICATE, 1.0)
        zero, _ = expected(shape, dtype, warpref.ZERO, 1.0)
        assert (valid == 255).any() and (valid == 0).any()
        assert not np.array_equal(rep, zero)
        assert not np.array_equal(expected(shape, np.float32, warpref.REPLICATE, 1.0)[0],
                                  expected(shape, np.float16, warpref.REPLICATE, 1.0)[0])
        assert not np.array_equal(rep, expected(shape, dtype, warpref.REPLICATE, 0.5)[0])
    # the other image layouts of the wrapper: one image of a stack, and (n, H, W) / (H, W) for one channel
    one, one_valid = disflow_mod.flow_warp(img[0], flows[dtype][0], with_valid=True)
    dst, valid = expected(shape, dtype, warpref.REPLICATE, 1.0)
    _assert_same(one, dst[0], "one (H, W, C) image")
    _assert_same(one_valid, valid[0], "one image's valid")
    if C == 1:
        _assert_same(disflow_mod.flow_warp(img[..., 0], flows[dtype]), dst[..., 0], "(n, H, W) images")
        _assert_same(disflow_mod.flow_warp(img[0, ..., 0], flows[dtype][0]), dst[0, ..., 0], "one (H, W) image")


def _offset_tensor(torch, host, lead, fill=7):
    """`host` (a flat numpy array) on the device, `lead` elements into a fresh
    allocation (allocations are at least 256-byte aligned)."""
    t = torch.full((lead + host.size,), fill, dtype=torch.from_numpy(host[:1].copy()).dtype, device="cuda:0")[lead:]
    t.copy_(torch.from_numpy(host.copy()))
    return t


@pytest.mark.parametrize("layout", ["aligned", "offset", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_matches_restatement_device(disflow_mod, shape, layout):
    # device pointers (torch tensors) on a caller's stream. aligned: every vector
    # form the shape allows; offset: flow one (u,v) pair in, image, dst and valid
    # 1 byte in, so no vector form applies; padded: rows and images of the
    # source further apart than they are long
    import torch
    W, H, n, C = shape
    img, flows = inputs(*shape)
    lead = 1 if layout == "offset" else 0
    stride, image_stride = W * C, W * C * H
    src_host = img.reshape(-1)
    if layout == "padded":
        stride = W * C + 5
        image_stride = stride * H + 7
        rng = np.random.default_rng(5)
        src_host = rng.integers(0, 256, n * image_stride, dtype=np.uint8)  # the padding holds other bytes
        for k in range(n):
            rows = src_host[k * image_stride:k * image_stride + H * stride].reshape(H, stride)
            rows[:, :W * C] = img[k].reshape(H, W * C)
    tsrc = _offset_tensor(torch, src_host, lead)
    px = n * H * W
    s = torch.cuda.Stream()
    for dtype in FLOW_DTYPES:
        tflow = _offset_tensor(torch, flows[dtype].reshape(-1), 2 * lead, fill=0)
        pair = 2 * flows[dtype].itemsize
        assert tsrc.data_ptr() % 16 == lead and tflow.data_ptr() % 16 == lead * pair
        for bname, border in BORDERS:
            for scale, with_valid in ((1.0, True), (0.5, False)):
                tdst = torch.full((lead + px * C,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
                tvalid = torch.full((lead + px,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
                torch.cuda.synchronize()
                disflow_mod.flow_warp_device(tsrc.data_ptr(), tflow.data_ptr(), dtype, n, W, H, C, tdst.data_ptr(),
                                             tvalid.data_ptr() if with_valid else 0, scale=scale, border=bname,
                                             src_stride=0 if layout != "padded" else stride,
                                             src_image_stride=0 if layout != "padded" else image_stride,
                                             stream=s.cuda_stream)
                s.synchronize()
                dst, valid = expected(shape, dtype, border, scale)
                what = f"{np.dtype(dtype).name} flow, {bname}, scale {scale}"
                _assert_same(tdst.cpu().numpy().reshape(n, H, W, C), dst, "dst, " + what)
                if with_valid:
                    _assert_same(tvalid.cpu().numpy().reshape(n, H, W), valid, "valid, " + what)
                else:
                    assert bool((tvalid == 9).all()), "valid written though not asked for"


def test_warp_rejects_misaligned_device_flow(disflow_mod):
    import torch
    f = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    b = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    for dtype, off in ((np.float32, 4), (np.float16, 2)):
        with pytest.raises(disflow_mod.DisError) as e:
            disflow_mod.flow_warp_device(b.data_ptr(), f.data_ptr() + off, dtype, 1, 2, 2, 1, b.data_ptr() + 32)
        assert e.value.status == disflow_mod.DIS_ERR_INVALID_ARGUMENT


def test_f16_engine_output_goes_straight_in(disflow_mod):
    W, H = 160, 120
    I0, I1 = disflow_mod.synth_pair(7, W, H)
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Preset.MEDIUM, W, H, flow_dtype=np.float16)
    flow = eng.calc(I0, I1)
    eng.close()
    assert flow.dtype == np.float16 and flow.shape == (H, W, 2)
    got, got_valid = disflow_mod.flow_warp(I1, flow, with_valid=True)
    dst, valid = warpref.warp(I1, flow.astype(np.float32))
    _assert_same(got, dst, "dst")
    _assert_same(got_valid, valid, "valid")


def test_warp_end_to_end_reduces_photometric_error(disflow_mod):
    # synth pair 7 at 160 x 120, MEDIUM: with the oracle's flow (the engine's,
    # bit for bit) and the restatement, the mean |warped I1 - I0| over the 18382
    # valid pixels is 3.526 against a mean |I1 - I0| of 29.281 over the same pixels
    W, H = 160, 120
    I0, I1 = disflow_mod.synth_pair(7, W, H)
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Preset.MEDIUM, W, H)
    flow = eng.calc(I0, I1)
    eng.close()
    got, got_valid = disflow_mod.flow_warp(I1, flow, with_valid=True)
    dst, valid = warpref.warp(I1, flow)
    _assert_same(got, dst, "dst")
    _assert_same(got_valid, valid, "valid")
    m = got_valid == 255
    assert m.sum() > W * H // 2
    warped_err = np.abs(got[m].astype(np.int32) - I0[m]).mean()
    plain_err = np.abs(I1[m].astype(np.int32) - I0[m]).mean()
    assert warped_err < plain_err, (warped_err, plain_err)


def test_cpp_facade_warp(tmp_path):
    # tests/cpp/test_warp.cpp: dis::flowWarp in its f32 form (the defaults, with
    # valid) and its f16 form (scale 0.5, Border::ZERO) on the (67, 33, 2, 3) case
    shape = (67, 33, 2, 3)
    img, flows = inputs(*shape)
    img.tofile(str(tmp_path / "src.u8"))
    flows[np.float32].tofile(str(tmp_path / "flow.f32"))
    flows[np.float16].tofile(str(tmp_path / "flow.f16"))
    dst, valid = expected(shape, np.float32, warpref.REPLICATE, 1.0)
    dst.tofile(str(tmp_path / "dst_f32.u8"))
    valid.tofile(str(tmp_path / "valid_f32.u8"))
    expected(shape, np.float16, warpref.ZERO, 0.5)[0].tofile(str(tmp_path / "dst_f16.u8"))
    exe = str(tmp_path / "test_warp")
    lib_dir = os.path.join(PKG, "disflow")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_warp.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout


@pytest.mark.parametrize("extra", [[], ["--batch", "1"], ["--bidir"], ["--warm-start"]],
                         ids=["plain", "batch1", "bidir", "warm-start"])
def test_cli_warp_writes_the_warped_second_frame(disflow_mod, tmp_path, extra):
    import pngio
    cli = os.path.join(PKG, "disflow", "dis_flow")
    png_tool = os.path.join(ROOT, "tests", "cpp", "png_tool")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "png_tool"])
    subprocess.check_call(["make", "-s", "-C", PKG])
    W, H = 160, 96
    a, b = disflow_mod.synth_pair(50, W, H)
    c, _ = disflow_mod.synth_pair(51, W, H)
    frames = [a, b, c]  # two pairs: (a, b) moves smoothly, (b, c) are unrelated frames
    d = tmp_path / "seq"
    d.mkdir()
    for k, f in enumerate(frames):
        pngio.write_gray8(str(d / f"frame_{k + 1:04d}.png"), f)
    args = [cli, "seq", "1", "3", "10", "8", "3", "1", "0.5", "1", "0", "--flo", "--warp"] + extra
    r = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in range(2):
        base = str(tmp_path / f"OF_seq/frame_{k + 1:04d}")
        flow = disflow_mod.read_flo(base + ".flo")
        raw_path = str(tmp_path / "warp.raw")
        subprocess.run([png_tool, "gray", base + "_warp.png", raw_path], check=True)
        raw = open(raw_path, "rb").read()
        assert struct.unpack("<ii", raw[:8]) == (W, H)
        got = np.frombuffer(raw[8:], np.uint8).reshape(H, W)
        _assert_same(got, disflow_mod.flow_warp(frames[k + 1], flow), f"pair {k}: warp PNG")
        assert f"warp seq/frame_{k + 1:04d}.png: mean |warped - first| " in r.stdout
