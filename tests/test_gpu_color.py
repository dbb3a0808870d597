"""GPU tests of colour frame input: the luma kernel (dis_frames_to_gray_u8)
against its numpy restatement (tests/lumaref.py) in every layout that selects
another load / store form, and a context with a colour frame format against a
gray context on the restatement's gray frames -- device, graph replay, eager,
bidirectional, warm-started, chunked host pipeline, format changes, f16 flows,
interpolation and the CLI's --color. Every comparison is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import lumaref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")


def _assert_same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    bad = g.view(np.uint8) != e.view(np.uint8)
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first at byte "
                             f"{int(np.flatnonzero(bad.reshape(-1))[0])}")


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
WIDTHS = [1, 15, 16, 17, 37, 80]  # below one group, one exact group, a partial last group, several groups
KH, KN = 3, 2
LAYOUTS = ["tight", "aligned", "odd"]
_frames = {}


def kernel_frames(fmt, W):
    """Random bytes, (KN, KH, W, C) ((KN, KH, W) for gray), and the restatement's gray: made once."""
    key = (fmt, W)
    if key not in _frames:
        C = lumaref.channels(fmt)
        rng = np.random.default_rng(1000 * lumaref.FORMATS[fmt][0] + W)
        a = rng.integers(0, 256, (KN, KH, W) + ((C,) if C > 1 else ()), dtype=np.uint8)
        g = lumaref.to_gray(a, fmt)
        a.setflags(write=False)
        g.setflags(write=False)
        _frames[key] = (a, g)
    return _frames[key]


def _lay_out(rows, stride, image_stride, lead, fill):
    """(n, H, row_bytes) rows placed in a flat buffer of `fill` bytes: image k's
    row y at lead + k * image_stride + y * stride. The buffer ends with the
    last row's last byte plus 32 bytes of fill."""
    n, H, rb = rows.shape
    buf = np.full(lead + (n - 1) * image_stride + (H - 1) * stride + rb + 32, fill, np.uint8)
    for k in range(n):
        for y in range(H):
            o = lead + k * image_stride + y * stride
            buf[o:o + rb] = rows[k, y]
    return buf


def _strides(layout, row_bytes):
    """(row stride, image stride, lead bytes from a 256-byte-aligned base; None = the call's 0)"""
    if layout == "tight":
        return row_bytes, row_bytes * KH, 0
    if layout == "aligned":  # rows and images padded to multiples of 16, from an aligned base
        st = (row_bytes + 15) // 16 * 16 + 16
        return st, st * KH + 32, 0
    st = row_bytes + 5 + (row_bytes % 2)  # odd stride, base 1 byte in: the general path
    return st, st * KH + 7, 1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("fmt", list(lumaref.COLOUR) + ["gray"])
def test_frames_to_gray_device_matches_restatement(disflow_mod, fmt, W, layout):
    import torch
    src, exp = kernel_frames(fmt, W)
    C = lumaref.channels(fmt)
    s_st, s_img, lead = _strides(layout, W * C)
    d_st, d_img, _ = _strides(layout, W)
    if layout == "odd":
        assert s_st % 2 == 1 and d_st % 2 == 1
    src_buf = _lay_out(src.reshape(KN, KH, W * C), s_st, s_img, lead, 0xA5)  # the padding holds other bytes
    dst_buf = _lay_out(np.full((KN, KH, W), 0x5A, np.uint8), d_st, d_img, 16 + lead, 0x5A)  # sentinel all over
    tsrc = torch.from_numpy(src_buf).cuda()
    tdst = torch.from_numpy(dst_buf).cuda()
    assert tsrc.data_ptr() % 256 == 0 and tdst.data_ptr() % 256 == 0
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    tight = layout == "tight"
    disflow_mod.frames_to_gray_device(tsrc.data_ptr() + lead, fmt, KN, W, KH, tdst.data_ptr() + 16 + lead,
                                      src_stride=0 if tight else s_st, src_image_stride=0 if tight else s_img,
                                      dst_stride=0 if tight else d_st, dst_image_stride=0 if tight else d_img,
                                      stream=s.cuda_stream)
    s.synchronize()
    want = _lay_out(exp.reshape(KN, KH, W), d_st, d_img, 16 + lead, 0x5A)  # the gray bytes, the sentinel elsewhere
    _assert_same(tdst.cpu().numpy(), want, f"{fmt} W={W} {layout}")
    _assert_same(tsrc.cpu().numpy(), src_buf, "the source")


def test_frames_to_gray_host_form(disflow_mod):
    for fmt in ("bgr", "rgba", "gray"):
        src, exp = kernel_frames(fmt, 37)
        _assert_same(disflow_mod.frames_to_gray(src, fmt), exp, fmt)
        _assert_same(disflow_mod.frames_to_gray(src[0], fmt), exp[0], fmt + ", one frame")
    # strided host buffers through the C entry: the destination's padding keeps its bytes
    src, exp = kernel_frames("rgb", 37)
    s_st, s_img, d_st, d_img = 37 * 3 + 4, (37 * 3 + 4) * KH + 9, 37 + 3, (37 + 3) * KH + 5
    sb = _lay_out(src.reshape(KN, KH, 37 * 3), s_st, s_img, 0, 0xA5)
    db = _lay_out(np.full((KN, KH, 37), 0x5A, np.uint8), d_st, d_img, 3, 0x5A)
    st = disflow_mod.lib().dis_frames_to_gray_u8(sb.ctypes.data, s_st, s_img, lumaref.FORMATS["rgb"][0], KN, 37, KH,
                                                 db.ctypes.data + 3, d_st, d_img, disflow_mod.MEM_HOST, None, 0)
    assert st == disflow_mod.DIS_OK, disflow_mod.lib().dis_last_error()
    _assert_same(db, _lay_out(exp, d_st, d_img, 3, 0x5A), "strided host call")


# ---------------------------------------------------------------------------
# 2.-6. a colour context against a gray context
# ---------------------------------------------------------------------------
def _params(S):
    return S.Params(coarsest_scale=3, finest_scale=1, patch_size=8, iterations=12, patch_overlap=0.5,
                    patch_normalization=1)


_colour = {}


def colour_pairs(S, W, H, n, C):
    """n synthetic pairs as colour frames whose channels differ: the gray pair
    plus per-channel noise (and random alpha for C = 4). (n, H, W, C) each."""
    key = (W, H, n, C)
    if key not in _colour:
        rng = np.random.default_rng(7000 + W + H + 10 * n + C)
        out = []
        for role in range(2):
            frames = np.stack([S.synth_pair(300 + k, W, H)[role] for k in range(n)])
            col = frames[..., None].astype(np.int32) + rng.integers(-40, 41, (n, H, W, C))
            col = np.clip(col, 0, 255).astype(np.uint8)
            if C == 4:
                col[..., 3] = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
            col.setflags(write=False)
            out.append(col)
        _colour[key] = tuple(out)
    return _colour[key]


_oracle_cache = {}


def oracle_flow(oracle, I0, I1, p):
    key = (I0.tobytes(), I1.tobytes(), I0.shape)
    if key not in _oracle_cache:
        out = oracle.calc_from_params(np.ascontiguousarray(I0), np.ascontiguousarray(I1), p)
        out.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _device_calc(eng, I0, I1, dtype=np.float32, bufs=None):
    """calc_device on torch buffers (kept in `bufs` across calls, so that a
    second call has the first one's graph key) -> the flows on the host."""
    import torch
    n, H, W = I0.shape[:3]
    if bufs is None or "d0" not in bufs:
        b = bufs if bufs is not None else {}
        b["d0"], b["d1"] = torch.from_numpy(np.array(I0)).cuda(), torch.from_numpy(np.array(I1)).cuda()
        b["out"] = torch.zeros((n, H, W, 2), dtype=torch.float16 if dtype == np.float16 else torch.float32,
                               device="cuda")
        b["s"] = torch.cuda.Stream()
        bufs = b
    torch.cuda.synchronize()
    with torch.cuda.stream(bufs["s"]):
        bufs["out"].fill_(-7.0)
    eng.calc_device(n, bufs["d0"].data_ptr(), bufs["d1"].data_ptr(), bufs["out"].data_ptr(),
                    stream=bufs["s"].cuda_stream)
    bufs["s"].synchronize()
    return bufs["out"].cpu().numpy()


@pytest.mark.parametrize("fmt", ["bgr", "rgba"])
@pytest.mark.parametrize("size", [(96, 80), (101, 67)], ids=["96x80", "101x67"])
def test_colour_calc_equals_gray_calc_and_oracle(disflow_mod, oracle, size, fmt):
    S = disflow_mod
    W, H = size
    n, p = 3, _params(S)
    C0, C1 = colour_pairs(S, W, H, n, lumaref.channels(fmt))
    G0, G1 = lumaref.to_gray(C0, fmt), lumaref.to_gray(C1, fmt)
    assert not np.array_equal(C0[..., 0], C0[..., 1]) and not np.array_equal(C0[..., 1], C0[..., 2])
    gray = S.DenseInverseSearch(p, W, H, max_batch=n)
    gray.set_concurrency(2)
    exp = _device_calc(gray, G0, G1)
    gray.close()
    for k in range(n):
        _assert_same(exp[k], oracle_flow(oracle, G0[k], G1[k], p), f"gray context against the oracle, pair {k}")
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, frame_format=fmt)
    eng.set_concurrency(2)  # sub-batches of 1 and 2 pairs: the second one's slice starts at pair 1
    bufs = {}
    _assert_same(_device_calc(eng, C0, C1, bufs=bufs), exp, "graphs on, capture")
    _assert_same(_device_calc(eng, C0, C1, bufs=bufs), exp, "graphs on, replay")
    eng.set_graphs(False)
    _assert_same(_device_calc(eng, C0, C1, bufs=bufs), exp, "graphs off")
    eng.close()


def test_colour_bidir_warm_and_host_calls(disflow_mod):
    S = disflow_mod
    W, H, n, fmt = 96, 80, 3, "bgr"
    p = _params(S)
    C0, C1 = colour_pairs(S, W, H, n, 3)
    G0, G1 = lumaref.to_gray(C0, fmt), lumaref.to_gray(C1, fmt)
    gray = S.DenseInverseSearch(p, W, H, max_batch=n)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, frame_format=fmt)
    # the chunked host pipeline: chunks of 2 and 1 pairs
    gray.set_host_pipeline(2)
    eng.set_host_pipeline(2)
    exp = gray.calc_batch(G0, G1)
    _assert_same(eng.calc_batch(C0, C1), exp, "chunked host pipeline")
    assert eng.host_pipeline_info()["last_chunks"] == 2
    # the host form of the bidirectional call
    efw, ebw = gray.calc_bidir_batch(G0, G1)
    fw, bw = eng.calc_bidir_batch(C0, C1)
    _assert_same(fw, efw, "host bidir, forward")
    _assert_same(bw, ebw, "host bidir, backward")
    _assert_same(efw, exp, "the forward flow is the plain call's")
    assert not np.array_equal(efw, ebw)
    # its device form
    import torch
    d0, d1 = torch.from_numpy(np.array(C0)).cuda(), torch.from_numpy(np.array(C1)).cuda()
    ofw = torch.zeros((n, H, W, 2), dtype=torch.float32, device="cuda")
    obw = torch.zeros_like(ofw)
    st = torch.cuda.current_stream()
    eng.calc_bidir_device(n, d0.data_ptr(), d1.data_ptr(), ofw.data_ptr(), obw.data_ptr(), st.cuda_stream)
    st.synchronize()
    _assert_same(ofw.cpu().numpy(), efw, "device bidir, forward")
    _assert_same(obw.cpu().numpy(), ebw, "device bidir, backward")
    # warm start from the previous output (host form: staged)
    ewarm = gray.calc_batch(G0, G1, init=exp)
    _assert_same(eng.calc_batch(C0, C1, init=exp), ewarm, "warm-started host call")
    gray.close()
    eng.close()


def test_format_changes_on_one_context(disflow_mod):
    S = disflow_mod
    W, H, n = 96, 80, 2
    p = _params(S)
    B0, B1 = colour_pairs(S, W, H, n, 3)
    R0, R1 = colour_pairs(S, W, H, n, 4)
    GB0, GB1 = lumaref.to_gray(B0, "bgr"), lumaref.to_gray(B1, "bgr")
    GR0, GR1 = lumaref.to_gray(R0, "rgba"), lumaref.to_gray(R1, "rgba")
    fresh = S.DenseInverseSearch(p, W, H, max_batch=n)
    exp_b, exp_r = _device_calc(fresh, GB0, GB1), _device_calc(fresh, GR0, GR1)
    exp_b_host = fresh.calc_batch(GB0, GB1)
    fresh.close()
    _assert_same(exp_b_host, exp_b, "host and device paths of the gray context")
    assert not np.array_equal(exp_b, exp_r)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n)
    gb, cb, cr = {}, {}, {}  # one buffer set per input: the same graph keys come back
    for step, fmt in enumerate(["gray", "bgr", "gray", "rgba"]):
        eng.set_frame_format(fmt)
        assert eng.frame_format == fmt
        if fmt == "gray":
            _assert_same(_device_calc(eng, GB0, GB1, bufs=gb), exp_b, f"step {step} gray, device")
            _assert_same(eng.calc_batch(GB0, GB1), exp_b, f"step {step} gray, host")
        elif fmt == "bgr":
            _assert_same(_device_calc(eng, B0, B1, bufs=cb), exp_b, f"step {step} bgr, device")
            _assert_same(eng.calc_batch(B0, B1), exp_b, f"step {step} bgr, host")
        else:
            _assert_same(_device_calc(eng, R0, R1, bufs=cr), exp_r, f"step {step} rgba, device")
            _assert_same(eng.calc_batch(R0, R1), exp_r, f"step {step} rgba, host")
    # colour frames handed to a gray context: the wrong shape, refused
    eng.set_frame_format("gray")
    with pytest.raises(S.DisError):
        eng.calc_batch(B0, B1)
    eng.close()


def test_f16_flows_from_rgb_frames(disflow_mod):
    S = disflow_mod
    W, H, n = 96, 80, 2
    p = _params(S)
    C0, C1 = colour_pairs(S, W, H, n, 3)
    G0, G1 = lumaref.to_gray(C0, "rgb"), lumaref.to_gray(C1, "rgb")
    gray = S.DenseInverseSearch(p, W, H, max_batch=n, flow_dtype=np.float16)
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, flow_dtype=np.float16, frame_format="rgb")
    exp = _device_calc(gray, G0, G1, np.float16)
    assert exp.dtype == np.float16
    _assert_same(_device_calc(eng, C0, C1, np.float16), exp, "device")
    _assert_same(eng.calc_batch(C0, C1), exp, "host")
    # rgb and bgr weigh the outer channels differently: another gray frame, another flow
    eng.set_frame_format("bgr")
    assert not np.array_equal(eng.calc_batch(C0, C1), exp)
    gray.close()
    eng.close()


def test_interpolate_on_a_colour_context(disflow_mod):
    S = disflow_mod
    W, H = 96, 80
    p = _params(S)
    C0, C1 = (a[0] for a in colour_pairs(S, W, H, 3, 3))
    G0, G1 = lumaref.to_gray(C0, "bgr"), lumaref.to_gray(C1, "bgr")
    gray = S.DenseInverseSearch(p, W, H)
    fw, bw = gray.calc_bidir(G0, G1)
    gray.close()
    eng = S.DenseInverseSearch(p, W, H, frame_format="bgr")
    ts = [0.25, 0.5]
    got = eng.interpolate(C0, C1, ts)
    eng.close()
    assert len(got) == 2
    for t, g in zip(ts, got):
        assert g.shape == (H, W, 3) and g.dtype == np.uint8
        _assert_same(g, S.flow_interp(C0, C1, fw, t, bw=bw), f"t = {t}")
    assert not np.array_equal(got[0], got[1])


def test_cpp_facade_color(tmp_path):
    # tests/cpp/test_color.cpp: dis::framesToGray, set_frame_format and the calc overloads on BGR / RGBA frames
    exe = str(tmp_path / "test_color")
    lib_dir = os.path.join(PKG, "disflow")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_color.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout


# ---------------------------------------------------------------------------
# 7. the CLI
# ---------------------------------------------------------------------------
def test_cli_color(disflow_mod, tmp_path):
    import pngio
    S = disflow_mod
    cli = os.path.join(PKG, "disflow", "dis_flow")
    subprocess.check_call(["make", "-s", "-C", PKG])
    W, H = 64, 48
    rng = np.random.default_rng(11)
    frames = []
    for k, f in enumerate([S.synth_pair(60, W, H)[0], S.synth_pair(60, W, H)[1], S.synth_pair(61, W, H)[1]]):
        col = np.clip(f[..., None].astype(np.int32) + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)
        frames.append(col)  # RGB
    for name in ("plain", "color"):
        d = tmp_path / name
        d.mkdir()
        for k, f in enumerate(frames):
            pngio.write_png(str(d / f"frame_{k + 1:04d}.png"), f, 2, 8)
    common = ["1", "3", "10", "8", "3", "1", "0.5", "1", "0", "--flo", "--bidir"]
    r = subprocess.run([cli, "plain"] + common, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([cli, "color"] + common + ["--color", "--interp", "1"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in range(2):
        a = (tmp_path / f"OF_plain/frame_{k + 1:04d}.flo").read_bytes()
        b = (tmp_path / f"OF_color/frame_{k + 1:04d}.flo").read_bytes()
        assert len(a) == 12 + W * H * 8 and a == b, f"pair {k}: .flo files differ"
        assert ((tmp_path / f"OF_plain/frame_{k + 1:04d}.png").read_bytes() ==
                (tmp_path / f"OF_color/frame_{k + 1:04d}.png").read_bytes()), f"pair {k}: colour coding differs"
        fw = S.read_flo(str(tmp_path / f"OF_color/frame_{k + 1:04d}.flo"))
        bw = S.read_flo(str(tmp_path / f"OF_color/frame_{k + 1:04d}_bw.flo"))
        got = pngio.read_rgb8(str(tmp_path / f"OF_color/frame_{k + 1:04d}_interp_1.png"))
        _assert_same(got, S.flow_interp(frames[k], frames[k + 1], fw, 0.5, bw=bw), f"pair {k}: interpolated frame")
    # the flows are those of the luma frames
    p = S.Params(coarsest_scale=3, finest_scale=1, patch_size=8, iterations=10, patch_overlap=0.5,
                 patch_normalization=1)
    eng = S.DenseInverseSearch(p, W, H)
    exp = eng.calc(lumaref.to_gray(frames[0], "rgb"), lumaref.to_gray(frames[1], "rgb"))
    eng.close()
    _assert_same(S.read_flo(str(tmp_path / "OF_color/frame_0001.flo")), exp, "the flow of the luma frames")
