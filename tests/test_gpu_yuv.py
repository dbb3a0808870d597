"""GPU tests of the 4:2:0 conversions (dis_yuv420_to_frames_u8,
dis_frames_to_yuv420_u8; csrc/dis_yuv.hip) against their numpy restatement
(tests/yuvref.py), bit for bit: every layout, frame format and (matrix, range)
row, at sizes and offsets that select each vector and byte form of each side,
with every padding byte of every output plane watched; the host forms; all 2^24
(Y, Cb, Cr) triples and all 2^24 colours; and the Y planes of converted frames
going into the engine in place."""
import numpy as np
import pytest

import lumaref
import yuvref

pytestmark = pytest.mark.gpu

FORMATS = ["gray", "bgr", "rgb", "bgra", "rgba"]
SENTINEL = 0x5A


def _assert_same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    bad = g.view(np.uint8) != e.view(np.uint8)
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first at byte "
                             f"{int(np.flatnonzero(bad.reshape(-1))[0])}")


# ---------------------------------------------------------------------------
# shared data: random surfaces and frames with their restated conversions, made once
# ---------------------------------------------------------------------------
_cache = {}


def surface_case(W, H, n, fmt, row, alpha):
    """Random planes (Y, Cb, Cr) and the restatement's frames of them."""
    key = ("s", W, H, n, fmt, row, alpha)
    if key not in _cache:
        rng = np.random.default_rng(10 * W + H + n)
        y = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
        cb = rng.integers(0, 256, (n, H // 2, W // 2), dtype=np.uint8)
        cr = rng.integers(0, 256, (n, H // 2, W // 2), dtype=np.uint8)
        out = yuvref.to_frames(y, cb, cr, fmt, row[0], row[1], alpha)
        for a in (y, cb, cr, out):
            a.setflags(write=False)
        _cache[key] = (y, cb, cr, out)
    return _cache[key]


def frames_case(W, H, n, fmt, row):
    """Random frames (non-uniform blocks) and the restatement's planes of them."""
    key = ("f", W, H, n, fmt, row)
    if key not in _cache:
        C = lumaref.channels(fmt)
        rng = np.random.default_rng(7 * W + 3 * H + n + C)
        f = rng.integers(0, 256, (n, H, W) + ((C,) if C > 1 else ()), dtype=np.uint8)
        planes = yuvref.to_yuv420(f, fmt, row[0], row[1])
        for a in (f,) + planes:
            a.setflags(write=False)
        _cache[key] = (f,) + planes
    return _cache[key]


def _surface_geometry(layout, W, H, n, padded, y_off, c_off):
    """Where the planes of n images lie in one flat buffer: the layout's offsets
    (tests/yuvref.py), rows and images padded to multiples of 16 when `padded`
    (else tight), the Y planes moved y_off bytes and the chroma planes c_off
    bytes from there. -> (lay, image_stride, base, bytes)."""
    ys = (W + 15) // 16 * 16 + 32 if padded else 0
    gap = 16 if padded or y_off or c_off else 0
    lay = dict(yuvref.surface_layout(layout, W, H, ys, gap))
    image = lay["bytes"] + (48 if padded else 0)
    if padded:
        assert lay["y_stride"] % 16 == 0 and lay["c_stride"] % 8 == 0 and image % 16 == 0
    lay["y"] += y_off
    lay["cb"] += c_off
    lay["cr"] += c_off
    base = 32
    return lay, image, base, base + n * image + 64


def _frames_geometry(W, H, C, n, padded, p_off):
    st = (W * C + 15) // 16 * 16 + 16 if padded else W * C
    image = st * H + (32 if padded else 0)
    base = 32 + p_off
    return st, image, base, base + n * image + 64


def _place_frames(buf, base, st, image, frames):
    n, H = frames.shape[:2]
    rows = frames.reshape(n, H, -1)
    for i in range(n):
        for r in range(H):
            o = base + i * image + r * st
            buf[o:o + rows.shape[2]] = rows[i, r]
    return buf


def _to_frames_device(S, layout, W, H, n, fmt, row, alpha, padded, offs):
    import torch
    y, cb, cr, exp = surface_case(W, H, n, fmt, row, alpha)
    C = lumaref.channels(fmt)
    lay, simg, sbase, sbytes = _surface_geometry(layout, W, H, n, padded, offs[0], offs[1])
    st, pimg, pbase, pbytes = _frames_geometry(W, H, C, n, padded, offs[2])
    src = yuvref.place(np.full(sbytes, 0xA5, np.uint8), sbase, lay, simg, y, cb, cr)
    dst = np.full(pbytes, SENTINEL, np.uint8)
    tsrc, tdst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    assert tsrc.data_ptr() % 256 == 0 and tdst.data_ptr() % 256 == 0
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    p = tsrc.data_ptr() + sbase
    tight = not padded and not any(offs)
    gray = fmt == "gray"
    S.yuv420_to_frames_device(
        p + lay["y"], 0 if gray else p + lay["cb"], 0 if gray else p + lay["cr"], lay["c_step"], n, W, H,
        tdst.data_ptr() + pbase, fmt, row[0], row[1], alpha,
        y_stride=0 if tight else lay["y_stride"], y_image_stride=simg, c_stride=0 if tight else lay["c_stride"],
        c_image_stride=simg, dst_stride=0 if tight else st, dst_image_stride=0 if tight else pimg,
        stream=s.cuda_stream)
    s.synchronize()
    what = f"to frames: {layout} {W}x{H} n={n} {fmt} {row} padded={padded} offsets={offs}"
    _assert_same(tdst.cpu().numpy(), _place_frames(dst.copy(), pbase, st, pimg, exp), what)
    _assert_same(tsrc.cpu().numpy(), src, what + ": the source")


def _from_frames_device(S, layout, W, H, n, fmt, row, padded, offs):
    import torch
    f, y, cb, cr = frames_case(W, H, n, fmt, row)
    C = lumaref.channels(fmt)
    lay, simg, sbase, sbytes = _surface_geometry(layout, W, H, n, padded, offs[0], offs[1])
    st, pimg, pbase, pbytes = _frames_geometry(W, H, C, n, padded, offs[2])
    src = _place_frames(np.full(pbytes, 0xA5, np.uint8), pbase, st, pimg, f)
    dst = np.full(sbytes, SENTINEL, np.uint8)
    tsrc, tdst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    p = tdst.data_ptr() + sbase
    tight = not padded and not any(offs)
    S.frames_to_yuv420_device(
        tsrc.data_ptr() + pbase, fmt, n, W, H, p + lay["y"], p + lay["cb"], p + lay["cr"], lay["c_step"],
        row[0], row[1], src_stride=0 if tight else st, src_image_stride=0 if tight else pimg,
        y_stride=0 if tight else lay["y_stride"], y_image_stride=simg, c_stride=0 if tight else lay["c_stride"],
        c_image_stride=simg, stream=s.cuda_stream)
    s.synchronize()
    what = f"from frames: {layout} {W}x{H} n={n} {fmt} {row} padded={padded} offsets={offs}"
    # the samples where they belong, and the sentinel in every other byte: the planes' padding, the bytes
    # between the planes and between the images
    _assert_same(tdst.cpu().numpy(), yuvref.place(dst.copy(), sbase, lay, simg, y, cb, cr), what)
    _assert_same(tsrc.cpu().numpy(), src, what + ": the source")


# 2 x 2: one block; 18 x 4: a full strip and a partial one; 32 x 2: full strips only, one row of them;
# 50 x 6: three full strips and a pair, three strip rows (four strips a row, the last partial: no quad of lanes
# stores together); 64 x 2 and 128 x 4: one and two quads of full strips a row, which store their packed rows
# together; 114 x 2: eight strips a row, the first quad full, the second with a partial strip
SIZES = [(2, 2), (18, 4), (32, 2), (50, 6), (64, 2), (128, 4), (114, 2)]
# (Y, chroma, frames) bases moved by a byte each in turn: the side goes byte by byte, the others keep their form
OFFSETS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
ROW = ("bt601", "limited")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", yuvref.LAYOUTS)
def test_to_frames_device_every_form(disflow_mod, layout, size):
    W, H = size
    for padded in (False, True):
        for offs in OFFSETS:
            for fmt, alpha in (("bgr", 255), ("rgba", 200), ("gray", 255)):
                _to_frames_device(disflow_mod, layout, W, H, 3, fmt, ROW, alpha, padded, offs)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", yuvref.LAYOUTS)
def test_from_frames_device_every_form(disflow_mod, layout, size):
    W, H = size
    for padded in (False, True):
        for offs in OFFSETS:
            for fmt in ("bgr", "rgba", "gray"):
                _from_frames_device(disflow_mod, layout, W, H, 3, fmt, ROW, padded, offs)


@pytest.mark.parametrize("row", yuvref.ROWS, ids="-".join)
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_and_row(disflow_mod, fmt, row):
    # 50 x 6 padded (the vector forms and a partial strip) and tight (the byte forms), NV12 and I420
    for layout in ("nv12", "i420"):
        for padded in (True, False):
            for alpha in (0, 200):
                _to_frames_device(disflow_mod, layout, 50, 6, 2, fmt, row, alpha, padded, (0, 0, 0))
            _from_frames_device(disflow_mod, layout, 50, 6, 2, fmt, row, padded, (0, 0, 0))


def test_one_image_ignores_its_image_strides(disflow_mod):
    # n = 1 with image strides that are no multiple of 16 still takes the vector forms (same bytes either way)
    import torch
    S = disflow_mod
    W, H = 64, 4
    f, y, cb, cr = frames_case(W, H, 1, "bgra", ("bt709", "full"))
    lay = yuvref.surface_layout("nv12", W, H)
    tsrc = torch.from_numpy(np.array(f)).cuda()
    tdst = torch.full((lay["bytes"] + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    S.frames_to_yuv420_device(tsrc.data_ptr(), "bgra", 1, W, H, tdst.data_ptr(), tdst.data_ptr() + lay["cb"],
                              tdst.data_ptr() + lay["cr"], 2, "bt709", "full", src_image_stride=W * H * 4 + 7,
                              y_image_stride=lay["bytes"] + 3, c_image_stride=lay["bytes"] + 5)
    torch.cuda.synchronize()
    want = yuvref.place(np.full(lay["bytes"] + 16, SENTINEL, np.uint8), 0, lay, 0, y, cb, cr)
    _assert_same(tdst.cpu().numpy(), want, "one image, odd image strides")


def test_larger_random_frames_round_trip_through_both_kernels(disflow_mod):
    # several blocks of lanes (210 x 34 x 5 images: 14 strips x 17 rows x 5 > 256 lanes), non-uniform 2 x 2 blocks
    S = disflow_mod
    W, H, n = 210, 34, 5
    for layout in ("nv12", "yv12"):
        _from_frames_device(S, layout, W, H, n, "rgb", ("bt709", "limited"), True, (0, 0, 0))
        _to_frames_device(S, layout, W, H, n, "bgra", ("bt601", "full"), 17, True, (0, 0, 0))


# ---------------------------------------------------------------------------
# host pointers
# ---------------------------------------------------------------------------
def _nv12_buffer(y, cb, cr):
    n, H, W = y.shape
    buf = np.empty((n, H * 3 // 2, W), np.uint8)
    buf[:, :H] = y
    buf[:, H:, 0::2] = cb
    buf[:, H:, 1::2] = cr
    return buf


def _i420_buffer(y, cb, cr):
    n, H, W = y.shape
    return np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], axis=1).reshape(n, H * 3 // 2, W)


def test_host_forms(disflow_mod):
    S = disflow_mod
    W, H, n = 50, 6, 3
    for fmt, row, alpha in (("bgr", ("bt601", "limited"), 255), ("rgba", ("bt709", "full"), 9),
                            ("gray", ("bt601", "limited"), 255)):
        y, cb, cr, exp = surface_case(W, H, n, fmt, row, alpha)
        nv12, i420 = _nv12_buffer(y, cb, cr), _i420_buffer(y, cb, cr)
        _assert_same(S.nv12_to_frames(nv12, fmt, row[0], row[1], alpha), exp, f"nv12_to_frames {fmt}")
        _assert_same(S.i420_to_frames(i420, fmt, row[0], row[1], alpha), exp, f"i420_to_frames {fmt}")
        _assert_same(S.nv12_to_frames(nv12[0], fmt, row[0], row[1], alpha), exp[0], f"nv12_to_frames {fmt}, one")
        f, y, cb, cr = frames_case(W, H, n, fmt, row)
        _assert_same(S.frames_to_nv12(f, fmt, row[0], row[1]), _nv12_buffer(y, cb, cr), f"frames_to_nv12 {fmt}")
        _assert_same(S.frames_to_i420(f, fmt, row[0], row[1]), _i420_buffer(y, cb, cr), f"frames_to_i420 {fmt}")
        _assert_same(S.frames_to_i420(f[1], fmt, row[0], row[1]), _i420_buffer(y, cb, cr)[1], f"frames_to_i420 {fmt}, one")
        _assert_same(S.nv12_luma(S.frames_to_nv12(f, fmt, row[0], row[1])), y, "nv12_luma")
    # defaults: BT.601 limited, alpha 255
    y, cb, cr, exp = surface_case(W, H, n, "bgra", ("bt601", "limited"), 255)
    _assert_same(S.nv12_to_frames(_nv12_buffer(y, cb, cr), "bgra"), exp, "defaults")


@pytest.mark.parametrize("layout", ["nv12", "yv12"])
def test_strided_host_calls_keep_every_other_byte(disflow_mod, layout):
    # padded surfaces of 3 images in one host buffer (the planes lie inside each other's extents) through the C
    # entries: the samples arrive, every padding byte and every byte between the planes keeps its value
    S = disflow_mod
    L = S.lib()
    W, H, n, fmt, row = 50, 6, 3, "bgr", ("bt709", "limited")
    lay, simg, sbase, sbytes = _surface_geometry(layout, W, H, n, True, 1, 0)
    st, pimg, pbase, pbytes = _frames_geometry(W, H, 3, n, True, 1)
    f, y, cb, cr = frames_case(W, H, n, fmt, row)
    src = _place_frames(np.full(pbytes, 0xA5, np.uint8), pbase, st, pimg, f)
    dst = np.full(sbytes, SENTINEL, np.uint8)
    p = dst.ctypes.data + sbase
    status = L.dis_frames_to_yuv420_u8(src.ctypes.data + pbase, st, pimg, 1, 1, 0, n, W, H, p + lay["y"], lay["y_stride"],
                                       simg, p + lay["cb"], p + lay["cr"], lay["c_stride"], simg, lay["c_step"],
                                       S.MEM_HOST, None, 0)
    assert status == S.DIS_OK, L.dis_last_error()
    _assert_same(dst, yuvref.place(np.full(sbytes, SENTINEL, np.uint8), sbase, lay, simg, y, cb, cr), "host, from frames")
    y, cb, cr, exp = surface_case(W, H, n, fmt, row, 255)
    src = yuvref.place(np.full(sbytes, 0xA5, np.uint8), sbase, lay, simg, y, cb, cr)
    dst = np.full(pbytes, SENTINEL, np.uint8)
    p = src.ctypes.data + sbase
    status = L.dis_yuv420_to_frames_u8(p + lay["y"], lay["y_stride"], simg, p + lay["cb"], p + lay["cr"], lay["c_stride"],
                                       simg, lay["c_step"], 1, 0, n, W, H, dst.ctypes.data + pbase, st, pimg, 1, 255,
                                       S.MEM_HOST, None, 0)
    assert status == S.DIS_OK, L.dis_last_error()
    _assert_same(dst, _place_frames(np.full(pbytes, SENTINEL, np.uint8), pbase, st, pimg, exp), "host, to frames")


# ---------------------------------------------------------------------------
# exhaustive
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", yuvref.ROWS, ids="-".join)
def test_to_frames_on_every_triple(disflow_mod, row):
    # a 4096 x 4096 NV12 surface holding every (Y, Cb, Cr): block b has the chroma pair b >> 6 and the four
    # luma values 4 * (b & 63) .. + 3
    import torch
    S = disflow_mod
    W = H = 4096
    if "triples" not in _cache:
        b = np.arange((W // 2) * (H // 2), dtype=np.uint32).reshape(H // 2, W // 2)
        cb, cr = ((b >> 6) >> 8).astype(np.uint8), ((b >> 6) & 255).astype(np.uint8)
        y = np.empty((H, W), np.uint8)
        for dy in range(2):
            for dx in range(2):
                y[dy::2, dx::2] = ((b & 63) * 4 + 2 * dy + dx).astype(np.uint8)
        triples = (y.astype(np.uint32) << 16 | np.repeat(np.repeat(cb, 2, 0), 2, 1).astype(np.uint32) << 8 |
                   np.repeat(np.repeat(cr, 2, 0), 2, 1))
        assert np.array_equal(np.bincount(triples.reshape(-1), minlength=1 << 24), np.ones(1 << 24, np.int64))
        _cache["triples"] = (y, cb, cr)
    y, cb, cr = _cache["triples"]
    surf = torch.from_numpy(_nv12_buffer(y[None], cb[None], cr[None])).cuda()
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    p = surf.data_ptr()
    S.yuv420_to_frames_device(p, p + W * H, p + W * H + 1, 2, 1, W, H, out.data_ptr(), "bgra", row[0], row[1], 77,
                              y_stride=W, c_stride=W)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for r0 in range(0, H, 512):  # (the restatement in slabs: less memory)
        exp = yuvref.to_frames(y[r0:r0 + 512], cb[r0 // 2:r0 // 2 + 256], cr[r0 // 2:r0 // 2 + 256], "bgra", row[0],
                               row[1], 77)
        _assert_same(got[r0:r0 + 512], exp, f"every triple, {row}, rows {r0}..")


@pytest.mark.parametrize("row", yuvref.ROWS, ids="-".join)
def test_from_frames_on_every_colour(disflow_mod, row):
    # 8192 x 8192 BGR frames holding every colour in a uniform 2 x 2 block: block b is the colour b
    # (R << 16 | G << 8 | B). The restatement's formulas on the 4096 x 4096 colours: Y of a pixel, chroma of
    # the sums 4 R, 4 G, 4 B.
    import torch
    S = disflow_mod
    W = H = 8192
    b = np.arange(1 << 24, dtype=np.uint32).reshape(H // 2, W // 2)
    R, G, B = (b >> 16).astype(np.uint8), ((b >> 8) & 255).astype(np.uint8), (b & 255).astype(np.uint8)
    col = np.stack([B, G, R], axis=-1)
    frames = torch.from_numpy(col).cuda().repeat_interleave(2, 0).repeat_interleave(2, 1).contiguous()
    assert tuple(frames.shape) == (H, W, 3)
    surf = torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    p = surf.data_ptr()
    S.frames_to_yuv420_device(frames.data_ptr(), "bgr", 1, W, H, p, p + W * H, p + W * H + 1, 2, row[0], row[1],
                              y_stride=W, c_stride=W)
    torch.cuda.synchronize()
    got = surf.cpu().numpy()
    del frames, surf
    ey = yuvref.rgb_to_y(R, G, B, row[0], row[1]).astype(np.uint8)
    _assert_same(got[:H:2, 0::2], ey, f"every colour, {row}: Y, pixel (0, 0) of the blocks")
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        assert np.array_equal(got[dy:H:2, dx::2], ey), f"every colour, {row}: Y, pixel ({dx}, {dy}) of the blocks"
    ecb, ecr = yuvref.sums_to_chroma(4 * R.astype(np.int32), 4 * G.astype(np.int32), 4 * B.astype(np.int32), row[0], row[1])
    _assert_same(got[H:, 0::2], ecb.astype(np.uint8), f"every colour, {row}: Cb")
    _assert_same(got[H:, 1::2], ecr.astype(np.uint8), f"every colour, {row}: Cr")


# ---------------------------------------------------------------------------
# the chain: converted frames' Y planes into the engine, in place
# ---------------------------------------------------------------------------
def test_nv12_luma_planes_feed_the_engine_in_place(disflow_mod):
    import torch
    S = disflow_mod
    W, H, n = 96, 80, 3
    p = S.Params(coarsest_scale=3, finest_scale=1, patch_size=8, iterations=12, patch_overlap=0.5,
                 patch_normalization=1)
    rng = np.random.default_rng(5)
    stacks = []
    for role in range(2):
        g = np.stack([S.synth_pair(400 + k, W, H)[role] for k in range(n)])
        col = np.clip(g[..., None].astype(np.int32) + rng.integers(-40, 41, (n, H, W, 3)), 0, 255).astype(np.uint8)
        stacks.append(col)
    dev = [torch.from_numpy(c).cuda() for c in stacks]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    # the reference: an engine that takes the BGR frames themselves
    eng = S.DenseInverseSearch(p, W, H, max_batch=n, frame_format="bgr")
    exp = torch.zeros((n, H, W, 2), dtype=torch.float32, device="cuda")
    eng.calc_device(n, dev[0].data_ptr(), dev[1].data_ptr(), exp.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    eng.close()
    # BGR -> NV12 (601 full) on the device, then the gray engine on the Y planes where they lie
    img = W * H * 3 // 2
    surf = [torch.zeros((n, H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for d, s in zip(dev, surf):
        q = s.data_ptr()
        S.frames_to_yuv420_device(d.data_ptr(), "bgr", n, W, H, q, q + W * H, q + W * H + 1, 2, "bt601", "full",
                                  y_stride=W, y_image_stride=img, c_stride=W, c_image_stride=img,
                                  stream=st.cuda_stream)
    gray = S.DenseInverseSearch(p, W, H, max_batch=n)
    got = torch.zeros((n, H, W, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    luma = [S.nv12_luma(s) for s in surf]
    assert luma[0].data_ptr() == surf[0].data_ptr() and tuple(luma[0].stride()) == (img, W, 1)
    gray.calc_device(n, luma[0].data_ptr(), luma[1].data_ptr(), got.data_ptr(), stream=st.cuda_stream, stride=W,
                     pair_stride=img)
    st.synchronize()
    gray.close()
    for k in range(2):
        _assert_same(luma[k].cpu().numpy(), lumaref.to_gray(stacks[k], "bgr"), "the Y plane is the engine's gray frame")
    _assert_same(got.cpu().numpy(), exp.cpu().numpy(), "flow of the Y planes in place against the bgr engine's")
    assert np.abs(exp.cpu().numpy()).max() > 0.5


# ---------------------------------------------------------------------------
# the C++ facade
# ---------------------------------------------------------------------------
def test_cpp_facade_yuv(tmp_path):
    # tests/cpp/test_yuv.cpp: dis::Yuv420's makers, dis::framesToYuv420 and dis::yuv420ToFrames on host buffers
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "optical-flow-using-dense-inverse-search_amd", "disflow")
    exe = str(tmp_path / "test_yuv")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "test_yuv.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout
