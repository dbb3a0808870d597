"""Video stabilisation on the GPU: dis_warp_motion_u8 bit for bit against
tests/stabref.py (warpref's warp of motionref's field) and against the GPU
chain motion_to_flow + flow_warp, over shapes around the 64 x 16 tile, 1 / 3 / 4
channels, both borders, with and without valid, host and device pointers
(aligned, 1 byte off, padded strides; params in device memory on a caller's
stream), models for every route of the kernel; DenseInverseSearch.stabilize
end to end on tests/stabscene.py's shaky sequence; the facade program and the
CLI."""
import os
import struct
import subprocess

import numpy as np
import pytest

import motionref
import stabref
import stabscene
import warpref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")
CPP = os.path.join(ROOT, "tests", "cpp")
F32 = np.float32


def _assert_same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    bad = g != e
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first at {idx[0].tolist()} "
                             f"got {g[tuple(idx[0])]!r} exp {e[tuple(idx[0])]!r}")


# (W, H, n): a single pixel; a short last lane; exactly one tile; a tile plus
# one each way; odd sizes over several tiles; five tiles a row; many rows; two
# rows (every tile corner lies on row 0 or 1: where "cancelling partial sums"
# stages its blocks and sends pixels of them to global memory)
SHAPES = [(1, 1, 1), (5, 3, 2), (64, 16, 1), (65, 17, 2), (67, 33, 3), (257, 64, 2), (160, 120, 2), (160, 2, 1)]
CHANNELS = [1, 3, 4]
BORDERS = [("replicate", warpref.REPLICATE), ("zero", warpref.ZERO)]


def _about_centre(W, H, deg, scale, tx=0.0, ty=0.0):
    """The model of x -> scale * R(deg) (x - c) + c + t."""
    c, s = scale * np.cos(np.deg2rad(deg)), scale * np.sin(np.deg2rad(deg))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return [cx - (c * cx - s * cy) + tx, c - 1, -s, cy - (s * cx + c * cy) + ty, s, c - 1]


# name -> (W, H) -> six parameters. The non-finite ones sit between finite ones,
# so that a batch holds both.
MODELS = [
    ("identity", lambda W, H: [0, 0, 0, 0, 0, 0]),
    ("integer translation", lambda W, H: [3, 0, 0, -2, 0, 0]),
    ("nan", lambda W, H: [1.5, 0, np.nan, 0, 0, 0]),
    ("sub-pixel translation", lambda W, H: [2.25, 0, 0, -1.5, 0, 0]),
    ("rotation 0.6 scale 1.01", lambda W, H: _about_centre(W, H, 0.6, 1.01, 1.25, -0.75)),  # staged
    ("inf", lambda W, H: [0, 0, 0, -np.inf, 0, 0]),
    ("rotation 30 scale 0.5", lambda W, H: _about_centre(W, H, 30, 0.5)),
    ("rotation 30 scale 4", lambda W, H: _about_centre(W, H, 30, 4.0)),  # boxes beyond the LDS budget: direct
    ("all outside", lambda W, H: [3.0 * W + 7.5, 0, 0, -2.0 * H - 0.5, 0, 0]),
    ("vectors beyond 1e9", lambda W, H: [3e9, 0, 0, 1.0, 0, 0]),
    ("vectors beyond 1e9 from x = 11 on", lambda W, H: [-2.0, 1e8, 0, 0.5, 0, 0.01]),
    ("shear beyond the margin", lambda W, H: [0.3, 0.2, 0.45, -0.2, -0.3, 0.1]),
    # on row 1 p0 + p1*x is rounded to a multiple of 32 before p2*y cancels it: targets inside the frame,
    # tens of pixels outside the box of their tile's corners
    ("cancelling partial sums", lambda W, H: [-5e8, -0.4, 5e8, 0, 0, 0]),
]
_inputs = {}
_expected = {}


def groups(n):
    """The models in batches of n (the last one wraps round)."""
    k = len(MODELS)
    return [[(g * n + i) % k for i in range(n)] for g in range((k + n - 1) // n)]


def images(W, H, n, C):
    key = (W, H, n, C)
    if key not in _inputs:
        rng = np.random.default_rng(100000 * C + 1000 * W + 10 * H + n)
        img = rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)
        img.setflags(write=False)
        _inputs[key] = img
    return _inputs[key]


def params_of(shape, group):
    W, H, n = shape
    return np.array([MODELS[m][1](W, H) for m in group], np.float64).astype(F32)


def expected(shape, C, g, border):
    """The restatement's (dst, valid) of one batch: computed once, never changed."""
    key = (shape, C, g, border)
    if key not in _expected:
        W, H, n = shape
        dst, valid = stabref.warp(images(W, H, n, C), params_of(shape, groups(n)[g]), border)
        dst.setflags(write=False)
        valid.setflags(write=False)
        _expected[key] = (dst, valid)
    return _expected[key]


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_motion_matches_restatement_and_chain_host(disflow_mod, shape, C):
    d = disflow_mod
    W, H, n = shape
    img = images(W, H, n, C)
    for g, group in enumerate(groups(n)):
        p = params_of(shape, group)
        names = ", ".join(MODELS[m][0] for m in group)
        field = d.motion_to_flow(p, W, H)
        for bname, border in BORDERS:
            dst, valid = expected(shape, C, g, border)
            got, gvalid = d.warp_motion(img, p, border=bname, return_valid=True)
            _assert_same(got, dst, f"dst, {bname}: {names}")
            _assert_same(gvalid, valid, f"valid, {bname}: {names}")
            _assert_same(d.warp_motion(img, p, border=bname), dst, f"dst without valid, {bname}: {names}")
            cdst, cvalid = d.flow_warp(img, field, border=bname, with_valid=True)
            _assert_same(got, cdst, f"dst against the GPU chain, {bname}: {names}")
            _assert_same(gvalid, cvalid, f"valid against the GPU chain, {bname}: {names}")
        for k, m in enumerate(group):
            name = MODELS[m][0]
            dst, valid = expected(shape, C, g, warpref.REPLICATE)
            if name == "identity":
                _assert_same(dst[k], img[k], "the identity returns the source")
                assert (valid[k] == 255).all()
            if name in ("nan", "inf", "vectors beyond 1e9", "all outside"):
                assert not valid[k].any()
            if name in ("nan", "inf", "vectors beyond 1e9"):
                assert not dst[k].any()
    if C == 1:  # the other layouts of the Python entry
        p = params_of(shape, groups(n)[0])
        dst, valid = expected(shape, C, 0, warpref.REPLICATE)
        _assert_same(d.warp_motion(img[..., 0], p), dst[..., 0], "(n, H, W) images")
        _assert_same(d.warp_motion(img[0, ..., 0], p[0]), dst[0, ..., 0], "one (H, W) image")
        one, v1 = d.warp_motion(img[0], p[0], return_valid=True)
        _assert_same(one, dst[0], "one (H, W, C) image")
        _assert_same(v1, valid[0], "its (H, W) valid map")


def _offset_tensor(torch, host, lead, fill=7):
    """`host` (a flat numpy array) on the device, `lead` elements into a fresh
    allocation (allocations are at least 256-byte aligned)."""
    t = torch.full((lead + host.size,), fill, dtype=torch.from_numpy(host[:1].copy()).dtype, device="cuda:0")[lead:]
    t.copy_(torch.from_numpy(host.copy()))
    return t


@pytest.mark.parametrize("layout", ["aligned", "offset", "padded", "padded4"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_motion_matches_restatement_device(disflow_mod, shape, layout):
    # device pointers (torch tensors) and device params on a caller's stream.
    # aligned: every vector form the shape allows; offset: image, dst and valid 1
    # byte in, so no vector form applies; padded: rows and images of the source
    # further apart than they are long, by odd amounts; padded4: by multiples of
    # 4, so the padded rows still take the dword forms
    import torch
    W, H, n = shape
    lead = 1 if layout == "offset" else 0
    s = torch.cuda.Stream()
    for C in CHANNELS:
        img = images(W, H, n, C)
        stride, image_stride = W * C, W * C * H
        src_host = img.reshape(-1)
        if layout.startswith("padded"):
            stride = W * C + 5 if layout == "padded" else (W * C + 3) // 4 * 4 + 8
            image_stride = stride * H + (7 if layout == "padded" else 12)
            rng = np.random.default_rng(5)
            src_host = rng.integers(0, 256, n * image_stride, dtype=np.uint8)  # the padding holds other bytes
            for k in range(n):
                rows = src_host[k * image_stride:k * image_stride + H * stride].reshape(H, stride)
                rows[:, :W * C] = img[k].reshape(H, W * C)
            src_host = src_host[:(n - 1) * image_stride + (H - 1) * stride + W * C]  # the source ends with its last sample
        tsrc = _offset_tensor(torch, src_host, lead)
        px = n * H * W
        for g, group in enumerate(groups(n)):
            tpar = torch.from_numpy(params_of(shape, group)).to("cuda:0")
            for (bname, border), with_valid in zip(BORDERS, (True, False) if g % 2 == 0 else (False, True)):
                tdst = torch.full((lead + px * C,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
                tvalid = torch.full((lead + px,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
                torch.cuda.synchronize()
                disflow_mod.warp_motion_device(tsrc.data_ptr(), tpar.data_ptr(), n, W, H, C, tdst.data_ptr(),
                                               tvalid.data_ptr() if with_valid else 0, border=bname,
                                               src_stride=stride if layout.startswith("padded") else 0,
                                               src_image_stride=image_stride if layout.startswith("padded") else 0,
                                               stream=s.cuda_stream)
                s.synchronize()
                dst, valid = expected(shape, C, g, border)
                what = f"{C} channels, {bname}, group {g}"
                _assert_same(tdst.cpu().numpy().reshape(n, H, W, C), dst, "dst, " + what)
                if with_valid:
                    _assert_same(tvalid.cpu().numpy().reshape(n, H, W), valid, "valid, " + what)
                else:
                    assert bool((tvalid == 9).all()), "valid written though not asked for"


def test_warp_motion_rejects_misaligned_device_params(disflow_mod):
    import torch
    p = torch.zeros(16, dtype=torch.float32, device="cuda:0")
    b = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    o = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(disflow_mod.DisError):
        disflow_mod.warp_motion_device(b.data_ptr(), p.data_ptr() + 2, 1, 8, 8, 1, o.data_ptr())
    disflow_mod.warp_motion_device(b.data_ptr(), p.data_ptr() + 4, 1, 8, 8, 1, o.data_ptr())
    torch.cuda.synchronize()


ROUTE_CASES = [  # (model, (W, H), channels)
    ("rotation 0.6 scale 1.01", (160, 120), 3), ("rotation 30 scale 4", (160, 120), 3), ("nan", (160, 120), 3),
    ("vectors beyond 1e9 from x = 11 on", (160, 120), 3), ("cancelling partial sums", (160, 2), 3),
    ("cancelling partial sums", (160, 120), 3), ("all outside", (257, 64), 3), ("identity", (67, 33), 3),
    ("rotation 0.6 scale 1.01", (160, 120), 1), ("cancelling partial sums", (160, 2), 4),
]


def _kernel_routes(p, W, H, C, border):
    """The route counters of the kernel itself: tools/stabilize_ab's route mode
    (built by build(); it includes the kernel's source and launches the library's
    choice of kernel with its counters)."""
    exe = os.path.join(ROOT, "tools", "stabilize_ab")
    assert os.path.exists(exe), "tools/stabilize_ab is not built: run __graft_entry__.build()"
    r = subprocess.run([exe, "routes", str(W), str(H), str(C), str(border)] + ["%.9g" % v for v in p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "routes" and len(words) == 4, r.stdout
    return tuple(int(w) for w in words[1:])


def test_every_route_is_taken_by_the_kernel():
    """The kernel's own route counters -- blocks that stage their box, blocks
    that run the direct form, pixels of staged blocks that read global memory --
    equal tests/stabref.py's restatement of its decision, case by case, and
    every route is taken. Only 3 channels stage. There the small rotation stages
    every block; the fourfold rotation sends blocks whose box lies inside the
    frame to the direct form; a model that is not finite or whose corner vectors
    are not valid runs direct everywhere; and "cancelling partial sums" on two
    rows stages all three blocks and sends 31 of their pixels to global memory
    under either border (their targets lie inside the frame)."""
    seen = np.zeros(3, np.int64)
    for name, (W, H), C in ROUTE_CASES:
        p = np.array(dict(MODELS)[name](W, H), np.float64).astype(F32)
        for _, border in BORDERS:
            exp = stabref.routes(p, W, H, C, border)
            got = _kernel_routes(p, W, H, C, border)
            assert got == exp, f"{name}, {W} x {H}, {C} channels, border {border}: kernel {got}, restated {exp}"
            seen += got
    by = {name: f for name, f in MODELS}
    q = np.array(by["cancelling partial sums"](160, 2), np.float64).astype(F32)
    assert stabref.routes(q, 160, 2, 3) == stabref.routes(q, 160, 2, 3, warpref.ZERO) == (3, 0, 31)
    assert stabref.routes(np.array(by["rotation 0.6 scale 1.01"](160, 120)).astype(F32), 160, 120, 3) == (24, 0, 0)
    st, di, la = stabref.routes(np.array(by["rotation 30 scale 4"](160, 120)).astype(F32), 160, 120, 3)
    assert st >= 1 and di >= 1 and st + di == 24
    assert stabref.routes(q, 160, 2, 1) == stabref.routes(q, 160, 2, 4) == (0, 3, 0)
    assert (seen > 0).all()
    # and the bit-for-bit cases above hold all three
    total = np.zeros(3, np.int64)
    for shp in SHAPES:
        for group in groups(shp[2]):
            for _, border in BORDERS:
                total += stabref.routes(params_of(shp, group), shp[0], shp[1], 3, border)
    print(f"routes over the 3-channel cases: {total[0]} staged blocks, {total[1]} direct blocks, "
          f"{total[2]} pixels of staged blocks read global memory")
    assert (total > 0).all()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _engine(disflow_mod, frame_format="gray", max_batch=4):
    C, F, ps, it, ov = stabscene.ENGINE
    return disflow_mod.DenseInverseSearch(disflow_mod.Params(C, F, ps, it, ov, 1), stabscene.W, stabscene.H,
                                          max_batch=max_batch, frame_format=frame_format)


@pytest.mark.parametrize("frame_format", ["gray", "bgr"])
def test_stabilize_is_the_restated_chain_on_the_engines_flows(disflow_mod, frame_format):
    fr = stabscene.frames()
    if frame_format == "bgr":
        fr = np.stack([fr, 255 - fr, fr // 2 + 40], axis=-1)
    N, W, H = stabscene.N, stabscene.W, stabscene.H
    eng = _engine(disflow_mod, frame_format)
    flows = np.concatenate([eng.calc_batch(fr[k:min(k + 4, N - 1)], fr[k + 1:min(k + 4, N - 1) + 1])
                            for k in range(0, N - 1, 4)])
    out, pair, corr = eng.stabilize(fr, radius=3, zoom=1.05, return_models=True)
    plain = eng.stabilize(fr, model="affine", radius=5, sigma=2.5, border="zero")
    eng.close()
    epair = np.stack([motionref.fit_one(f, None, motionref.SIMILARITY, 3, 1.0)[0] for f in flows])
    _assert_same(pair.view(np.uint32), epair.view(np.uint32), "the pair models")
    ecorr, est, erep = stabref.stabilize(epair, W, H, 3, 1.5, 1.05)
    assert est.all() and erep == 0
    _assert_same(corr.view(np.uint32), ecorr.view(np.uint32), "the corrections")
    _assert_same(out, stabref.warp(fr, ecorr)[0], "the stabilised frames")
    apair = np.stack([motionref.fit_one(f, None, motionref.AFFINE, 3, 1.0)[0] for f in flows])
    _assert_same(plain, stabref.warp(fr, stabref.stabilize(apair, W, H, 5, 2.5, 1.0)[0], warpref.ZERO)[0],
                 "affine models, zero border")
    if frame_format == "gray":
        A = stabscene.true_pair_matrices()
        raw, steady = stabscene.roughness(A), stabscene.roughness(A, stabref.stabilize(epair, W, H, 3, 1.5, 1.0)[0])
        print(f"centre track, RMS second difference: raw {raw:.3f} px, stabilised {steady:.3f} px")
        assert steady < raw / 4


def test_stabilize_of_one_frame_and_bad_arguments(disflow_mod):
    fr = stabscene.frames()
    eng = _engine(disflow_mod)
    _assert_same(eng.stabilize(fr[:1]), fr[:1], "one frame comes back as it is")
    two, pair, corr = eng.stabilize(fr[:2], radius=0, zoom=2.0, return_models=True)
    z = stabref.stabilize(pair, stabscene.W, stabscene.H, 0, 0.5, 2.0)[0]
    _assert_same(corr.view(np.uint32), z.view(np.uint32), "radius 0: the corrections")
    assert np.abs(z - np.array([79.5 / 2, -0.5, 0, 59.5 / 2, 0, -0.5])).max() < 1e-4  # the zoom alone
    _assert_same(two, stabref.warp(fr[:2], z)[0], "radius 0: the frames")
    for kw in (dict(model="projective"), dict(radius=-1), dict(zoom=0.5), dict(sigma=0.0), dict(border="mirror"),
               dict(iterations=17), dict(threshold=-1.0)):
        with pytest.raises(ValueError):
            eng.stabilize(fr, **kw)
    with pytest.raises(disflow_mod.DisError):
        eng.stabilize(fr[:, :50])
    eng.close()


def test_cpp_facade_stabilize(tmp_path):
    # tests/cpp/test_stabilize.cpp: dis::stabilizePath and dis::warpMotion on four BGR frames of 67 x 33
    W, H, C, n, radius, zoom = 67, 33, 3, 4, 2, 1.25
    img = images(W, H, n, C)
    pair = np.array([_about_centre(W, H, 0.5, 1.01, 2.0, -1.0), [1.5, 0, 0, -0.5, 0, 0],
                     _about_centre(W, H, -0.7, 0.99, -3.0, 2.0)], np.float64).astype(F32)
    img.tofile(str(tmp_path / "frames.u8"))
    pair.tofile(str(tmp_path / "pair.f32"))
    exe = str(tmp_path / "test_stabilize")
    r = subprocess.run(["make", "-s", "-C", CPP, "-f", "stabilize.mk", "test_stabilize", f"STAB_OUT={exe}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(tmp_path), str(W), str(H), str(C), str(n), str(radius), str(zoom)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout
    got = {line.split()[1]: line.split()[2:] for line in r.stdout.splitlines() if line.startswith("bits ")}

    def words(a):
        return [f"{int(v):08x}" for v in np.ascontiguousarray(a).view(np.uint32).reshape(-1)]
    assert got["plain"] == words(stabref.stabilize(pair, W, H, radius, 1.0, 1.0)[0])
    corr = stabref.stabilize(pair, W, H, radius, 1.0, zoom)[0]
    assert got["zoomed"] == words(corr)
    dst, valid = stabref.warp(img, corr)
    _assert_same(np.fromfile(str(tmp_path / "stab.u8"), np.uint8).reshape(dst.shape), dst, "dst")
    _assert_same(np.fromfile(str(tmp_path / "valid.u8"), np.uint8).reshape(valid.shape), valid, "valid")
    _assert_same(np.fromfile(str(tmp_path / "zero.u8"), np.uint8).reshape(dst.shape),
                 stabref.warp(img, corr, warpref.ZERO)[0], "dst, zero border")


def _read_png(path, tmp_path, kind):
    png_tool = os.path.join(CPP, "png_tool")
    subprocess.check_call(["make", "-s", "-C", CPP, "png_tool"])
    raw_path = str(tmp_path / "png.raw")
    subprocess.run([png_tool, kind, path, raw_path], check=True)
    raw = open(raw_path, "rb").read()
    w, h = struct.unpack("<ii", raw[:8])
    return np.frombuffer(raw[8:], np.uint8).reshape(h, w)


def test_cli_stabilize_writes_the_frames(disflow_mod, tmp_path):
    import pngio
    cli = os.path.join(PKG, "disflow", "dis_flow")
    T = 6
    fr = stabscene.frames()[:T]
    d = tmp_path / "seq"
    d.mkdir()
    for k, f in enumerate(fr):
        pngio.write_gray8(str(d / f"frame_{k + 1:04d}.png"), f)
    args = [cli, "seq", "1", str(T), "12", "8", "3", "1", "0.5", "1", "0", "--batch", "4", "--flo", "--stabilize", "2",
            "--stab-zoom", "1.1"]
    r = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    flows = np.stack([disflow_mod.read_flo(str(tmp_path / f"OF_seq/frame_{k + 1:04d}.flo")) for k in range(T - 1)])
    pair = np.stack([motionref.fit_one(f, None, motionref.SIMILARITY, 3, 1.0)[0] for f in flows])  # similarity without --motion
    corr = stabref.stabilize(pair, stabscene.W, stabscene.H, 2, 1.0, 1.1)[0]
    lines = open(str(tmp_path / "OF_seq/stab_corrections.txt")).read().splitlines()
    assert lines == [" ".join("%.9g" % v for v in q) for q in corr]
    exp = stabref.warp(fr, corr)[0]
    for t in range(T):
        got = _read_png(str(tmp_path / f"OF_seq/frame_{t + 1:04d}_stab.png"), tmp_path, "gray")
        _assert_same(got, exp[t], f"frame {t + 1}")
        assert f"stabilised seq/frame_{t + 1:04d}.png" in r.stdout
    assert not os.path.exists(str(tmp_path / "OF_seq/frame_0001_motion.txt"))  # the models are written with --motion only
    for bad in (["--stabilize", "-1"], ["--stabilize", "2", "--stab-zoom", "0.5"], ["--stabilize", "1025"]):
        r = subprocess.run(args[:11] + bad, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert r.returncode == 2 and "--stabilize" in r.stderr
