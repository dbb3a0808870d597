"""GPU tests of motion-compensated temporal denoising (dis_temporal_denoise_u8):
the kernel against its numpy restatement (tests/denoiseref.py) on host arrays
and on device pointers (aligned; offset by a byte with padded strides and flows
that are only pair-aligned), with every mask form, flows that hold invalid,
outward and half-pixel vectors, the engine's denoise() end to end, the C++
facade and the CLI's --denoise. Every comparison is bit for bit."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import denoiseref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")

F32, F16 = np.float32, np.float16

# (W, H, n, K): one pixel; a frame smaller than the window; odd sides, two images
# and neighbours; more than one tile in x and y with partial ones; eight neighbours
# and several full tiles; one pixel more than two 64 x 16 tiles in each dimension
SHAPES = [(1, 1, 1, 1), (2, 2, 1, 1), (5, 3, 2, 2), (67, 33, 3, 2), (160, 120, 1, 8), (129, 33, 2, 3)]
CHANNELS = (1, 3, 4)
MASKS = ("none", "some", "all")
TABLE = denoiseref.weights(12.0)
TABLE.setflags(write=False)
_inputs = {}
_expected = {}


def _ids(s):
    return "x".join(map(str, s))


def _assert_same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype == np.uint8, f"{what}: {g.shape} {g.dtype} against {e.shape} {e.dtype}"
    bad = g != e
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first at {idx[0].tolist()} "
                             f"got {g[tuple(idx[0])]} exp {e[tuple(idx[0])]}")


def inputs(W, H, n, K, C):
    """cur: value noise plus pixel noise; neighbour k: cur moved by a whole-pixel
    shift with fresh noise, a patch of it replaced by other content; flow k: the
    shift back with jitter quantised to quarter pixels (so exact half-pixel
    targets occur) on half the pixels and free jitter on the rest, vectors that
    lead outside the frame along the borders, and a handful of NaN, +-1e9, 2e9 and
    +-inf vectors; as float32 and narrowed to float16; masks with 25 % zeros. Made
    once, never changed."""
    key = (W, H, n, K, C)
    if key not in _inputs:
        rng = np.random.default_rng(100000 * C + 1000 * W + 10 * H + K)
        m = 8
        big = rng.normal(0, 1, (n, H + 2 * m, W + 2 * m, C))
        for _ in range(3):  # a cheap low-pass: structure a flow can follow
            big = (big + np.roll(big, 1, 1) + np.roll(big, 1, 2) + np.roll(big, -1, 1) + np.roll(big, -1, 2)) / 5
        big = 128 + 400 * big
        cur = np.clip(np.round(big[:, m:m + H, m:m + W] + rng.normal(0, 6, (n, H, W, C))), 0, 255).astype(np.uint8)
        nbs, flows32, flows16, masks = [], [], [], []
        for k in range(K):
            dx, dy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
            nb = big[:, m - dy:m - dy + H, m - dx:m - dx + W] + rng.normal(0, 6, (n, H, W, C))
            nb[:, H // 3:H // 3 + max(H // 4, 1), W // 2:W // 2 + max(W // 4, 1)] = rng.uniform(0, 255, (1, 1, 1, C))
            nbs.append(np.clip(np.round(nb), 0, 255).astype(np.uint8))
            fl = np.empty((n, H, W, 2))
            fl[..., 0], fl[..., 1] = -dx, -dy
            quant = rng.random((n, H, W)) < 0.5
            jit = rng.uniform(-1.5, 1.5, fl.shape)
            fl += np.where(quant[..., None], np.round(jit * 4) / 4, jit)
            edge = np.zeros((n, H, W), bool)
            edge[:, 0], edge[:, -1], edge[:, :, 0], edge[:, :, -1] = True, True, True, True
            fl[edge & (rng.random((n, H, W)) < 0.5)] *= 4
            fl = fl.astype(F32)
            bad = [(np.nan, np.nan), (1e9, -1e9), (-1e9, 2.0), (np.inf, 0.5), (1.0, -np.inf), (0.0, np.nan), (2e9, 0.0),
                   (0.5, 0.5), (-0.5, 1.5)]
            flat = fl.reshape(-1, 2)
            for j, q in enumerate(rng.choice(flat.shape[0], size=min(len(bad), max(flat.shape[0] // 8, 1)), replace=False)):
                flat[q] = bad[j]
            with np.errstate(over="ignore"):
                fl16 = fl.astype(F16)  # (+-1e9 become +-inf: still invalid)
            flows32.append(fl)
            flows16.append(fl16)
            masks.append(np.where(rng.random((n, H, W)) < 0.25, 0, rng.integers(1, 256, (n, H, W))).astype(np.uint8))
        for arr in [cur] + nbs + flows32 + flows16 + masks:
            arr.setflags(write=False)
        _inputs[key] = dict(cur=cur, nbs=nbs, flows={np.dtype(F32): flows32, np.dtype(F16): flows16}, masks=masks)
    return _inputs[key]


def mask_list(inp, mode):
    """none: no masks at all; some: a mask for every odd neighbour; all: one for each."""
    if mode == "none":
        return None
    return [m if (mode == "all" or k % 2) else None for k, m in enumerate(inp["masks"])]


def expected(shape, C, dtype, mode, table=TABLE):
    """The restatement's (dst, support) of one case: computed once."""
    key = (shape, C, np.dtype(dtype), mode, table.tobytes())
    if key not in _expected:
        inp = inputs(*shape, C)
        r = denoiseref.denoise(inp["cur"], inp["nbs"], inp["flows"][np.dtype(dtype)], table, mask_list(inp, mode))
        for a in r:
            a.setflags(write=False)
        _expected[key] = r
    return _expected[key]


CASES = list(itertools.product(CHANNELS, (F32, F16), MASKS))


# ---------------------------------------------------------------------------
# host arrays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_matches_restatement_host(disflow_mod, shape):
    W, H, n, K = shape
    for C, dtype, mode in CASES:
        inp = inputs(*shape, C)
        what = f"{C} channels, {np.dtype(dtype).name}, masks {mode}"
        dst, sup = expected(shape, C, dtype, mode)
        got = disflow_mod.temporal_denoise(inp["cur"], inp["nbs"], inp["flows"][np.dtype(dtype)], weights=TABLE,
                                           masks=mask_list(inp, mode), return_support=True)
        _assert_same(got[0], dst, "dst, " + what)
        _assert_same(got[1], sup, "support, " + what)
    inp = inputs(*shape, 3)
    dst, sup = expected(shape, 3, F32, "all")
    alone = disflow_mod.temporal_denoise(inp["cur"], inp["nbs"], inp["flows"][np.dtype(F32)], weights=TABLE,
                                         masks=inp["masks"])
    _assert_same(alone, dst, "dst without support")
    # one image of a stack: the wrapper's (H, W, C) form
    one = disflow_mod.temporal_denoise(inp["cur"][0], [a[0] for a in inp["nbs"]],
                                       [f[0] for f in inp["flows"][np.dtype(F32)]], weights=TABLE,
                                       masks=[m[0] for m in inp["masks"]], return_support=True)
    assert one[0].shape == (H, W, 3) and one[1].shape == (H, W)
    _assert_same(one[0], dst[0], "one (H, W, C) image")
    _assert_same(one[1], sup[0], "its support")
    # sigma = 12 gives the same table
    _assert_same(disflow_mod.temporal_denoise(inp["cur"], inp["nbs"], inp["flows"][np.dtype(F32)], sigma=12.0,
                                              masks=inp["masks"]), dst, "sigma instead of weights")
    if W * H >= 1000:  # a kernel that ignores an argument cannot pass
        a, b, c = (expected(shape, 1, F32, mode) for mode in MASKS)
        assert (a[1] == K).mean() > 0.5 and (a[1] < K).any() and a[1].max() == K
        assert (c[1] <= b[1]).all() and (b[1] <= a[1]).all() and (c[1] < b[1]).any() and (b[1] < a[1]).any()
        assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], inputs(*shape, 1)["cur"])
        assert not np.array_equal(expected(shape, 1, F32, "none")[0], expected(shape, 1, F16, "none")[0])


@pytest.mark.parametrize("C", CHANNELS)
def test_weights_all_zero_give_cur(disflow_mod, C):
    shape = (67, 33, 3, 2)
    inp = inputs(*shape, C)
    dst, sup = disflow_mod.temporal_denoise(inp["cur"], inp["nbs"], inp["flows"][np.dtype(F32)],
                                            weights=np.zeros(256, F32), return_support=True)
    _assert_same(dst, inp["cur"], "dst")
    assert not sup.any()
    # and a table that is 1 everywhere still agrees with the restatement
    ones = np.ones(256, F32)
    dst = disflow_mod.temporal_denoise(inp["cur"], inp["nbs"], inp["flows"][np.dtype(F16)], weights=ones)
    _assert_same(dst, expected(shape, C, F16, "none", ones)[0], "weights all 1")


# ---------------------------------------------------------------------------
# device pointers
# ---------------------------------------------------------------------------
def _device_bytes(torch, host, lead, fill=0xAB):
    """`host` (a flat u8 numpy array) on the device, `lead` bytes into a fresh
    allocation (allocations are at least 256-byte aligned)."""
    t = torch.full((lead + host.size,), fill, dtype=torch.uint8, device="cuda:0")[lead:]
    t.copy_(torch.from_numpy(np.array(host, copy=True)))
    return t


def _strided(stack, stride, image_stride):
    """(n, H, W, C) u8 -> the flat bytes of the stack with padded rows and images (0xCD in the padding)."""
    n, H, W, C = stack.shape
    out = np.full((n - 1) * image_stride + (H - 1) * stride + W * C, 0xCD, np.uint8)
    for i in range(n):
        for y in range(H):
            o = i * image_stride + y * stride
            out[o:o + W * C] = stack[i, y].reshape(-1)
    return out


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_matches_restatement_device(disflow_mod, shape, layout):
    # device pointers (torch tensors) on a caller's stream. offset: every image
    # stack one byte in with rows padded by 3 and images by 5 bytes, the flows one
    # (u,v) pair in (pair-aligned, not 16-byte aligned), masks, dst and support one
    # byte in
    import torch
    W, H, n, K = shape
    lead = 1 if layout == "offset" else 0
    px = n * H * W
    s = torch.cuda.Stream()
    for C in CHANNELS:
        inp = inputs(*shape, C)
        stride = W * C + (3 if lead else 0)
        image_stride = stride * H + (5 if lead else 0)
        imgs = [_device_bytes(torch, _strided(a.reshape(n, H, W, C), stride, image_stride), lead)
                for a in [inp["cur"]] + inp["nbs"]]
        tmasks = [_device_bytes(torch, m.reshape(-1), lead) for m in inp["masks"]]
        for dtype in (F32, F16):
            df = np.dtype(dtype)
            tfl = [_device_bytes(torch, f.reshape(-1).view(np.uint8), lead * 2 * df.itemsize, fill=0)
                   for f in inp["flows"][df]]
            for t in tfl:
                assert t.data_ptr() % 16 == lead * 2 * df.itemsize
            for mode, with_support in itertools.product(MASKS, (True, False)):
                tdst = torch.full((lead + px * C + 1,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
                tsup = torch.full((lead + px + 1,), 9, dtype=torch.uint8, device="cuda:0")[lead:]
                ml = mask_list(inp, mode)
                mask_ptrs = None if ml is None else [0 if m is None else tmasks[k].data_ptr() for k, m in enumerate(ml)]
                torch.cuda.synchronize()
                disflow_mod.temporal_denoise_device(
                    imgs[0].data_ptr(), [t.data_ptr() for t in imgs[1:]], [t.data_ptr() for t in tfl], df, n, W, H, C,
                    tdst.data_ptr(), weights=TABLE, mask_ptrs=mask_ptrs, support_ptr=tsup.data_ptr() if with_support else 0,
                    stride=stride if lead else 0, image_stride=image_stride if lead else 0, stream=s.cuda_stream)
                s.synchronize()
                dst, sup = expected(shape, C, dtype, mode)
                what = f"{C} channels, {df.name}, masks {mode}"
                _assert_same(tdst[:px * C].cpu().numpy().reshape(dst.shape), dst, "dst, " + what)
                assert int(tdst[px * C]) == 9, "a byte after dst written"
                if with_support:
                    _assert_same(tsup[:px].cpu().numpy().reshape(sup.shape), sup, "support, " + what)
                    assert int(tsup[px]) == 9, "a byte after support written"
                else:
                    assert bool((tsup == 9).all()), "support written though not asked for"
            for t, f in zip(tfl, inp["flows"][df]):
                assert np.array_equal(t.cpu().numpy(), f.reshape(-1).view(np.uint8)), "a flow changed"
        for t, a in zip(imgs, [inp["cur"]] + inp["nbs"]):
            assert np.array_equal(t.cpu().numpy(), _strided(a.reshape(n, H, W, C), stride, image_stride)), "an image changed"


def test_rejects_bad_device_pointers(disflow_mod):
    import torch
    t = [torch.zeros(256, dtype=torch.uint8, device="cuda:0") for _ in range(5)]
    cur, nb, fl, dst, sup = (x.data_ptr() for x in t)
    # (flow, dtype, dst, support)
    for fp, fd, dp, sp in ((fl + 4, F32, dst, 0), (fl + 2, F16, dst, 0), (fl, F32, cur, 0), (fl, F32, dst, dst + 3),
                           (fl, F32, nb + 3, 0), (fl, F32, dst, fl + 31)):
        with pytest.raises(disflow_mod.DisError) as e:
            disflow_mod.temporal_denoise_device(cur, [nb], [fp], fd, 1, 2, 2, 1, dp, weights=TABLE, support_ptr=sp)
        assert e.value.status == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    disflow_mod.temporal_denoise_device(cur, [nb], [fl], F32, 1, 2, 2, 1, dst, weights=TABLE, support_ptr=sup)
    torch.cuda.synchronize()
    assert bool((t[3][:4] == 0).all()) and bool((t[4][:4] == 1).all())


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
EW, EH = 64, 48


def _sequence(C, seed=5):
    """Three noisy EW x EH frames of one moving texture, (3, EH, EW) or (3, EH, EW, C)."""
    rng = np.random.default_rng(seed)
    m = 8
    big = rng.normal(0, 1, (EH + 2 * m, EW + 2 * m, C))
    for _ in range(4):
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, -1, 0) + np.roll(big, -1, 1)) / 5
    big = 128 + 500 * big
    fr = [big[m - t:m - t + EH, m + 2 * t:m + 2 * t + EW] + rng.normal(0, 8, (EH, EW, C)) for t in (-1, 0, 1)]
    fr = np.clip(np.round(np.stack(fr)), 0, 255).astype(np.uint8)
    return fr[..., 0] if C == 1 else fr


@pytest.mark.parametrize("fmt,C", [("gray", 1), ("bgr", 3)])
def test_engine_denoise_equals_the_restatement_on_its_own_flows(disflow_mod, fmt, C):
    fr = _sequence(C)
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Params(2, 1, 8, 12, 0.5, 1), EW, EH, max_batch=4, frame_format=fmt)
    got = eng.denoise(fr, radius=1, sigma=12.0)
    pairs = [(0, 1), (1, 0), (1, 2), (2, 1)]  # what denoise() asks of the engine, in one call of max_batch pairs
    flows = eng.calc_batch(fr[[t for t, _ in pairs]], fr[[j for _, j in pairs]])
    eng.close()
    assert got.shape == fr.shape and got.dtype == np.uint8
    for t in range(3):
        mine = [i for i, (a, _) in enumerate(pairs) if a == t]
        exp, _ = denoiseref.denoise(fr[t], [fr[pairs[i][1]] for i in mine], [flows[i] for i in mine], TABLE)
        _assert_same(got[t], exp, f"{fmt} frame {t}")
    assert not np.array_equal(got, fr)
    # a radius past the sequence's ends uses the frames that exist
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Params(2, 1, 8, 12, 0.5, 1), EW, EH, max_batch=2, frame_format=fmt)
    wide = eng.denoise(fr, radius=2, weights=TABLE)
    f01 = eng.calc_batch(fr[[0, 0]], fr[[1, 2]])
    eng.close()
    exp, _ = denoiseref.denoise(fr[0], [fr[1], fr[2]], list(f01), TABLE)
    _assert_same(wide[0], exp, f"{fmt} frame 0 at radius 2")


# ---------------------------------------------------------------------------
# the facade and the CLI
# ---------------------------------------------------------------------------
def test_cpp_facade_denoise(disflow_mod, tmp_path):
    # tests/cpp/test_denoise.cpp: dis::temporalDenoise in its f32 and half_bits forms
    # and dis::denoiseWeights on the (67, 33, 3, 2) case with 3 channels
    shape, C = (67, 33, 3, 2), 3
    W, H, n, K = shape
    inp = inputs(*shape, C)
    files = {"cur.u8": inp["cur"], "nb0.u8": inp["nbs"][0], "nb1.u8": inp["nbs"][1], "mask1.u8": inp["masks"][1]}
    for k in range(2):
        files[f"flow{k}.f32"] = inp["flows"][np.dtype(F32)][k]
        files[f"flow{k}.f16"] = inp["flows"][np.dtype(F16)][k]
    for name, arr in files.items():
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
    exe = str(tmp_path / "test_denoise")
    lib_dir = os.path.join(PKG, "disflow")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_denoise.cpp"), "-o", exe,
                           "-L" + lib_dir, "-ldis_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path), str(W), str(H), str(n), str(C)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK: 0 failure(s)" in r.stdout
    table = np.fromfile(str(tmp_path / "table.f32"), F32)
    assert np.array_equal(table.view(np.uint32), disflow_mod.denoise_weights(12.0).view(np.uint32))
    dst, sup = expected(shape, C, F32, "some", table)  # "some": a mask for neighbour 1 only
    _assert_same(np.fromfile(str(tmp_path / "dst_f32.u8"), np.uint8).reshape(dst.shape), dst, "dst, f32")
    _assert_same(np.fromfile(str(tmp_path / "support_f32.u8"), np.uint8).reshape(sup.shape), sup, "support, f32")
    dst16, _ = expected(shape, C, F16, "none", table)
    _assert_same(np.fromfile(str(tmp_path / "dst_f16.u8"), np.uint8).reshape(dst16.shape), dst16, "dst, half_bits")


def _read_png(path, tmp_path, kind):
    png_tool = os.path.join(ROOT, "tests", "cpp", "png_tool")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "png_tool"])
    raw_path = str(tmp_path / "png.raw")
    subprocess.run([png_tool, kind, path, raw_path], check=True)
    raw = open(raw_path, "rb").read()
    w, h = struct.unpack("<ii", raw[:8])
    return np.frombuffer(raw[8:], np.uint8).reshape(h, w)


def test_cli_denoise_writes_the_frames(disflow_mod, tmp_path):
    import pngio
    cli = os.path.join(PKG, "disflow", "dis_flow")
    fr = _sequence(1, seed=6)
    d = tmp_path / "seq"
    d.mkdir()
    for k, f in enumerate(fr):
        pngio.write_gray8(str(d / f"frame_{k + 1:04d}.png"), f)
    args = [cli, "seq", "1", "3", "12", "8", "2", "1", "0.5", "1", "0", "--batch", "2", "--denoise", "1", "12"]
    r = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    eng = disflow_mod.DenseInverseSearch(disflow_mod.Params(2, 1, 8, 12, 0.5, 1), EW, EH, max_batch=2)
    for t, js in enumerate(([1], [0, 2], [1])):
        flows = eng.calc_batch(fr[[t] * len(js)], fr[js])
        exp, _ = denoiseref.denoise(fr[t], [fr[j] for j in js], list(flows), TABLE)
        got = _read_png(str(tmp_path / f"OF_seq/frame_{t + 1:04d}_denoised.png"), tmp_path, "gray")
        _assert_same(got, exp, f"frame {t + 1}")
        assert f"denoised seq/frame_{t + 1:04d}.png from {len(js)} frames" in r.stdout
    eng.close()
    assert not os.path.exists(str(tmp_path / "OF_seq/frame_0004_denoised.png"))
