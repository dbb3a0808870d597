"""CPU tests of the warm start's host side: the NumPy restatement of the init
plane (tests/initref.py) against a per-pixel loop, the Python-side shape and
kind checks (they raise before any library call), and the C-ABI's buffer
aliasing and other pure argument rules (csrc/dis_args.h) as a stand-alone
program under the host sanitizers; beside it, the geometry and the kernel
argument builders (csrc/dis_launch_args.hip) the same way."""
import os
import subprocess

import numpy as np
import pytest

import initref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")
f32 = np.float32


def _loop_reference(flow, C):
    """flow_to_init written out per pixel, level by level."""
    H, W = flow.shape[:2]
    Wp, Hp, pl, pt = initref.padded_size(W, H, C)
    P = np.zeros((Hp, Wp, 2), f32)
    for y in range(Hp):
        for x in range(Wp):
            for k in range(2):
                c = flow[min(max(y - pt, 0), H - 1), min(max(x - pl, 0), W - 1), k]
                P[y, x, k] = c if (np.isfinite(c) and abs(c) < 1e9) else f32(0)
    for _ in range(C + 1):
        h, w = P.shape[:2]
        Q = np.zeros(((h + 1) // 2, (w + 1) // 2, 2), f32)
        for y in range(Q.shape[0]):
            for x in range(Q.shape[1]):
                x1, y1 = min(2 * x + 1, w - 1), min(2 * y + 1, h - 1)
                for k in range(2):
                    a, b, c, d = P[2 * y, 2 * x, k], P[2 * y, x1, k], P[y1, 2 * x, k], P[y1, x1, k]
                    Q[y, x, k] = f32(f32(f32(a + b) + f32(c + d)) * f32(0.125))
        P = Q
    return P


@pytest.mark.parametrize("C", [0, 1, 2])
def test_initref_matches_per_pixel_loop(C):
    rng = np.random.default_rng(5 + C)
    flow = rng.uniform(-300, 300, (6, 10, 2)).astype(f32)  # 10 x 6: padded and odd at every C here
    flow[1, 2, 0] = np.nan
    flow[3, 7, 1] = np.inf
    flow[5, 9, 0] = -np.inf
    flow[0, 0, 1] = 1e9
    flow[4, 4, 0] = -1e9
    flow[2, 5, 1] = np.nextafter(f32(1e9), f32(0))  # the largest value kept
    got = initref.flow_to_init(flow, C)
    exp = _loop_reference(flow, C)
    iw, ih = initref.plane_size(10, 6, C)
    assert got.shape == exp.shape == (ih, iw, 2)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.isfinite(got).all()


def test_initref_lookup_and_sanitize():
    plane = np.arange(30, dtype=f32).reshape(3, 5, 2)
    plane[1, 2] = (np.nan, 2e9)
    init = initref.lookup(plane)
    assert init(0, f32(8), f32(4)) == (plane[2, 4, 0] * 2, plane[2, 4, 1] * 2)  # the last cell of an odd 9 x 5 level
    assert init(0, f32(4), f32(3)) == (0.0, 0.0)
    assert init(0, f32(0), f32(0)) == (0.0, 2.0)
    s = initref.sanitize(np.array([1.5, -np.inf, np.nan, 1e9, -999999936.0], f32))
    assert s.tolist() == [1.5, 0.0, 0.0, 0.0, -999999936.0]


def _engine_without_library(disflow_mod, W, H, C):
    """A DenseInverseSearch whose context was never created: every path that
    reaches the library would fail on the null context, and the checks below
    must raise before that."""
    eng = object.__new__(disflow_mod.DenseInverseSearch)
    eng.params = disflow_mod.Params(coarsest_scale=C, finest_scale=0)
    eng.width, eng.height, eng.max_batch, eng.device = W, H, 4, 0
    eng._ctx = None
    return eng


def test_python_init_checks_raise_before_any_library_call(disflow_mod, monkeypatch):
    called = []

    def no_lib():
        called.append(1)
        raise AssertionError("the library was reached")

    monkeypatch.setattr(disflow_mod, "lib", no_lib)
    W, H, C = 36, 20, 2
    eng = _engine_without_library(disflow_mod, W, H, C)
    assert eng._plane_shape() == (3, 5)
    I = np.zeros((H, W), np.uint8)
    bad = [
        (np.zeros((H, W, 2), f32), "dense"),          # unknown kind
        (np.zeros((H, W, 2), f32), 2),
        (np.zeros((H, W), f32), "fullres"),           # no vector axis
        (np.zeros((H, W + 1, 2), f32), "fullres"),    # wrong size
        (np.zeros((3, 5, 2), f32), "fullres"),        # a plane passed as a full-resolution flow
        (np.zeros((H, W, 2), f32), "coarse"),         # and the reverse
        (np.zeros((5, 3, 2), f32), "coarse"),         # transposed plane
    ]
    for init, kind in bad:
        with pytest.raises(disflow_mod.DisError) as e:
            eng.calc(I, I, init=init, init_kind=kind)
        assert e.value.status == disflow_mod.DIS_ERR_INVALID_ARGUMENT, (init.shape, kind)
    with pytest.raises(disflow_mod.DisError):  # one init for two pairs
        eng.calc_batch(np.stack([I, I]), np.stack([I, I]), init=np.zeros((1, H, W, 2), f32))
    with pytest.raises(disflow_mod.DisError):
        eng.calc_device(1, 8, 16, 24, init_ptr=32, init_kind="dense")
    with pytest.raises(disflow_mod.DisError):
        eng.flow_to_init(np.zeros((H, W + 2, 2), f32))
    assert not called


def test_plane_shape_matches_initref(disflow_mod):
    for W, H, C in [(37, 21, 2), (36, 20, 2), (200, 136, 6), (1920, 1080, 6), (64, 48, 0), (1, 1, 0)]:
        eng = _engine_without_library(disflow_mod, W, H, C)
        iw, ih = initref.plane_size(W, H, C)
        assert eng._plane_shape() == (ih, iw)


def test_aliasing_rules_under_asan_ubsan(tmp_path):
    """tests/cpp/args_host.cpp (csrc/dis_args.h: init may be flow itself or
    disjoint from it, never partly over it or over the frames; and the other
    pure argument rules: sizes, strides and extents, disjoint buffers)
    compiled with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "args_host")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "args_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower() and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout


def test_launch_args_under_asan_ubsan(tmp_path):
    """tests/cpp/launch_args_host.cpp compiled together with
    csrc/dis_launch_args.hip (geometry, the per-geometry constants and the
    kernel argument builders: host code that makes no HIP runtime call), the
    host side under -fsanitize=address,undefined, and run on the CPU."""
    exe = str(tmp_path / "launch_args_host")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Wall", "-O1", "-g",
                        "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "launch_args_host.cpp"),
                        os.path.join(PKG, "csrc", "dis_launch_args.hip"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower() and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout
