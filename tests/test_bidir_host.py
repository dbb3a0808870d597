"""CPU tests of the bidirectional-flow feature: the numpy restatement of the
forward-backward check (tests/fbref.py) on hand-derived cases, the argument
validation of dis_calc_bidir_batch_u8 and dis_flow_consistency (it runs before
any HIP call, so it answers without a device), and the CLI's usage text."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fbref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-using-dense-inverse-search_amd")
CLI = os.path.join(PKG, "disflow", "dis_flow")

W, H = 16, 4
BX, BY = slice(6, 10), slice(1, 3)  # the 4 x 2 block of flipped backward vectors


def _uniform(u, v):
    f = np.empty((H, W, 2), np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def test_restatement_uniform_shift():
    # fw = (3, 0) everywhere, bw = (-3, 0): every vector that stays in the frame
    # (x + 3 <= 15) comes back exactly; columns 13..15 leave it
    mask, err = fbref.check(_uniform(3, 0), _uniform(-3, 0))
    assert mask.dtype == np.uint8 and err.dtype == np.float32
    assert (mask[:, :13] == 255).all() and (err[:, :13] == 0.0).all()
    assert (mask[:, 13:] == 0).all() and np.isposinf(err[:, 13:]).all()


def _touching(fw, weights_matter):
    """Pixels whose target's taps (those with a non-zero bilinear weight, if
    weights_matter) lie in the block, from the tap indices themselves."""
    valid, ix0, ix1, iy0, iy1, a, b = fbref.taps(fw)
    blk = np.zeros((H, W), bool)
    blk[BY, BX] = True
    one = np.float32(1)
    hit = np.zeros((H, W), bool)
    for iy, ix, w in ((iy0, ix0, (one - a) * (one - b)), (iy0, ix1, a * (one - b)),
                      (iy1, ix0, (one - a) * b), (iy1, ix1, a * b)):
        hit |= blk[iy, ix] & ((w != 0) if weights_matter else True)
    return valid & hit


def test_restatement_flipped_block_integer_shift():
    # integer targets: a = b = 0, so only tap (iy0, ix0) carries weight; a pixel
    # flips when that tap is in the block (s = +3, err = 36 > 0.01 * 18 + 0.5)
    fw, bw = _uniform(3, 0), _uniform(-3, 0)
    bw[BY, BX, 0] = 3
    mask, err = fbref.check(fw, bw)
    flip = _touching(fw, weights_matter=True)
    assert flip.sum() == 8 and flip[1:3, 3:7].all()  # x + 3 in 6..9, y in 1..2
    exp = np.where(flip | ~fbref.taps(fw)[0], 0, 255)
    assert np.array_equal(mask, exp)
    assert (err[flip] == 36.0).all()


def test_restatement_flipped_block_half_pixel_shift():
    # targets at half pixels: all four taps weigh 1/4, so one tap in the block is
    # enough (k taps: err = 1.625 k^2 against a threshold below 0.7)
    fw, bw = _uniform(2.5, 0.5), _uniform(-2.5, -0.5)
    bw[BY, BX] = (2.5, 0.5)
    mask, err = fbref.check(fw, bw)
    valid = fbref.taps(fw)[0]
    assert valid[:3, :13].all() and valid.sum() == 39  # x + 2.5 <= 15 and y + 0.5 <= 3
    flip = _touching(fw, weights_matter=False)
    assert np.array_equal(flip, _touching(fw, weights_matter=True)) and flip.sum() == 15
    assert np.array_equal(mask, np.where(flip | ~valid, 0, 255))
    assert (err[valid & ~flip] == 0.0).all() and np.isposinf(err[~valid]).all()


def _lib(disflow_mod):
    return disflow_mod.lib()


def _consistency_args(**over):
    """A valid host call's arguments of dis_flow_consistency, by name."""
    fw = np.zeros((H, W, 2), np.float32)
    bw = np.zeros((H, W, 2), np.float32)
    mask = np.zeros((H, W), np.uint8)
    a = dict(fw=fw.ctypes.data, bw=bw.ctypes.data, n=1, width=W, height=H, alpha1=0.01, alpha2=0.5,
             mask=mask.ctypes.data, err=None, where=0, stream=None, device=0)
    a.update(over)
    return (fw, bw, mask), list(a.values())


@pytest.mark.parametrize("over", [
    dict(fw=None), dict(bw=None), dict(mask=None),
    dict(n=0), dict(n=-3), dict(width=0), dict(height=0), dict(width=-5),
    dict(alpha1=-0.01), dict(alpha2=-1.0), dict(alpha1=float("nan")), dict(alpha2=float("inf")),
    dict(alpha1=float("-inf")), dict(where=2),
    dict(n=2**31 - 1, width=2**24, height=2**24),  # more blocks than a grid holds
    dict(width=2**24 + 1),                         # pixel coordinates must be exact floats
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_flow_consistency_rejects_before_any_device_call(disflow_mod, over):
    L = _lib(disflow_mod)
    keep, args = _consistency_args(**over)
    assert L.dis_flow_consistency(*args) == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    assert L.dis_last_error()


def test_flow_consistency_valid_arguments_reach_the_device(disflow_mod):
    # the same call with nothing wrong gets past validation: it succeeds on a GPU
    # and reports the missing device without one
    import torch
    L = _lib(disflow_mod)
    keep, args = _consistency_args()
    st = L.dis_flow_consistency(*args)
    assert st == (disflow_mod.DIS_OK if torch.cuda.is_available() else disflow_mod.DIS_ERR_DEVICE)


@pytest.mark.parametrize("bad", ["I0", "I1", "flow_fw", "flow_bw", "n=0", "n=-1", "overlap", "where", "ctx"])
def test_calc_bidir_rejects_before_any_device_call(disflow_mod, bad):
    L = _lib(disflow_mod)
    I0 = np.zeros((H, W), np.uint8)
    I1 = np.zeros((H, W), np.uint8)
    fw = np.zeros((H, W, 2), np.float32)
    bw = np.zeros((H, W, 2), np.float32)
    a = dict(ctx=None, n=1, I0=I0.ctypes.data, I1=I1.ctypes.data, stride=0, pair_stride=0,
             flow_fw=fw.ctypes.data, flow_bw=bw.ctypes.data, where=0, stream=None)
    expect = {"I0": "null", "I1": "null", "flow_fw": "null", "flow_bw": "null", "n=0": "max_batch",
              "n=-1": "max_batch", "overlap": "overlap", "where": "dis_mem", "ctx": "ctx is null"}[bad]
    if bad in a and bad != "ctx":
        a[bad] = None if bad != "where" else 7
    elif bad.startswith("n="):
        a["n"] = int(bad[2:])
    elif bad == "overlap":
        a["flow_bw"] = a["flow_fw"]
    # (no context exists without a device: the checks that need none come first,
    # and each names its cause)
    assert L.dis_calc_bidir_batch_u8(*a.values()) == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    assert expect in L.dis_last_error().decode()


def test_png_gray_encoder_round_trip(tmp_path):
    exe = str(tmp_path / "png_gray_roundtrip")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(PKG, "cli"),
                           os.path.join(ROOT, "tests", "cpp", "png_gray_roundtrip.cpp"), "-o", exe, "-lz"])
    r = subprocess.run([exe, str(tmp_path / "g.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_cli_usage_names_bidir(tmp_path):
    subprocess.check_call(["make", "-s", "-C", PKG])
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "--bidir" in r.stdout and "--fb-alpha" in r.stdout
