"""CPU tests of the f16 flow format: the two entries are exported and declared,
dis_flow_convert and dis_set_flow_format validate their arguments before any
HIP call (so they answer without a device), and the Python binding's dtype
checks raise before any library call."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dis_abi.h")


def test_entries_and_enum_are_declared_and_exported(disflow_mod):
    src = open(HEADER).read()
    assert re.search(r"typedef enum dis_flow_format \{ DIS_FLOW_F32 = 0, DIS_FLOW_F16 = 1 \} dis_flow_format;", src)
    assert re.search(r"#define DIS_ABI_VERSION 8\b", src)  # additive within v8
    L = disflow_mod.lib()
    for name in ("dis_set_flow_format", "dis_flow_convert"):
        assert name in disflow_mod.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert (disflow_mod.FLOW_F32, disflow_mod.FLOW_F16) == (0, 1)
    assert L.dis_abi_version() == 8


def _convert_args(**over):
    src = np.zeros(8, np.float32)
    dst = np.zeros(8, np.float16)
    a = dict(src=src.ctypes.data, src_format=0, dst=dst.ctypes.data, dst_format=1, count=8, where=0, stream=None,
             device=0)
    a.update(over)
    return (src, dst), list(a.values())


@pytest.mark.parametrize("over,why", [
    (dict(src=None), "null"), (dict(dst=None), "null"),
    (dict(src_format=2), "DIS_FLOW"), (dict(dst_format=-1), "DIS_FLOW"), (dict(src_format=7, dst_format=7), "DIS_FLOW"),
    (dict(where=2), "dis_mem"), (dict(count=2 ** 41), "count"),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) if isinstance(o, dict) else o)
def test_flow_convert_rejects_before_any_device_call(disflow_mod, over, why):
    L = disflow_mod.lib()
    keep, args = _convert_args(**over)
    assert L.dis_flow_convert(*args) == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    assert why in L.dis_last_error().decode()


def test_flow_convert_rejects_overlap_and_misaligned_device_pointers(disflow_mod):
    L = disflow_mod.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert L.dis_flow_convert(p, 0, p + 8, 1, 8, 0, None, 0) == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    assert b"overlap" in L.dis_last_error()
    # (addresses only: refused before anything dereferences them)
    assert L.dis_flow_convert(p + 2, 0, p + 128, 1, 8, 1, None, 0) == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    assert b"aligned" in L.dis_last_error()
    assert L.dis_flow_convert(p, 0, p + 129, 1, 8, 1, None, 0) == disflow_mod.DIS_ERR_INVALID_ARGUMENT


def test_flow_convert_valid_arguments_reach_the_device(disflow_mod):
    # nothing wrong: succeeds on a GPU, reports the missing device without one;
    # an empty conversion needs neither
    import torch
    L = disflow_mod.lib()
    keep, args = _convert_args()
    st = L.dis_flow_convert(*args)
    assert st == (disflow_mod.DIS_OK if torch.cuda.is_available() else disflow_mod.DIS_ERR_DEVICE)
    keep, args = _convert_args(count=0)
    assert L.dis_flow_convert(*args) == disflow_mod.DIS_OK
    # equal formats on host pointers are a plain copy
    a = np.arange(8, dtype=np.float32)
    b = np.zeros(8, np.float32)
    assert L.dis_flow_convert(a.ctypes.data, 0, b.ctypes.data, 0, 8, 0, None, 0) == disflow_mod.DIS_OK
    assert np.array_equal(a, b)


def test_set_flow_format_needs_a_context(disflow_mod):
    L = disflow_mod.lib()
    assert L.dis_set_flow_format(None, 1) == disflow_mod.DIS_ERR_INVALID_ARGUMENT
    assert b"ctx is null" in L.dis_last_error()


def test_python_dtype_checks_raise_without_a_device(disflow_mod):
    S = disflow_mod
    p = S.Params(coarsest_scale=2, finest_scale=0)
    for bad in (np.float64, np.int16, "f8", None, object()):
        with pytest.raises(ValueError):
            S.DenseInverseSearch(p, 64, 48, flow_dtype=bad)  # before dis_create
        with pytest.raises(ValueError):
            S.flow_convert(np.zeros(4, np.float32), bad)
    with pytest.raises(ValueError):
        S.flow_convert(np.zeros(4, np.float64), np.float16)
    with pytest.raises(ValueError):
        S.flow_convert_device(0, np.float32, 0, np.int8, 4)
    assert S.flow_convert(np.zeros((0, 2), np.float32), np.float16).dtype == np.float16  # empty: no device call
    # the init checks of an engine, on an object that never reached dis_create
    eng = S.DenseInverseSearch.__new__(S.DenseInverseSearch)
    eng._ctx = ctypes.c_void_p()
    eng.params, eng.width, eng.height = p, 64, 48
    for dt, init_dt, kind, shape in ((np.float16, np.float32, "fullres", (1, 48, 64, 2)),
                                     (np.float16, np.float16, "coarse", (1, 6, 8, 2)),
                                     (np.float32, np.float16, "fullres", (1, 48, 64, 2)),
                                     (np.float32, np.float16, "coarse", (1, 6, 8, 2))):
        eng.flow_dtype = np.dtype(dt)
        with pytest.raises(ValueError):
            eng._check_init(np.zeros(shape, init_dt), kind, 1)
    eng.flow_dtype = np.dtype(np.float16)
    a, kind = eng._check_init(np.zeros((1, 48, 64, 2), np.float16), "fullres", 1)
    assert a.dtype == np.float16 and kind == S.INIT_FULLRES
    a, kind = eng._check_init(np.zeros((1, 6, 8, 2), np.float32), "coarse", 1)
    assert a.dtype == np.float32 and kind == S.INIT_COARSE
    eng.flow_dtype = np.dtype(np.float32)
    a, kind = eng._check_init(np.zeros((1, 48, 64, 2), np.float64), "fullres", 1)  # as before: converted
    assert a.dtype == np.float32
