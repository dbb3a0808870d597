"""disflow -- Python host mirror of the DIS engine's C-ABI (include/dis_abi.h).

The product is the HIP library ``libdis_hip.so`` next to this file; this module
only binds it with ctypes (plain pointers and sizes) so tests and the bench can
drive it. The interface mirrors the reference's entry points:

* :class:`DenseInverseSearch` ``.calc(I0, I1)`` -- u8 frames to full-resolution
  flow (the reference's per-pair body, src/main.cpp:135-198);
* :func:`optical_flow_from_pyramids` -- the ``OpticalFlow::OpticalFlowClass``
  constructor (include/optical_flow.hpp:43-54) over caller-built padded
  pyramids, returning the finest-level flow;
* :class:`Preset` -- build-defined presets.

There is no CPU fallback: every compute call goes to the HIP library and fails
loudly (:class:`DisError`) when it or a device is missing.
"""
from __future__ import annotations

import ctypes
import enum
import os
from dataclasses import dataclass

import numpy as np

# torch (if present) must own the process's HIP runtime before libdis_hip.so is
# loaded, so both bind the same libamdhip64 (it is plumbing: device buffers and
# streams for bench.py; never on the compute path of this module).
try:  # pragma: no cover - import side effect only
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DISFLOW_LIB") or os.path.join(_HERE, "libdis_hip.so")

DIS_OK = 0
DIS_ERR_INVALID_ARGUMENT = -1
DIS_ERR_UNSUPPORTED = -2
DIS_ERR_DEVICE = -3
DIS_ERR_OUT_OF_MEMORY = -4
DIS_ERR_INTERNAL = -5

MEM_HOST = 0
MEM_DEVICE = 1

STAGE_IMG0, STAGE_IMG1, STAGE_DX0, STAGE_DY0, STAGE_PATCH_U, STAGE_DENSE, STAGE_FALLBACK = range(7)

PRECISION_EXACT, PRECISION_FMA = 0, 1

KERNEL_PYRAMID, KERNEL_SEARCH, KERNEL_SEARCH_FINEST, KERNEL_DENSIFY, KERNEL_VR_LIN, KERNEL_VR_SOR = range(6)
KERNEL_INIT = 6  # the init-plane launch of a warm-started call
KERNEL_LUMA = 7  # the luma launch of a colour frame format

INIT_COARSE, INIT_FULLRES = 0, 1

FLOW_F32, FLOW_F16 = 0, 1  # dis_flow_format

BORDER_REPLICATE, BORDER_ZERO = 0, 1  # dis_border

MOTION_TRANSLATION, MOTION_SIMILARITY, MOTION_AFFINE = 0, 1, 2  # dis_motion_model

FRAME_GRAY8, FRAME_BGR8, FRAME_RGB8, FRAME_BGRA8, FRAME_RGBA8 = range(5)  # dis_frame_format
_FRAME_FORMATS = {"gray": FRAME_GRAY8, "bgr": FRAME_BGR8, "rgb": FRAME_RGB8, "bgra": FRAME_BGRA8,
                  "rgba": FRAME_RGBA8}
_FRAME_CHANNELS = {FRAME_GRAY8: 1, FRAME_BGR8: 3, FRAME_RGB8: 3, FRAME_BGRA8: 4, FRAME_RGBA8: 4}

YUV_BT601, YUV_BT709 = 0, 1  # dis_yuv_matrix
YUV_LIMITED, YUV_FULL = 0, 1  # dis_yuv_range
_YUV_MATRICES = {"bt601": YUV_BT601, "bt709": YUV_BT709, YUV_BT601: YUV_BT601, YUV_BT709: YUV_BT709}
_YUV_RANGES = {"limited": YUV_LIMITED, "full": YUV_FULL, YUV_LIMITED: YUV_LIMITED, YUV_FULL: YUV_FULL}


def _frame_format(fmt) -> int:
    """dis_frame_format of "gray" / "bgr" / "rgb" / "bgra" / "rgba" (or of the enum's
    own value); ValueError for anything else."""
    if isinstance(fmt, str) and fmt in _FRAME_FORMATS:
        return _FRAME_FORMATS[fmt]
    if isinstance(fmt, int) and not isinstance(fmt, bool) and fmt in _FRAME_CHANNELS:
        return int(fmt)
    raise ValueError(f"frame format must be one of {sorted(_FRAME_FORMATS)}, not {fmt!r}")


def _flow_format(dtype) -> int:
    """dis_flow_format of a flow dtype (np.float32 / np.float16); ValueError for any other."""
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt == np.float32:
        return FLOW_F32
    if dt == np.float16:
        return FLOW_F16
    raise ValueError(f"flow dtype must be float32 or float16, not {dtype!r}")


_FLOW_DTYPES = {FLOW_F32: np.dtype(np.float32), FLOW_F16: np.dtype(np.float16)}
_BORDERS = {"replicate": BORDER_REPLICATE, "zero": BORDER_ZERO, BORDER_REPLICATE: BORDER_REPLICATE,
            BORDER_ZERO: BORDER_ZERO}
_MOTION_MODELS = {"translation": MOTION_TRANSLATION, "similarity": MOTION_SIMILARITY, "affine": MOTION_AFFINE,
                  MOTION_TRANSLATION: MOTION_TRANSLATION, MOTION_SIMILARITY: MOTION_SIMILARITY,
                  MOTION_AFFINE: MOTION_AFFINE}
_INIT_KINDS = {"coarse": INIT_COARSE, "fullres": INIT_FULLRES, INIT_COARSE: INIT_COARSE, INIT_FULLRES: INIT_FULLRES}

# Every symbol include/dis_abi.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "dis_abi_version", "dis_last_error", "dis_preset_params", "dis_validate_params",
    "dis_workload_info", "dis_create", "dis_destroy", "dis_calc_u8", "dis_calc_batch_u8",
    "dis_flow_from_pyramids", "dis_set_debug", "dis_stage_size", "dis_debug_dump",
    "dis_set_kernel_timing", "dis_kernel_time", "dis_synth_pair", "dis_set_kernel_variant",
    "dis_set_concurrency", "dis_set_precision", "dis_set_graphs", "dis_flow_color", "dis_flo_info",
    "dis_read_flo", "dis_write_flo", "dis_build_kind", "dis_set_host_pipeline", "dis_host_pipeline_info",
    "dis_host_alloc", "dis_host_free", "dis_batch_stream_plan", "dis_check_stream_plan",
    "dis_calc_bidir_batch_u8", "dis_flow_consistency",
    "dis_init_plane_size", "dis_flow_to_init", "dis_calc_batch_init_u8",
    "dis_set_flow_format", "dis_flow_convert", "dis_flow_warp_u8",
    "dis_flow_interp_workspace", "dis_flow_interp_u8",
    "dis_set_frame_format", "dis_frames_to_gray_u8",
    "dis_flow_compose", "dis_flow_advect_points",
    "dis_flow_fill_workspace", "dis_flow_fill",
    "dis_flow_fit_motion_workspace", "dis_flow_fit_motion", "dis_motion_to_flow",
    "dis_denoise_weights", "dis_temporal_denoise_u8",
    "dis_motion_stabilize", "dis_warp_motion_u8",
    "dis_yuv420_to_frames_u8", "dis_frames_to_yuv420_u8",
    "dis_flow_fit_homography_workspace", "dis_flow_fit_homography", "dis_homography_to_flow",
    "dis_warp_homography_u8", "dis_homography_stabilize",
)


class Preset(enum.IntEnum):
    ULTRAFAST = 0
    FAST = 1
    MEDIUM = 2
    SLOW = 3
    REFERENCE = 4


class DisError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"dis status {status}: {msg}")
        self.status = status


class _Params(ctypes.Structure):
    _fields_ = [
        ("coarsest_scale", ctypes.c_int),
        ("finest_scale", ctypes.c_int),
        ("patch_size", ctypes.c_int),
        ("iterations", ctypes.c_int),
        ("patch_overlap", ctypes.c_float),
        ("patch_normalization", ctypes.c_int),
        ("var_refine_iters", ctypes.c_int),
        ("paper_mode", ctypes.c_int),
    ]


class _HostInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("chunk_pairs", "last_chunks", "last_direct_in", "last_direct_out")]


class _Workload(ctypes.Structure):
    _fields_ = [
        ("padded_width", ctypes.c_int),
        ("padded_height", ctypes.c_int),
        ("steps", ctypes.c_int),
        ("patches", ctypes.c_longlong),
        ("updates", ctypes.c_longlong),
        ("algorithmic_bytes", ctypes.c_double),
        ("search_bytes_finest", ctypes.c_double),
        ("search_bytes_all", ctypes.c_double),
        ("search_launches", ctypes.c_int),
        ("patches_finest", ctypes.c_longlong),
        ("search_flops_finest", ctypes.c_double),
    ]


@dataclass
class Params:
    coarsest_scale: int
    finest_scale: int
    patch_size: int = 8
    iterations: int = 25
    patch_overlap: float = 0.625
    patch_normalization: int = 1
    var_refine_iters: int = 0
    paper_mode: int = 0

    def _c(self) -> _Params:
        return _Params(self.coarsest_scale, self.finest_scale, self.patch_size, self.iterations,
                       self.patch_overlap, int(self.patch_normalization), self.var_refine_iters,
                       int(self.paper_mode))

    @staticmethod
    def _from_c(p: _Params) -> "Params":
        return Params(p.coarsest_scale, p.finest_scale, p.patch_size, p.iterations,
                      float(p.patch_overlap), p.patch_normalization, p.var_refine_iters, p.paper_mode)


_lib = None


def lib() -> ctypes.CDLL:
    """Load libdis_hip.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DisError(DIS_ERR_INTERNAL, f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P, I, F, D, Z, V = ctypes.POINTER, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
        L.dis_abi_version.restype = I
        L.dis_last_error.restype = ctypes.c_char_p
        L.dis_preset_params.argtypes = [I, I, I, P(_Params)]
        L.dis_validate_params.argtypes = [P(_Params), I, I]
        L.dis_workload_info.argtypes = [P(_Params), I, I, P(_Workload)]
        L.dis_create.argtypes = [P(V), P(_Params), I, I, I, I]
        L.dis_destroy.argtypes = [V]
        L.dis_calc_u8.argtypes = [V, V, V, Z, V, I, V]
        L.dis_calc_batch_u8.argtypes = [V, I, V, V, Z, Z, V, I, V]
        L.dis_flow_from_pyramids.argtypes = [P(V)] * 6 + [I, V, I, I, I, I, I, I, F, I, I]
        L.dis_set_debug.argtypes = [V, I]
        L.dis_set_kernel_variant.argtypes = [V, I]
        L.dis_set_concurrency.argtypes = [V, I]
        if L.dis_abi_version() >= 4:  # (older builds load for A/B timing only)
            L.dis_set_precision.argtypes = [V, I]
            L.dis_set_graphs.argtypes = [V, I]
        if L.dis_abi_version() >= 6:
            L.dis_build_kind.restype = ctypes.c_char_p
        if L.dis_abi_version() >= 8:
            L.dis_set_host_pipeline.argtypes = [V, I]
            L.dis_host_pipeline_info.argtypes = [V, P(_HostInfo)]
            L.dis_host_alloc.argtypes = [Z, P(V)]
            L.dis_host_free.argtypes = [V]
            L.dis_batch_stream_plan.argtypes = [I, I, P(I), I, P(I)]
            L.dis_check_stream_plan.argtypes = [P(I), I, I, I]
        if hasattr(L, "dis_calc_bidir_batch_u8"):  # (added within v8; older v8 builds load for A/B timing)
            L.dis_calc_bidir_batch_u8.argtypes = [V, I, V, V, Z, Z, V, V, I, V]
        if hasattr(L, "dis_flow_consistency"):
            L.dis_flow_consistency.argtypes = [V, V, I, I, I, F, F, V, V, I, V, I]
        if hasattr(L, "dis_calc_batch_init_u8"):  # (added within v8)
            L.dis_init_plane_size.argtypes = [V, P(I), P(I)]
            L.dis_flow_to_init.argtypes = [V, I, V, V, I, V]
            L.dis_calc_batch_init_u8.argtypes = [V, I, V, V, Z, Z, V, I, V, I, V]
        if hasattr(L, "dis_set_flow_format"):  # (added within v8)
            L.dis_set_flow_format.argtypes = [V, I]
            L.dis_flow_convert.argtypes = [V, I, V, I, Z, I, V, I]
        if hasattr(L, "dis_flow_warp_u8"):  # (added within v8)
            L.dis_flow_warp_u8.argtypes = [V, Z, Z, I, V, I, I, I, I, F, I, V, V, I, V, I]
        if hasattr(L, "dis_flow_interp_u8"):  # (added within v8)
            L.dis_flow_interp_workspace.argtypes = [I, I, I, P(Z)]
            L.dis_flow_interp_u8.argtypes = [V, V, Z, Z, I, V, V, I, I, I, I, F, V, V, V, I, V, I]
        if hasattr(L, "dis_frames_to_gray_u8"):  # (added within v8)
            L.dis_set_frame_format.argtypes = [V, I]
            L.dis_frames_to_gray_u8.argtypes = [V, Z, Z, I, I, I, I, V, Z, Z, I, V, I]
        if hasattr(L, "dis_flow_compose"):  # (added within v8)
            L.dis_flow_compose.argtypes = [V, I, V, I, I, I, I, V, V, V, I, V, I, V, I]
            L.dis_flow_advect_points.argtypes = [V, I, I, I, I, V, I, V, V, I, V, I]
        if hasattr(L, "dis_flow_fill"):  # (added within v8)
            L.dis_flow_fill_workspace.argtypes = [I, I, I, P(Z)]
            L.dis_flow_fill.argtypes = [V, I, V, I, I, I, V, I, V, V, I, V, I]
        if hasattr(L, "dis_flow_fit_motion"):  # (added within v8)
            L.dis_flow_fit_motion_workspace.argtypes = [I, I, I, P(Z)]
            L.dis_flow_fit_motion.argtypes = [V, I, V, I, I, I, I, I, ctypes.c_float, V, V, V, V, I, V, I]
            L.dis_motion_to_flow.argtypes = [V, I, I, I, V, I, I, V, I]
        if hasattr(L, "dis_temporal_denoise_u8"):
            L.dis_denoise_weights.argtypes = [ctypes.c_float, V]
            L.dis_temporal_denoise_u8.argtypes = [V, V, Z, Z, I, V, I, V, I, I, I, I, V, V, V, I, V, I]
        if hasattr(L, "dis_warp_motion_u8"):  # (added within v8)
            L.dis_motion_stabilize.argtypes = [V, I, I, I, I, ctypes.c_float, ctypes.c_float, V, V, P(I)]
            L.dis_warp_motion_u8.argtypes = [V, Z, Z, I, V, I, I, I, I, V, V, I, V, I]
        if hasattr(L, "dis_flow_fit_homography"):  # (added within v8)
            L.dis_flow_fit_homography_workspace.argtypes = [I, I, I, P(Z)]
            L.dis_flow_fit_homography.argtypes = [V, I, V, I, I, I, I, ctypes.c_float, V, V, V, V, I, V, I]
            L.dis_homography_to_flow.argtypes = [V, I, I, I, V, I, I, V, I]
            L.dis_homography_stabilize.argtypes = [V, I, I, I, I, ctypes.c_float, ctypes.c_float, V, V, P(I)]
            L.dis_warp_homography_u8.argtypes = [V, Z, Z, I, V, I, I, I, I, V, V, I, V, I]
        if hasattr(L, "dis_yuv420_to_frames_u8"):  # (added within v8)
            L.dis_yuv420_to_frames_u8.argtypes = [V, Z, Z, V, V, Z, Z, I, I, I, I, I, I, V, Z, Z, I, I, I, V, I]
            L.dis_frames_to_yuv420_u8.argtypes = [V, Z, Z, I, I, I, I, I, I, V, Z, Z, V, V, Z, Z, I, I, V, I]
        L.dis_stage_size.argtypes = [V, I, I, P(Z)]
        L.dis_debug_dump.argtypes = [V, I, I, I, V, Z]
        L.dis_set_kernel_timing.argtypes = [V, I]
        L.dis_kernel_time.argtypes = [V, I, P(I), P(D)]
        L.dis_synth_pair.argtypes = [ctypes.c_uint64, I, I, V, V, V]
        L.dis_flow_color.argtypes = [V, I, I, I, ctypes.c_float, V, I, V, I]
        L.dis_flo_info.argtypes = [ctypes.c_char_p, P(I), P(I)]
        L.dis_read_flo.argtypes = [ctypes.c_char_p, V, I, I, I]
        L.dis_write_flo.argtypes = [ctypes.c_char_p, V, I, I, I]
        for name in EXPORTED_SYMBOLS:
            if name not in ("dis_abi_version", "dis_last_error", "dis_build_kind") and hasattr(L, name):
                getattr(L, name).restype = I
        _lib = L
    return _lib


def build_kind() -> str:
    """"product" (the sources carry no compile-time variants since ABI v7)."""
    return lib().dis_build_kind().decode()


def _check(st: int) -> None:
    if st != DIS_OK:
        raise DisError(st, lib().dis_last_error().decode())


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def preset_params(preset: Preset, width: int, height: int) -> Params:
    p = _Params()
    _check(lib().dis_preset_params(int(preset), width, height, ctypes.byref(p)))
    return Params._from_c(p)


def validate(params: Params, width: int, height: int) -> int:
    return lib().dis_validate_params(ctypes.byref(params._c()), width, height)


def workload(params: Params, width: int, height: int) -> dict:
    w = _Workload()
    _check(lib().dis_workload_info(ctypes.byref(params._c()), width, height, ctypes.byref(w)))
    return {k: getattr(w, k) for k, _ in _Workload._fields_}


def flow_color(flow: np.ndarray, maxmotion: float = -1.0, device: int = 0) -> np.ndarray:
    """Middlebury colour coding (src/color_coding.cpp draw_optical_flow) of an
    (H, W, 2) or (n, H, W, 2) float field on the GPU -> u8 BGR (..., 3)."""
    f = np.ascontiguousarray(flow, dtype=np.float32)
    single = f.ndim == 3
    if single:
        f = f[None]
    if f.ndim != 4 or f.shape[-1] != 2:
        raise DisError(DIS_ERR_INVALID_ARGUMENT, "flow must be (H, W, 2) or (n, H, W, 2)")
    n, H, W = f.shape[:3]
    out = np.empty((n, H, W, 3), np.uint8)
    _check(lib().dis_flow_color(_ptr(f), n, W, H, float(maxmotion), _ptr(out), MEM_HOST, None, device))
    return out[0] if single else out


def flow_color_device(flow_ptr: int, n: int, width: int, height: int, bgr_ptr: int, maxmotion: float = -1.0,
                      stream: int = 0, device: int = 0) -> None:
    """dis_flow_color on raw device pointers (float32 fields, n * W * H * 3 bytes of BGR),
    asynchronous on `stream`."""
    _check(lib().dis_flow_color(flow_ptr, n, width, height, float(maxmotion), bgr_ptr, MEM_DEVICE, stream or None, device))


def flow_consistency(fw: np.ndarray, bw: np.ndarray, alpha1: float = 0.01, alpha2: float = 0.5,
                     with_err: bool = False, device: int = 0):
    """Forward-backward consistency (dis_flow_consistency) of (H, W, 2) or
    (n, H, W, 2) float fields on the GPU -> u8 mask (..., H, W), 255 where
    following fw and then the backward vector sampled there leads back within
    alpha1 * (|fw|^2 + |bw|^2) + alpha2; with_err: also the squared round-trip
    distance (float32, +inf where the target leaves the frame)."""
    f = np.ascontiguousarray(fw, dtype=np.float32)
    b = np.ascontiguousarray(bw, dtype=np.float32)
    single = f.ndim == 3
    if single:
        f, b = f[None], (b[None] if b.ndim == 3 else b)
    if f.ndim != 4 or f.shape[-1] != 2 or b.shape != f.shape:
        raise DisError(DIS_ERR_INVALID_ARGUMENT, "fw and bw must both be (H, W, 2) or (n, H, W, 2)")
    n, H, W = f.shape[:3]
    mask = np.empty((n, H, W), np.uint8)
    err = np.empty((n, H, W), np.float32) if with_err else None
    _check(lib().dis_flow_consistency(_ptr(f), _ptr(b), n, W, H, float(alpha1), float(alpha2), _ptr(mask),
                                      _ptr(err) if with_err else None, MEM_HOST, None, device))
    if single:
        mask, err = mask[0], (err[0] if with_err else None)
    return (mask, err) if with_err else mask


def flow_consistency_device(fw_ptr: int, bw_ptr: int, n: int, width: int, height: int, mask_ptr: int,
                            err_ptr: int = 0, alpha1: float = 0.01, alpha2: float = 0.5, stream: int = 0,
                            device: int = 0) -> None:
    """dis_flow_consistency on raw device pointers, asynchronous on `stream`."""
    _check(lib().dis_flow_consistency(fw_ptr, bw_ptr, n, width, height, float(alpha1), float(alpha2), mask_ptr,
                                      err_ptr or None, MEM_DEVICE, stream or None, device))


def flow_convert(array: np.ndarray, dtype, device: int = 0) -> np.ndarray:
    """dis_flow_convert on a host array: float32 <-> float16 flow values (any
    shape) on the GPU. float32 -> float16 is the engine's own narrowing (round
    to nearest even, subnormals kept, |v| >= 65520 -> +-inf); float16 -> float32
    is exact; equal dtypes copy."""
    src_format, dst_format = _flow_format(np.asarray(array).dtype), _flow_format(dtype)
    a = np.ascontiguousarray(array)
    out = np.empty(a.shape, _FLOW_DTYPES[dst_format])
    if a.size:
        _check(lib().dis_flow_convert(_ptr(a), src_format, _ptr(out), dst_format, a.size, MEM_HOST, None, device))
    return out


def flow_convert_device(src_ptr: int, src_dtype, dst_ptr: int, dst_dtype, count: int, stream: int = 0,
                        device: int = 0) -> None:
    """dis_flow_convert on raw device pointers (`count` values), asynchronous on `stream`."""
    _check(lib().dis_flow_convert(src_ptr, _flow_format(src_dtype), dst_ptr, _flow_format(dst_dtype), count,
                                  MEM_DEVICE, stream or None, device))


def _border(border) -> int:
    try:
        return _BORDERS[border]
    except (KeyError, TypeError):
        raise ValueError(f"border must be 'replicate' or 'zero', not {border!r}") from None


def flow_warp(image: np.ndarray, flow: np.ndarray, scale: float = 1.0, border="replicate",
              with_valid: bool = False, device: int = 0):
    """Backward warp (dis_flow_warp_u8) of u8 images by flow fields on the GPU:
    out(x, y) = image sampled bilinearly at (x + scale*u, y + scale*v), rounded
    to nearest even; with the I0 -> I1 flow and image = I1 the result
    reconstructs I0. image: (H, W), (H, W, C), (n, H, W) or (n, H, W, C) with C
    in 1, 3, 4 (a 3-D image is (H, W, C) when its leading dimensions match the
    flow's (H, W), else (n, H, W)); flow: float32 or float16 (..., H, W, 2),
    read in its own dtype. border: "replicate" (targets outside the frame are
    clamped) or "zero". Returns the warped array of the image's shape; with_valid:
    also the u8 mask (..., H, W), 255 where the target lies inside the frame.
    Invalid vectors (NaN, |c| >= 1e9) give 0 and valid 0."""
    fl = np.asarray(flow)
    fmt = _flow_format(fl.dtype)
    bd = _border(border)
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError(f"image dtype must be uint8, not {img.dtype}")
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError("flow must be (H, W, 2) or (n, H, W, 2)")
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    if img.ndim == 2:
        shape4 = (1,) + img.shape + (1,)
    elif img.ndim == 3:
        shape4 = (1,) + img.shape if img.shape[:2] == (H, W) else img.shape + (1,)
    elif img.ndim == 4:
        shape4 = img.shape
    else:
        raise ValueError("image must be (H, W), (H, W, C), (n, H, W) or (n, H, W, C)")
    if shape4[:3] != (n, H, W):
        raise ValueError(f"image shape {img.shape} does not match flow shape {fl.shape}")
    C = shape4[3]
    if C not in (1, 3, 4):
        raise ValueError(f"image must have 1, 3 or 4 channels, not {C}")
    img = np.ascontiguousarray(img)
    fl = np.ascontiguousarray(fl)
    out = np.empty(img.shape, np.uint8)
    valid = np.empty(fl.shape[:-1], np.uint8) if with_valid else None
    _check(lib().dis_flow_warp_u8(_ptr(img), 0, 0, C, _ptr(fl), fmt, n, W, H, float(scale), bd, _ptr(out),
                                  _ptr(valid) if with_valid else None, MEM_HOST, None, device))
    return (out, valid) if with_valid else out


def flow_warp_device(src_ptr: int, flow_ptr: int, flow_dtype, n: int, width: int, height: int, channels: int,
                     dst_ptr: int, valid_ptr: int = 0, scale: float = 1.0, border="replicate", src_stride: int = 0,
                     src_image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_flow_warp_u8 on raw device pointers, asynchronous on `stream`."""
    fmt, bd = _flow_format(flow_dtype), _border(border)
    _check(lib().dis_flow_warp_u8(src_ptr, src_stride, src_image_stride, channels, flow_ptr, fmt, n, width, height,
                                  float(scale), bd, dst_ptr, valid_ptr or None, MEM_DEVICE, stream or None, device))


def flow_interp_workspace(n: int, width: int, height: int) -> int:
    """Bytes of dis_flow_interp_u8's workspace for n W x H pairs (n*W*H*8)."""
    b = ctypes.c_size_t()
    _check(lib().dis_flow_interp_workspace(n, width, height, ctypes.byref(b)))
    return b.value


def _interp_time(t) -> float:
    t = float(t)
    if not 0.0 <= t <= 1.0:  # (False for NaN)
        raise ValueError(f"t must lie in [0, 1], not {t!r}")
    return t


def flow_interp(I0: np.ndarray, I1: np.ndarray, fw: np.ndarray, t: float, bw=None, return_fill: bool = False,
                device: int = 0):
    """The frame at time t in [0, 1] between I0 and I1 (dis_flow_interp_u8) on the
    GPU: the forward flow fw (I0 -> I1) is projected to time t, collisions go to
    the candidate with the lower photometric cost, and both frames are sampled
    with the projected flow; holes are filled from I1 through bw (I1 -> I0) where
    it is given and leads inside the frame, else with fw's own vector there.
    I0, I1: u8 images of one shape, flow_warp's layouts; fw, bw: float32 or
    float16 (..., H, W, 2) of one dtype and shape, read in their own dtype.
    Returns the frame in the images' shape; return_fill: also the u8 map
    (..., H, W): 0 = a projected vector, 1 = filled from bw, 2 = filled from fw."""
    fl = np.asarray(fw)
    fmt = _flow_format(fl.dtype)
    t = _interp_time(t)
    a, b = np.asarray(I0), np.asarray(I1)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError(f"image dtype must be uint8, not {a.dtype} and {b.dtype}")
    if a.shape != b.shape:
        raise ValueError(f"I0 and I1 must have one shape, not {a.shape} and {b.shape}")
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError("fw must be (H, W, 2) or (n, H, W, 2)")
    if bw is not None:
        bl = np.asarray(bw)
        if bl.dtype != fl.dtype or bl.shape != fl.shape:
            raise ValueError(f"bw must have fw's dtype and shape ({fl.dtype} {fl.shape}), not {bl.dtype} {bl.shape}")
        bl = np.ascontiguousarray(bl)
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    if a.ndim == 2:
        shape4 = (1,) + a.shape + (1,)
    elif a.ndim == 3:
        shape4 = (1,) + a.shape if a.shape[:2] == (H, W) else a.shape + (1,)
    elif a.ndim == 4:
        shape4 = a.shape
    else:
        raise ValueError("images must be (H, W), (H, W, C), (n, H, W) or (n, H, W, C)")
    if shape4[:3] != (n, H, W):
        raise ValueError(f"image shape {a.shape} does not match flow shape {fl.shape}")
    C = shape4[3]
    if C not in (1, 3, 4):
        raise ValueError(f"images must have 1, 3 or 4 channels, not {C}")
    a, b, fl = np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(fl)
    out = np.empty(a.shape, np.uint8)
    fill = np.empty(fl.shape[:-1], np.uint8) if return_fill else None
    _check(lib().dis_flow_interp_u8(_ptr(a), _ptr(b), 0, 0, C, _ptr(fl), _ptr(bl) if bw is not None else None, fmt,
                                    n, W, H, t, _ptr(out), _ptr(fill) if return_fill else None, None, MEM_HOST,
                                    None, device))
    return (out, fill) if return_fill else out


def flow_interp_device(I0_ptr: int, I1_ptr: int, fw_ptr: int, flow_dtype, n: int, width: int, height: int,
                       channels: int, t: float, dst_ptr: int, workspace_ptr: int, bw_ptr: int = 0, fill_ptr: int = 0,
                       stride: int = 0, image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_flow_interp_u8 on raw device pointers, asynchronous on `stream`;
    workspace_ptr: flow_interp_workspace(n, width, height) bytes, 8-byte aligned."""
    fmt, t = _flow_format(flow_dtype), _interp_time(t)
    _check(lib().dis_flow_interp_u8(I0_ptr, I1_ptr, stride, image_stride, channels, fw_ptr, bw_ptr or None, fmt, n,
                                    width, height, t, dst_ptr, fill_ptr or None, workspace_ptr or None, MEM_DEVICE,
                                    stream or None, device))


def _byte_plane(plane, shape, name):
    """An optional u8 plane of flow_compose as a contiguous array of `shape`."""
    if plane is None:
        return None
    m = np.asarray(plane)
    if m.dtype != np.uint8:
        raise ValueError(f"{name} dtype must be uint8, not {m.dtype}")
    if m.shape != shape:
        raise ValueError(f"{name} must be {shape}, not {m.shape}")
    return np.ascontiguousarray(m)


def flow_compose(a: np.ndarray, b: np.ndarray, valid_a=None, mask_b=None, out_dtype=np.float32,
                 with_valid: bool = False, device: int = 0):
    """Composition of flow fields (dis_flow_compose) on the GPU: with `a` the flow
    from frame 0 to frame k and `b` the flow from frame k to frame k+1, returns
    the flow from frame 0 to frame k+1, a(x) + b sampled bilinearly at x + a(x).
    a, b: float32 or float16 (H, W, 2) or (n, H, W, 2) of one shape, each read in
    its own dtype; out_dtype: float32 (default) or float16. valid_a, mask_b:
    optional u8 (..., H, W), nonzero = trusted (the previous call's valid and
    flow_consistency's mask of pair k). A pixel whose vector is invalid (NaN,
    |c| >= 1e9) or not trusted, whose target leaves the frame, or one of whose
    four taps of b is invalid or masked out gets NaN; with_valid: also the u8
    map (..., H, W), 255 where the result is a vector."""
    fa, fb = np.asarray(a), np.asarray(b)
    a_fmt, b_fmt, o_fmt = _flow_format(fa.dtype), _flow_format(fb.dtype), _flow_format(out_dtype)
    if fa.ndim not in (3, 4) or fa.shape[-1] != 2 or fb.shape != fa.shape:
        raise ValueError(f"a and b must both be (H, W, 2) or (n, H, W, 2), not {fa.shape} and {fb.shape}")
    va = _byte_plane(valid_a, fa.shape[:-1], "valid_a")
    mb = _byte_plane(mask_b, fa.shape[:-1], "mask_b")
    H, W = fa.shape[-3], fa.shape[-2]
    n = fa.shape[0] if fa.ndim == 4 else 1
    fa, fb = np.ascontiguousarray(fa), np.ascontiguousarray(fb)
    out = np.empty(fa.shape, _FLOW_DTYPES[o_fmt])
    valid = np.empty(fa.shape[:-1], np.uint8) if with_valid else None
    _check(lib().dis_flow_compose(_ptr(fa), a_fmt, _ptr(fb), b_fmt, n, W, H, None if va is None else _ptr(va),
                                  None if mb is None else _ptr(mb), _ptr(out), o_fmt,
                                  _ptr(valid) if with_valid else None, MEM_HOST, None, device))
    return (out, valid) if with_valid else out


def flow_compose_device(a_ptr: int, a_dtype, b_ptr: int, b_dtype, n: int, width: int, height: int, out_ptr: int,
                        out_dtype=np.float32, valid_a_ptr: int = 0, mask_b_ptr: int = 0, valid_out_ptr: int = 0,
                        stream: int = 0, device: int = 0) -> None:
    """dis_flow_compose on raw device pointers, asynchronous on `stream`. out_ptr
    may be a_ptr (equal dtypes) and valid_out_ptr valid_a_ptr: in place."""
    a_fmt, b_fmt, o_fmt = _flow_format(a_dtype), _flow_format(b_dtype), _flow_format(out_dtype)
    _check(lib().dis_flow_compose(a_ptr, a_fmt, b_ptr, b_fmt, n, width, height, valid_a_ptr or None,
                                  mask_b_ptr or None, out_ptr, o_fmt, valid_out_ptr or None, MEM_DEVICE,
                                  stream or None, device))


def flow_fill_workspace(n: int, width: int, height: int) -> int:
    """Bytes of device workspace dis_flow_fill needs for n W x H fields on device
    pointers: 8 per cell of the push-pull levels above the field (0 for 1 x 1)."""
    b = ctypes.c_size_t(0)
    _check(lib().dis_flow_fill_workspace(n, width, height, ctypes.byref(b)))
    return int(b.value)


def flow_fill(flow: np.ndarray, mask=None, out_dtype=np.float32, with_level: bool = False, device: int = 0):
    """Untrusted vectors of flow fields replaced from the trusted ones by
    push-pull (dis_flow_fill) on the GPU. flow: float32 or float16 (H, W, 2) or
    (n, H, W, 2); mask: optional u8 (..., H, W), nonzero = trusted
    (flow_consistency's mask, flow_compose's valid map); out_dtype: float32
    (default) or float16. A trusted vector (not NaN, |c| < 1e9, mask byte not 0)
    is kept; every other pixel gets the bilinear upsample of the nearest coarser
    level that holds trusted data. A field without any trusted vector comes back
    as NaN. with_level: also the u8 map (..., H, W) of the level each vector came
    from: 0 = kept, l = from about 2^l pixels away, 255 = empty field."""
    fl = np.asarray(flow)
    f_fmt, o_fmt = _flow_format(fl.dtype), _flow_format(out_dtype)
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError(f"flow must be (H, W, 2) or (n, H, W, 2), not {fl.shape}")
    m = _byte_plane(mask, fl.shape[:-1], "mask")
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    fl = np.ascontiguousarray(fl)
    out = np.empty(fl.shape, _FLOW_DTYPES[o_fmt])
    level = np.empty(fl.shape[:-1], np.uint8) if with_level else None
    _check(lib().dis_flow_fill(_ptr(fl), f_fmt, None if m is None else _ptr(m), n, W, H, _ptr(out), o_fmt,
                               _ptr(level) if with_level else None, None, MEM_HOST, None, device))
    return (out, level) if with_level else out


def flow_fill_device(flow_ptr: int, flow_dtype, n: int, width: int, height: int, out_ptr: int, workspace_ptr: int,
                     out_dtype=np.float32, mask_ptr: int = 0, level_ptr: int = 0, stream: int = 0,
                     device: int = 0) -> None:
    """dis_flow_fill on raw device pointers, asynchronous on `stream`.
    workspace_ptr: flow_fill_workspace(n, width, height) bytes, 8-byte aligned
    (0 for 1 x 1 fields). out_ptr may be flow_ptr (equal dtypes): in place."""
    f_fmt, o_fmt = _flow_format(flow_dtype), _flow_format(out_dtype)
    _check(lib().dis_flow_fill(flow_ptr, f_fmt, mask_ptr or None, n, width, height, out_ptr, o_fmt, level_ptr or None,
                               workspace_ptr or None, MEM_DEVICE, stream or None, device))


def _motion_args(model, iterations, threshold):
    """(dis_motion_model, iterations, threshold) of fit_motion, checked as the library checks them."""
    if isinstance(model, bool) or model not in _MOTION_MODELS:
        raise ValueError(f"model must be 'translation', 'similarity' or 'affine', not {model!r}")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= 16:
        raise ValueError(f"iterations must be an integer in [0, 16], not {iterations!r}")
    t = float(threshold)
    if not (abs(t) <= float(np.finfo(np.float32).max) and t >= 0.0):  # (false for NaN; what a float holds)
        raise ValueError(f"threshold must be finite and >= 0, not {threshold!r}")
    return _MOTION_MODELS[model], int(iterations), t


def fit_motion_workspace(n: int, width: int, height: int) -> int:
    """Bytes of device workspace dis_flow_fit_motion needs for n W x H fields on
    device pointers: n * (ceil(W * H / 16384) * 12 + 16) * 8."""
    b = ctypes.c_size_t(0)
    _check(lib().dis_flow_fit_motion_workspace(n, width, height, ctypes.byref(b)))
    return int(b.value)


def fit_motion(flow: np.ndarray, mask=None, model="affine", iterations: int = 3, threshold: float = 1.0,
               return_info: bool = False, return_inliers: bool = False, device: int = 0):
    """The global motion of flow fields (dis_flow_fit_motion) on the GPU: a
    "translation", "similarity" or "affine" model fitted to the trusted vectors
    by least squares, then refitted `iterations` times on the trusted vectors
    within `threshold` pixels of the previous fit, so that moving objects and
    outliers drop out. flow: float32 or float16 (H, W, 2) or (n, H, W, 2); mask:
    optional u8 (..., H, W), nonzero = trusted (flow_consistency's mask,
    flow_compose's valid map). Returns float32 params (6,) or (n, 6) with
    u = p0 + p1 x + p2 y, v = p3 + p4 x + p5 y over pixel indices; NaN where the
    fit failed (too few or collinear vectors). return_info: also uint32 (..., 4)
    {1 fitted / 0 failed, trusted pixels, pixels of the last fit, pixels that
    agree (0 without return_inliers)}; return_inliers: also the u8 plane
    (..., H, W), 255 where a trusted vector lies within the threshold of the
    result: its complement is the moving-object mask. Order: params, info,
    inliers."""
    fl = np.asarray(flow)
    fmt = _flow_format(fl.dtype)
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError(f"flow must be (H, W, 2) or (n, H, W, 2), not {fl.shape}")
    m = _byte_plane(mask, fl.shape[:-1], "mask")
    mdl, its, thr = _motion_args(model, iterations, threshold)
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    lead = fl.shape[:-3]
    fl = np.ascontiguousarray(fl)
    params = np.empty(lead + (6,), np.float32)
    info = np.empty(lead + (4,), np.uint32) if return_info else None
    inl = np.empty(fl.shape[:-1], np.uint8) if return_inliers else None
    _check(lib().dis_flow_fit_motion(_ptr(fl), fmt, None if m is None else _ptr(m), n, W, H, mdl, its, thr,
                                     _ptr(params), _ptr(info) if return_info else None,
                                     _ptr(inl) if return_inliers else None, None, MEM_HOST, None, device))
    out = (params,) + ((info,) if return_info else ()) + ((inl,) if return_inliers else ())
    return out if len(out) > 1 else params


def fit_motion_device(flow_ptr: int, flow_dtype, n: int, width: int, height: int, params_ptr: int, workspace_ptr: int,
                      model="affine", iterations: int = 3, threshold: float = 1.0, mask_ptr: int = 0,
                      info_ptr: int = 0, inliers_ptr: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_flow_fit_motion on raw device pointers, asynchronous on `stream`: no
    allocation and no host synchronisation, so it can be captured.
    workspace_ptr: fit_motion_workspace(n, width, height) bytes, 8-byte aligned;
    params_ptr: n * 6 float32; info_ptr: n * 4 uint32; inliers_ptr: n * W * H bytes."""
    fmt = _flow_format(flow_dtype)
    mdl, its, thr = _motion_args(model, iterations, threshold)
    _check(lib().dis_flow_fit_motion(flow_ptr, fmt, mask_ptr or None, n, width, height, mdl, its, thr, params_ptr,
                                     info_ptr or None, inliers_ptr or None, workspace_ptr or None, MEM_DEVICE,
                                     stream or None, device))


def motion_to_flow(params: np.ndarray, width: int, height: int, out_dtype=np.float32, device: int = 0) -> np.ndarray:
    """The flow field of motion models (dis_motion_to_flow) on the GPU: params
    float32 (6,) -> (H, W, 2), or (n, 6) -> (n, H, W, 2), u = (p0 + p1 x) + p2 y,
    v = (p3 + p4 x) + p5 y in float32, as out_dtype (float32 or float16). A model
    with a parameter that is not finite (a failed fit) gives a NaN field. The
    result feeds flow_warp (the stabilised frame) and flow_compose."""
    p = np.asarray(params)
    o_fmt = _flow_format(out_dtype)
    if p.dtype != np.float32:
        raise ValueError(f"params dtype must be float32, not {p.dtype}")
    if p.ndim not in (1, 2) or p.shape[-1] != 6 or p.size == 0:
        raise ValueError(f"params must be (6,) or (n, 6), not {p.shape}")
    if isinstance(width, bool) or isinstance(height, bool) or not isinstance(width, (int, np.integer)) or \
            not isinstance(height, (int, np.integer)) or width < 1 or height < 1:
        raise ValueError(f"width and height must be integers >= 1, not {width!r}, {height!r}")
    n = p.shape[0] if p.ndim == 2 else 1
    p = np.ascontiguousarray(p)
    out = np.empty(p.shape[:-1] + (int(height), int(width), 2), _FLOW_DTYPES[o_fmt])
    _check(lib().dis_motion_to_flow(_ptr(p), n, int(width), int(height), _ptr(out), o_fmt, MEM_HOST, None, device))
    return out


def motion_to_flow_device(params_ptr: int, n: int, width: int, height: int, out_ptr: int, out_dtype=np.float32,
                          stream: int = 0, device: int = 0) -> None:
    """dis_motion_to_flow on raw device pointers, asynchronous on `stream`."""
    o_fmt = _flow_format(out_dtype)
    _check(lib().dis_motion_to_flow(params_ptr, n, width, height, out_ptr, o_fmt, MEM_DEVICE, stream or None, device))


STABILIZE_MAX_RADIUS = 1024


def _stabilize_args(radius, sigma, zoom):
    """(radius, sigma, zoom) of stabilize_path, checked as the library checks them;
    sigma None: max(radius, 1) / 2."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or \
            not 0 <= radius <= STABILIZE_MAX_RADIUS:
        raise ValueError(f"radius must be an integer in [0, {STABILIZE_MAX_RADIUS}], not {radius!r}")
    s = max(int(radius), 1) / 2.0 if sigma is None else float(sigma)
    if not (0.0 < s <= float(np.finfo(np.float32).max)) or float(np.float32(s)) <= 0.0:  # (false for NaN)
        raise ValueError(f"sigma must be finite and > 0, not {sigma!r}")
    z = float(zoom)
    if not 1.0 <= z <= 16.0:  # (false for NaN)
        raise ValueError(f"zoom must lie in [1, 16], not {zoom!r}")
    return int(radius), s, z


def stabilize_path(pair_params, width: int, height: int, radius: int, sigma=None, zoom: float = 1.0,
                   with_status: bool = False):
    """The corrections of a stabiliser (dis_motion_stabilize, host only): the
    float32 (N-1, 6) models of consecutive pairs (fit_motion's params, frame k ->
    k+1; shape (0, 6) for a single frame) are composed into the camera path, the
    path is smoothed by a Gaussian of `sigma` frames (None: max(radius, 1) / 2)
    cut at `radius` frames, and frame k's correction is the model that moves it
    from the path onto the smoothed path, magnified by `zoom` (1..16) about the
    centre of the W x H frame. Returns float32 (N, 6): what warp_motion takes
    (or motion_to_flow and flow_warp). A pair model that is not finite (a failed
    fit) counts as no motion. with_status: (corrections, status u8 (N,),
    replaced): status 0 where the smoothed path could not be inverted (the
    correction is then all zeros), replaced the number of pair models that
    were not finite."""
    r, s, z = _stabilize_args(radius, sigma, zoom)
    p = np.asarray(pair_params)
    if p.dtype != np.float32:
        raise ValueError(f"pair_params dtype must be float32, not {p.dtype}")
    if p.ndim != 2 or p.shape[1] != 6:
        raise ValueError(f"pair_params must be (N-1, 6), not {p.shape}")
    if isinstance(width, bool) or isinstance(height, bool) or not isinstance(width, (int, np.integer)) or \
            not isinstance(height, (int, np.integer)) or width < 1 or height < 1:
        raise ValueError(f"width and height must be integers >= 1, not {width!r}, {height!r}")
    p = np.ascontiguousarray(p)
    n = p.shape[0] + 1
    out = np.empty((n, 6), np.float32)
    status = np.empty(n, np.uint8)
    replaced = ctypes.c_int(0)
    _check(lib().dis_motion_stabilize(_ptr(p) if n > 1 else None, n, int(width), int(height), r, s, z, _ptr(out),
                                      _ptr(status), ctypes.byref(replaced)))
    return (out, status, int(replaced.value)) if with_status else out


def warp_motion(image: np.ndarray, params: np.ndarray, border="replicate", return_valid: bool = False,
                device: int = 0):
    """Backward warp (dis_warp_motion_u8) of u8 images by motion models on the
    GPU: bit for bit flow_warp(image, motion_to_flow(params, W, H)), without the
    field. image: (H, W) or (H, W, C) with params float32 (6,), or (n, H, W) or
    (n, H, W, C) with params (n, 6); C in 1, 3, 4. border: "replicate" or "zero".
    Returns the warped array of the image's shape; return_valid: also the u8 mask
    (..., H, W), 255 where the target lies inside the frame. A model with a
    parameter that is not finite gives 0 everywhere and valid 0."""
    bd = _border(border)
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError(f"image dtype must be uint8, not {img.dtype}")
    p = np.asarray(params)
    if p.dtype != np.float32:
        raise ValueError(f"params dtype must be float32, not {p.dtype}")
    if p.ndim not in (1, 2) or p.shape[-1] != 6 or p.size == 0:
        raise ValueError(f"params must be (6,) or (n, 6), not {p.shape}")
    if p.ndim == 1:
        if img.ndim not in (2, 3):
            raise ValueError("one model takes an (H, W) or (H, W, C) image")
        shape4 = (1,) + img.shape + ((1,) if img.ndim == 2 else ())
    else:
        if img.ndim not in (3, 4):
            raise ValueError("(n, 6) models take (n, H, W) or (n, H, W, C) images")
        shape4 = img.shape + ((1,) if img.ndim == 3 else ())
        if shape4[0] != p.shape[0]:
            raise ValueError(f"image shape {img.shape} does not match params shape {p.shape}")
    n, H, W, C = shape4
    if C not in (1, 3, 4):
        raise ValueError(f"image must have 1, 3 or 4 channels, not {C}")
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"image shape {img.shape} has an empty dimension")
    img = np.ascontiguousarray(img)
    p = np.ascontiguousarray(p)
    out = np.empty(img.shape, np.uint8)
    valid = np.empty(shape4[:3] if p.ndim == 2 else shape4[1:3], np.uint8) if return_valid else None
    _check(lib().dis_warp_motion_u8(_ptr(img), 0, 0, C, _ptr(p), n, W, H, bd, _ptr(out),
                                    _ptr(valid) if return_valid else None, MEM_HOST, None, device))
    return (out, valid) if return_valid else out


def warp_motion_device(src_ptr: int, params_ptr: int, n: int, width: int, height: int, channels: int, dst_ptr: int,
                       valid_ptr: int = 0, border="replicate", src_stride: int = 0, src_image_stride: int = 0,
                       stream: int = 0, device: int = 0) -> None:
    """dis_warp_motion_u8 on raw device pointers (params_ptr: n * 6 float32 in
    device memory), asynchronous on `stream`: one launch, no allocation, no
    synchronisation."""
    bd = _border(border)
    _check(lib().dis_warp_motion_u8(src_ptr, src_stride, src_image_stride, channels, params_ptr, n, width, height, bd,
                                    dst_ptr, valid_ptr or None, MEM_DEVICE, stream or None, device))


def _fit_args(iterations, threshold):
    """(iterations, threshold) of fit_homography, checked as the library checks them."""
    _, its, thr = _motion_args(MOTION_AFFINE, iterations, threshold)
    return its, thr


def _models8(params, name="params"):
    """float32 (8,) or (n, 8) models, contiguous."""
    p = np.asarray(params)
    if p.dtype != np.float32:
        raise ValueError(f"{name} dtype must be float32, not {p.dtype}")
    if p.ndim not in (1, 2) or p.shape[-1] != 8 or p.size == 0:
        raise ValueError(f"{name} must be (8,) or (n, 8), not {p.shape}")
    return np.ascontiguousarray(p)


def _sides(width, height):
    if isinstance(width, bool) or isinstance(height, bool) or not isinstance(width, (int, np.integer)) or \
            not isinstance(height, (int, np.integer)) or width < 1 or height < 1:
        raise ValueError(f"width and height must be integers >= 1, not {width!r}, {height!r}")
    return int(width), int(height)


def fit_homography_workspace(n: int, width: int, height: int) -> int:
    """Bytes of device workspace dis_flow_fit_homography needs for n W x H fields
    on device pointers: n * (ceil(W * H / 16384) * 27 + 16) * 8."""
    b = ctypes.c_size_t(0)
    _check(lib().dis_flow_fit_homography_workspace(n, width, height, ctypes.byref(b)))
    return int(b.value)


def fit_homography(flow: np.ndarray, mask=None, iterations: int = 3, threshold: float = 1.0,
                   return_info: bool = False, return_inliers: bool = False, device: int = 0):
    """The global motion of flow fields as a homography (dis_flow_fit_homography)
    on the GPU: what fit_motion does for its three models, for the eight-
    parameter projective model that a rotating camera induces. flow, mask,
    iterations, threshold, return_info and return_inliers as for fit_motion.
    Returns float32 params (8,) or (n, 8): with g = p6 x + p7 y,
    u = (p0 + p1 x + p2 y - x g) / (1 + g), v = (p3 + p4 x + p5 y - y g) / (1 + g)
    over pixel indices; NaN where the fit failed (fewer than four vectors in
    general position, or a model whose horizon comes near the frame). Order:
    params, info, inliers."""
    fl = np.asarray(flow)
    fmt = _flow_format(fl.dtype)
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError(f"flow must be (H, W, 2) or (n, H, W, 2), not {fl.shape}")
    m = _byte_plane(mask, fl.shape[:-1], "mask")
    its, thr = _fit_args(iterations, threshold)
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    lead = fl.shape[:-3]
    fl = np.ascontiguousarray(fl)
    params = np.empty(lead + (8,), np.float32)
    info = np.empty(lead + (4,), np.uint32) if return_info else None
    inl = np.empty(fl.shape[:-1], np.uint8) if return_inliers else None
    _check(lib().dis_flow_fit_homography(_ptr(fl), fmt, None if m is None else _ptr(m), n, W, H, its, thr,
                                         _ptr(params), _ptr(info) if return_info else None,
                                         _ptr(inl) if return_inliers else None, None, MEM_HOST, None, device))
    out = (params,) + ((info,) if return_info else ()) + ((inl,) if return_inliers else ())
    return out if len(out) > 1 else params


def fit_homography_device(flow_ptr: int, flow_dtype, n: int, width: int, height: int, params_ptr: int,
                          workspace_ptr: int, iterations: int = 3, threshold: float = 1.0, mask_ptr: int = 0,
                          info_ptr: int = 0, inliers_ptr: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_flow_fit_homography on raw device pointers, asynchronous on `stream`:
    no allocation and no host synchronisation. workspace_ptr:
    fit_homography_workspace(n, width, height) bytes, 8-byte aligned; params_ptr:
    n * 8 float32; info_ptr: n * 4 uint32; inliers_ptr: n * W * H bytes."""
    fmt = _flow_format(flow_dtype)
    its, thr = _fit_args(iterations, threshold)
    _check(lib().dis_flow_fit_homography(flow_ptr, fmt, mask_ptr or None, n, width, height, its, thr, params_ptr,
                                         info_ptr or None, inliers_ptr or None, workspace_ptr or None, MEM_DEVICE,
                                         stream or None, device))


def homography_to_flow(params: np.ndarray, width: int, height: int, out_dtype=np.float32,
                       device: int = 0) -> np.ndarray:
    """The flow field of homographies (dis_homography_to_flow) on the GPU: params
    float32 (8,) -> (H, W, 2), or (n, 8) -> (n, H, W, 2), as out_dtype (float32
    or float16). A model with a parameter that is not finite gives a NaN field,
    a pixel behind the model's horizon (1 + p6 x + p7 y <= 0) a NaN vector; with
    p6 = p7 = 0 the field is motion_to_flow's of p0..p5 bit for bit."""
    p = _models8(params)
    o_fmt = _flow_format(out_dtype)
    W, H = _sides(width, height)
    n = p.shape[0] if p.ndim == 2 else 1
    out = np.empty(p.shape[:-1] + (H, W, 2), _FLOW_DTYPES[o_fmt])
    _check(lib().dis_homography_to_flow(_ptr(p), n, W, H, _ptr(out), o_fmt, MEM_HOST, None, device))
    return out


def homography_to_flow_device(params_ptr: int, n: int, width: int, height: int, out_ptr: int, out_dtype=np.float32,
                              stream: int = 0, device: int = 0) -> None:
    """dis_homography_to_flow on raw device pointers, asynchronous on `stream`."""
    o_fmt = _flow_format(out_dtype)
    _check(lib().dis_homography_to_flow(params_ptr, n, width, height, out_ptr, o_fmt, MEM_DEVICE, stream or None,
                                        device))


def stabilize_path_homography(pair_params, width: int, height: int, radius: int, sigma=None, zoom: float = 1.0,
                              with_status: bool = False):
    """stabilize_path for homographies (dis_homography_stabilize, host only):
    float32 (N-1, 8) pair models (fit_homography's params) -> float32 (N, 8)
    corrections, what warp_homography takes. The path is a product of 3 x 3
    matrices kept at bottom-right 1 and smoothed entry by entry. Affine inputs
    (p6 = p7 = 0) give affine corrections. with_status as for stabilize_path."""
    r, s, z = _stabilize_args(radius, sigma, zoom)
    p = np.asarray(pair_params)
    if p.dtype != np.float32:
        raise ValueError(f"pair_params dtype must be float32, not {p.dtype}")
    if p.ndim != 2 or p.shape[1] != 8:
        raise ValueError(f"pair_params must be (N-1, 8), not {p.shape}")
    W, H = _sides(width, height)
    p = np.ascontiguousarray(p)
    n = p.shape[0] + 1
    out = np.empty((n, 8), np.float32)
    status = np.empty(n, np.uint8)
    replaced = ctypes.c_int(0)
    _check(lib().dis_homography_stabilize(_ptr(p) if n > 1 else None, n, W, H, r, s, z, _ptr(out), _ptr(status),
                                          ctypes.byref(replaced)))
    return (out, status, int(replaced.value)) if with_status else out


def warp_homography(image: np.ndarray, params: np.ndarray, border="replicate", return_valid: bool = False,
                    device: int = 0):
    """Backward warp (dis_warp_homography_u8) of u8 images by homographies on the
    GPU: bit for bit flow_warp(image, homography_to_flow(params, W, H)), without
    the field. image: (H, W) or (H, W, C) with params float32 (8,), or (n, H, W)
    or (n, H, W, C) with params (n, 8); C in 1, 3, 4. border, return_valid and
    non-finite models as for warp_motion; a pixel behind the horizon gets 0 and
    valid 0."""
    bd = _border(border)
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError(f"image dtype must be uint8, not {img.dtype}")
    p = _models8(params)
    if p.ndim == 1:
        if img.ndim not in (2, 3):
            raise ValueError("one model takes an (H, W) or (H, W, C) image")
        shape4 = (1,) + img.shape + ((1,) if img.ndim == 2 else ())
    else:
        if img.ndim not in (3, 4):
            raise ValueError("(n, 8) models take (n, H, W) or (n, H, W, C) images")
        shape4 = img.shape + ((1,) if img.ndim == 3 else ())
        if shape4[0] != p.shape[0]:
            raise ValueError(f"image shape {img.shape} does not match params shape {p.shape}")
    n, H, W, C = shape4
    if C not in (1, 3, 4):
        raise ValueError(f"image must have 1, 3 or 4 channels, not {C}")
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"image shape {img.shape} has an empty dimension")
    img = np.ascontiguousarray(img)
    out = np.empty(img.shape, np.uint8)
    valid = np.empty(shape4[:3] if p.ndim == 2 else shape4[1:3], np.uint8) if return_valid else None
    _check(lib().dis_warp_homography_u8(_ptr(img), 0, 0, C, _ptr(p), n, W, H, bd, _ptr(out),
                                        _ptr(valid) if return_valid else None, MEM_HOST, None, device))
    return (out, valid) if return_valid else out


def warp_homography_device(src_ptr: int, params_ptr: int, n: int, width: int, height: int, channels: int,
                           dst_ptr: int, valid_ptr: int = 0, border="replicate", src_stride: int = 0,
                           src_image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_warp_homography_u8 on raw device pointers (params_ptr: n * 8 float32 in
    device memory), asynchronous on `stream`: one launch, no allocation, no
    synchronisation."""
    bd = _border(border)
    _check(lib().dis_warp_homography_u8(src_ptr, src_stride, src_image_stride, channels, params_ptr, n, width, height,
                                        bd, dst_ptr, valid_ptr or None, MEM_DEVICE, stream or None, device))


DENOISE_MAX_NEIGHBOURS = 8


def denoise_weights(sigma: float) -> np.ndarray:
    """The Gaussian weight table of temporal_denoise (dis_denoise_weights, host
    only): float32 (256,), table[d] = exp(-d^2 / (2 sigma^2)) computed in double
    and rounded once; d is the mean absolute difference over a pixel's window."""
    table = np.empty(256, np.float32)
    _check(lib().dis_denoise_weights(float(sigma), _ptr(table)))
    return table


def _denoise_table(sigma, weights) -> np.ndarray:
    if (sigma is None) == (weights is None):
        raise ValueError("give exactly one of sigma and weights")
    if weights is None:
        return denoise_weights(sigma)
    w = np.asarray(weights)
    if w.dtype != np.float32 or w.shape != (256,):
        raise ValueError(f"weights must be float32 (256,), not {w.dtype} {w.shape}")
    return np.ascontiguousarray(w)


def _pointer_array(ptrs, count: int, name: str, optional: bool = False):
    """A host array of `count` pointers for the C-ABI (None / 0 entries are null)."""
    ptrs = list(ptrs)
    if len(ptrs) != count:
        raise ValueError(f"{name} must have {count} entries, not {len(ptrs)}")
    if not optional and any(not p for p in ptrs):
        raise ValueError(f"{name} must not hold a null pointer")
    return (ctypes.c_void_p * count)(*[int(p) if p else None for p in ptrs])


def temporal_denoise(cur: np.ndarray, neighbours, flows, sigma=None, weights=None, masks=None,
                     return_support: bool = False, device: int = 0):
    """Motion-compensated temporal denoising (dis_temporal_denoise_u8) on the GPU:
    each of the K (1..8) neighbours is warped to cur by its flow (flow_warp,
    scale 1, "replicate") and blended in with weights[d], d the mean absolute
    difference to cur over the pixel's 3 x 3 window and all channels:
    out = cur + sum_k w_k (warped_k - cur) / (1 + sum_k w_k). cur and every
    neighbour: u8 images of one shape, flow_warp's layouts; flows: K float32 or
    float16 (..., H, W, 2) fields of one dtype and shape, cur -> neighbour k.
    Give sigma (the table denoise_weights(sigma); about 1.5 times the noise's
    standard deviation) or weights (float32 (256,) in [0, 1]). masks: None, or K
    entries, each None or a u8 (..., H, W) plane whose zeros switch vectors off
    (e.g. a consistency mask). Returns the denoised array in cur's shape;
    return_support: also the u8 map (..., H, W) of how many neighbours took part."""
    table = _denoise_table(sigma, weights)
    img = np.asarray(cur)
    nbs, fls = list(neighbours), list(flows)
    K = len(nbs)
    if not 1 <= K <= DENOISE_MAX_NEIGHBOURS:
        raise ValueError(f"there must be 1 to {DENOISE_MAX_NEIGHBOURS} neighbours, not {K}")
    if len(fls) != K or (masks is not None and len(masks) != K):
        raise ValueError("neighbours, flows and masks must have one length")
    fls = [np.asarray(f) for f in fls]
    fl = fls[0]
    fmt = _flow_format(fl.dtype)
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError("flows must be (H, W, 2) or (n, H, W, 2)")
    if any(f.dtype != fl.dtype or f.shape != fl.shape for f in fls):
        raise ValueError("flows must have one dtype and one shape")
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    if img.dtype != np.uint8:
        raise ValueError(f"image dtype must be uint8, not {img.dtype}")
    if img.ndim == 2:
        shape4 = (1,) + img.shape + (1,)
    elif img.ndim == 3:
        shape4 = (1,) + img.shape if img.shape[:2] == (H, W) else img.shape + (1,)
    elif img.ndim == 4:
        shape4 = img.shape
    else:
        raise ValueError("images must be (H, W), (H, W, C), (n, H, W) or (n, H, W, C)")
    if shape4[:3] != (n, H, W):
        raise ValueError(f"image shape {img.shape} does not match flow shape {fl.shape}")
    C = shape4[3]
    if C not in (1, 3, 4):
        raise ValueError(f"images must have 1, 3 or 4 channels, not {C}")
    nbs = [np.asarray(a) for a in nbs]
    if any(a.dtype != np.uint8 or a.shape != img.shape for a in nbs):
        raise ValueError(f"every neighbour must be uint8 of cur's shape {img.shape}")
    mks = [None] * K if masks is None else [None if m is None else _byte_plane(m, fl.shape[:-1], "mask") for m in masks]
    img = np.ascontiguousarray(img)
    nbs = [np.ascontiguousarray(a) for a in nbs]
    fls = [np.ascontiguousarray(f) for f in fls]
    out = np.empty(img.shape, np.uint8)
    support = np.empty(fl.shape[:-1], np.uint8) if return_support else None
    _check(lib().dis_temporal_denoise_u8(
        _ptr(img), _pointer_array([_ptr(a) for a in nbs], K, "neighbours"), 0, 0, C,
        _pointer_array([_ptr(f) for f in fls], K, "flows"), fmt,
        None if masks is None else _pointer_array([None if m is None else _ptr(m) for m in mks], K, "masks", True),
        K, n, W, H, _ptr(table), _ptr(out), _ptr(support) if return_support else None, MEM_HOST, None, device))
    return (out, support) if return_support else out


def temporal_denoise_device(cur_ptr: int, neighbour_ptrs, flow_ptrs, flow_dtype, n: int, width: int, height: int,
                            channels: int, dst_ptr: int, sigma=None, weights=None, mask_ptrs=None, support_ptr: int = 0,
                            stride: int = 0, image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_temporal_denoise_u8 on raw device pointers, asynchronous on `stream`:
    neighbour_ptrs and flow_ptrs are sequences of K device pointers, mask_ptrs
    None or K entries (0 / None: no mask for that neighbour); the weight table
    (sigma or weights, as temporal_denoise's) is host memory."""
    table = _denoise_table(sigma, weights)
    fmt = _flow_format(flow_dtype)
    neighbour_ptrs = list(neighbour_ptrs)
    K = len(neighbour_ptrs)
    nbs = _pointer_array(neighbour_ptrs, K, "neighbour_ptrs", True)  # (a null entry is the library's to refuse)
    fls = _pointer_array(flow_ptrs, K, "flow_ptrs", True)
    mks = None if mask_ptrs is None else _pointer_array(mask_ptrs, K, "mask_ptrs", True)
    _check(lib().dis_temporal_denoise_u8(cur_ptr, nbs, stride, image_stride, channels, fls, fmt, mks, K, n, width, height,
                                         _ptr(table), dst_ptr, support_ptr or None, MEM_DEVICE, stream or None, device))


def advect_points(points: np.ndarray, flow: np.ndarray, with_status: bool = False, device: int = 0):
    """Points moved by flow fields (dis_flow_advect_points) on the GPU. flow:
    float32 or float16 (H, W, 2) with points (count, 2), or (n, H, W, 2) with
    (n, count, 2): (x, y) pairs, converted to float32. A point inside
    [0, W-1] x [0, H-1] whose four taps are valid vectors moves by the field
    sampled bilinearly there; any other point comes back unchanged. Returns the
    float32 points in the given shape; with_status: also the u8 (..., count),
    255 for a point that moved."""
    fl = np.asarray(flow)
    fmt = _flow_format(fl.dtype)
    if fl.ndim not in (3, 4) or fl.shape[-1] != 2:
        raise ValueError("flow must be (H, W, 2) or (n, H, W, 2)")
    pts = np.asarray(points)
    if pts.dtype.kind not in "fiu":
        raise ValueError(f"points must be numbers, not {pts.dtype}")
    if pts.ndim != fl.ndim - 1 or pts.shape[-1] != 2 or pts.shape[-2] < 1 or (fl.ndim == 4 and pts.shape[0] != fl.shape[0]):
        raise ValueError(f"points must be (count, 2) for one field or (n, count, 2) for n, not {pts.shape} "
                         f"with flow {fl.shape}")
    H, W = fl.shape[-3], fl.shape[-2]
    n = fl.shape[0] if fl.ndim == 4 else 1
    fl = np.ascontiguousarray(fl)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    out = np.empty(pts.shape, np.float32)
    status = np.empty(pts.shape[:-1], np.uint8) if with_status else None
    _check(lib().dis_flow_advect_points(_ptr(fl), fmt, n, W, H, _ptr(pts), pts.shape[-2], _ptr(out),
                                        _ptr(status) if with_status else None, MEM_HOST, None, device))
    return (out, status) if with_status else out


def advect_points_device(flow_ptr: int, flow_dtype, n: int, width: int, height: int, points_ptr: int, count: int,
                         points_out_ptr: int, status_ptr: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_flow_advect_points on raw device pointers, asynchronous on `stream`;
    points_out_ptr may be points_ptr."""
    fmt = _flow_format(flow_dtype)
    _check(lib().dis_flow_advect_points(flow_ptr, fmt, n, width, height, points_ptr, count, points_out_ptr,
                                        status_ptr or None, MEM_DEVICE, stream or None, device))


def frames_to_gray(frames: np.ndarray, frame_format, device: int = 0) -> np.ndarray:
    """dis_frames_to_gray_u8 on a host array: u8 (H, W, C) or (n, H, W, C) frames
    of `frame_format` ("bgr", "rgb", "bgra", "rgba"; "gray" takes (H, W) or
    (n, H, W) and copies) -> u8 gray (H, W) / (n, H, W) on the GPU, by
    (R*4899 + G*9617 + B*1868 + 8192) >> 14 (alpha ignored): the very conversion
    an engine made with that frame_format applies to its input."""
    fmt = _frame_format(frame_format)
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        raise ValueError(f"frames dtype must be uint8, not {a.dtype}")
    C = _FRAME_CHANNELS[fmt]
    if fmt == FRAME_GRAY8:
        if a.ndim not in (2, 3):
            raise ValueError(f"gray frames must be (H, W) or (n, H, W), not {a.shape}")
        shape3 = a.shape if a.ndim == 3 else (1,) + a.shape
    else:
        if a.ndim not in (3, 4) or a.shape[-1] != C:
            raise ValueError(f"{frame_format!r} frames must be (H, W, {C}) or (n, H, W, {C}), not {a.shape}")
        shape3 = a.shape[:-1] if a.ndim == 4 else (1,) + a.shape[:-1]
    n, H, W = shape3
    a = np.ascontiguousarray(a)
    out = np.empty(shape3, np.uint8)
    _check(lib().dis_frames_to_gray_u8(_ptr(a), 0, 0, fmt, n, W, H, _ptr(out), 0, 0, MEM_HOST, None, device))
    single = a.ndim == (2 if fmt == FRAME_GRAY8 else 3)
    return out[0] if single else out


def frames_to_gray_device(src_ptr: int, frame_format, n: int, width: int, height: int, dst_ptr: int,
                          src_stride: int = 0, src_image_stride: int = 0, dst_stride: int = 0,
                          dst_image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_frames_to_gray_u8 on raw device pointers (strides in bytes, 0 = tight),
    asynchronous on `stream`."""
    fmt = _frame_format(frame_format)
    _check(lib().dis_frames_to_gray_u8(src_ptr, src_stride, src_image_stride, fmt, n, width, height, dst_ptr,
                                       dst_stride, dst_image_stride, MEM_DEVICE, stream or None, device))


def _yuv_args(frame_format, matrix, range, alpha=255):
    """(dis_frame_format, dis_yuv_matrix, dis_yuv_range, alpha) of the names (or
    the enums' own values); ValueError for anything else."""
    fmt = _frame_format(frame_format)
    if isinstance(matrix, bool) or matrix not in _YUV_MATRICES:
        raise ValueError(f"matrix must be 'bt601' or 'bt709', not {matrix!r}")
    if isinstance(range, bool) or range not in _YUV_RANGES:
        raise ValueError(f"range must be 'limited' or 'full', not {range!r}")
    if not isinstance(alpha, (int, np.integer)) or isinstance(alpha, bool) or not 0 <= alpha <= 255:
        raise ValueError(f"alpha must be an integer in [0, 255], not {alpha!r}")
    return fmt, _YUV_MATRICES[matrix], _YUV_RANGES[range], int(alpha)


def _surface(buf):
    """A host 4:2:0 surface buffer, u8 (n, H*3//2, W) or (H*3//2, W) (NV12: the Y
    plane, then H/2 rows of Cb/Cr pairs; I420: the Y plane, the Cb plane, the Cr
    plane) -> (contiguous (n, H*3//2, W) array, single, n, W, H)."""
    a = np.asarray(buf)
    if a.dtype != np.uint8:
        raise ValueError(f"surface dtype must be uint8, not {a.dtype}")
    if a.ndim not in (2, 3):
        raise ValueError(f"a 4:2:0 surface buffer must be (H*3//2, W) or (n, H*3//2, W), not {a.shape}")
    rows, W = a.shape[-2:]
    H = rows * 2 // 3
    if rows < 3 or rows % 3 or H % 2 or W < 2 or W % 2:
        raise ValueError(f"a 4:2:0 surface buffer has H*3//2 rows of W bytes with even W and H, not {a.shape}")
    single = a.ndim == 2
    a = np.ascontiguousarray(a[None] if single else a)
    if a.shape[0] < 1:
        raise ValueError("no surface")
    return a, single, a.shape[0], W, H


def _packed(frames, fmt):
    """Host frames of dis_frame_format fmt with even sides -> (contiguous
    (n, H, W[, C]) array, single, n, W, H)."""
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        raise ValueError(f"frames dtype must be uint8, not {a.dtype}")
    C = _FRAME_CHANNELS[fmt]
    lead = a.ndim - (1 if C > 1 else 0)
    if lead not in (2, 3) or (C > 1 and a.shape[-1] != C):
        what = "(H, W) or (n, H, W)" if C == 1 else f"(H, W, {C}) or (n, H, W, {C})"
        raise ValueError(f"frames of this format must be {what}, not {a.shape}")
    single = lead == 2
    a = np.ascontiguousarray(a[None] if single else a)
    n, H, W = a.shape[:3]
    if n < 1 or H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 needs even sides, not {W} x {H}")
    return a, single, n, W, H


def _surface_planes(base, W, H, interleaved, swap):
    """(cb, cr, c_step, c_stride) of a tight one-buffer surface at `base`: NV12 /
    NV21 (interleaved) or I420 / YV12; swap: the Cr sample (plane) comes first."""
    c0 = base + W * H
    c1 = c0 + (1 if interleaved else (W // 2) * (H // 2))
    cb, cr = (c1, c0) if swap else (c0, c1)
    return cb, cr, (2 if interleaved else 1), (W if interleaved else W // 2)


def _surface_to_frames(buf, frame_format, matrix, range, alpha, device, interleaved):
    fmt, mat, rng, alpha = _yuv_args(frame_format, matrix, range, alpha)
    a, single, n, W, H = _surface(buf)
    C = _FRAME_CHANNELS[fmt]
    out = np.empty((n, H, W) + ((C,) if C > 1 else ()), np.uint8)
    cb, cr, step, cst = _surface_planes(_ptr(a), W, H, interleaved, False)
    img = W * H * 3 // 2
    _check(lib().dis_yuv420_to_frames_u8(_ptr(a), W, img, cb, cr, cst, img, step, mat, rng, n, W, H, _ptr(out), 0, 0,
                                         fmt, alpha, MEM_HOST, None, device))
    return out[0] if single else out


def _frames_to_surface(frames, frame_format, matrix, range, device, interleaved):
    fmt, mat, rng, _ = _yuv_args(frame_format, matrix, range)
    a, single, n, W, H = _packed(frames, fmt)
    out = np.empty((n, H * 3 // 2, W), np.uint8)
    cb, cr, step, cst = _surface_planes(_ptr(out), W, H, interleaved, False)
    img = W * H * 3 // 2
    _check(lib().dis_frames_to_yuv420_u8(_ptr(a), 0, 0, fmt, mat, rng, n, W, H, _ptr(out), W, img, cb, cr, cst, img,
                                         step, MEM_HOST, None, device))
    return out[0] if single else out


def nv12_to_frames(buf: np.ndarray, frame_format, matrix="bt601", range="limited", alpha: int = 255,
                   device: int = 0) -> np.ndarray:
    """dis_yuv420_to_frames_u8 on host NV12 surfaces: u8 (H*3//2, W) or
    (n, H*3//2, W), the Y plane followed by H/2 rows of Cb/Cr pairs -> frames of
    `frame_format` ((..., H, W, C), "gray": (..., H, W)) on the GPU, by the exact
    integer arithmetic of include/dis_abi.h (nearest chroma). matrix "bt601" /
    "bt709", range "limited" / "full"; alpha fills the fourth sample."""
    return _surface_to_frames(buf, frame_format, matrix, range, alpha, device, True)


def i420_to_frames(buf: np.ndarray, frame_format, matrix="bt601", range="limited", alpha: int = 255,
                   device: int = 0) -> np.ndarray:
    """As nv12_to_frames for I420 surfaces: the Y plane, then the W/2 x H/2 Cb
    plane, then the Cr plane, each tight, in H*3//2 rows of W bytes."""
    return _surface_to_frames(buf, frame_format, matrix, range, alpha, device, False)


def frames_to_nv12(frames: np.ndarray, frame_format, matrix="bt601", range="limited", device: int = 0) -> np.ndarray:
    """dis_frames_to_yuv420_u8 on host frames with even sides ((H, W, C) or
    (n, H, W, C); "gray": (H, W) or (n, H, W)) -> NV12 surfaces, u8 (H*3//2, W) /
    (n, H*3//2, W). Y per pixel, Cb and Cr from each 2 x 2 block's sums. With
    "bt601" and "full" the Y plane is frames_to_gray's image."""
    return _frames_to_surface(frames, frame_format, matrix, range, device, True)


def frames_to_i420(frames: np.ndarray, frame_format, matrix="bt601", range="limited", device: int = 0) -> np.ndarray:
    """As frames_to_nv12, to I420 surfaces (the Y, Cb and Cr planes in turn)."""
    return _frames_to_surface(frames, frame_format, matrix, range, device, False)


def nv12_luma(buf):
    """The Y planes of NV12 (or I420) surface buffers (H*3//2, W) / (n, H*3//2, W):
    a strided view (H, W) / (n, H, W), no copy -- numpy arrays and torch tensors
    alike. They are gray frames with row stride W and image stride W*H*3//2,
    which calc_device(..., stride, pair_stride) takes in place."""
    if len(buf.shape) not in (2, 3):
        raise ValueError(f"a 4:2:0 surface buffer must be (H*3//2, W) or (n, H*3//2, W), not {tuple(buf.shape)}")
    rows, W = buf.shape[-2:]
    H = rows * 2 // 3
    if rows < 3 or rows % 3 or H % 2 or W < 2 or W % 2:
        raise ValueError(f"a 4:2:0 surface buffer has H*3//2 rows of W bytes with even W and H, not {tuple(buf.shape)}")
    return buf[..., :H, :]


def yuv420_to_frames_device(y_ptr: int, cb_ptr: int, cr_ptr: int, c_step: int, n: int, width: int, height: int,
                            dst_ptr: int, frame_format, matrix="bt601", range="limited", alpha: int = 255,
                            y_stride: int = 0, y_image_stride: int = 0, c_stride: int = 0, c_image_stride: int = 0,
                            dst_stride: int = 0, dst_image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_yuv420_to_frames_u8 on raw device pointers (strides in bytes, 0 = tight),
    asynchronous on `stream`. NV12: cb_ptr = y_ptr + y_stride * height,
    cr_ptr = cb_ptr + 1, c_step = 2, c_stride = y_stride; I420: c_step = 1. With a
    "gray" target cb_ptr and cr_ptr may be 0."""
    fmt, mat, rng, alpha = _yuv_args(frame_format, matrix, range, alpha)
    _check(lib().dis_yuv420_to_frames_u8(y_ptr, y_stride, y_image_stride, cb_ptr or None, cr_ptr or None, c_stride,
                                         c_image_stride, c_step, mat, rng, n, width, height, dst_ptr, dst_stride,
                                         dst_image_stride, fmt, alpha, MEM_DEVICE, stream or None, device))


def frames_to_yuv420_device(src_ptr: int, frame_format, n: int, width: int, height: int, y_ptr: int, cb_ptr: int,
                            cr_ptr: int, c_step: int, matrix="bt601", range="limited", src_stride: int = 0,
                            src_image_stride: int = 0, y_stride: int = 0, y_image_stride: int = 0, c_stride: int = 0,
                            c_image_stride: int = 0, stream: int = 0, device: int = 0) -> None:
    """dis_frames_to_yuv420_u8 on raw device pointers (strides in bytes, 0 = tight),
    asynchronous on `stream`."""
    fmt, mat, rng, _ = _yuv_args(frame_format, matrix, range)
    _check(lib().dis_frames_to_yuv420_u8(src_ptr, src_stride, src_image_stride, fmt, mat, rng, n, width, height,
                                         y_ptr, y_stride, y_image_stride, cb_ptr or None, cr_ptr or None, c_stride,
                                         c_image_stride, c_step, MEM_DEVICE, stream or None, device))


def read_flo(path: str, channels: int = 2) -> np.ndarray:
    """Read a Middlebury .flo file (src/IO_flow.cpp:10-53) -> (H, W, channels) float32."""
    w, h = ctypes.c_int(), ctypes.c_int()
    _check(lib().dis_flo_info(os.fsencode(path), ctypes.byref(w), ctypes.byref(h)))
    out = np.empty((h.value, w.value, channels), np.float32)
    _check(lib().dis_read_flo(os.fsencode(path), _ptr(out), w.value, h.value, channels))
    return out


def write_flo(path: str, data: np.ndarray) -> None:
    """Write (H, W, channels) float32 as a .flo file (src/IO_flow.cpp:56-98)."""
    d = np.ascontiguousarray(data, dtype=np.float32)
    if d.ndim == 2:
        d = d[..., None]
    _check(lib().dis_write_flo(os.fsencode(path), _ptr(d), d.shape[1], d.shape[0], d.shape[2]))


def batch_stream_plan(nsub: int, nstages: int) -> list:
    """The fork / stage / join ops a batch call with nsub sub-batches issues
    (dis_batch_stream_plan): list of (kind, stream, event, stage)."""
    n = ctypes.c_int()
    _check(lib().dis_batch_stream_plan(nsub, nstages, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int * (4 * n.value))()
    _check(lib().dis_batch_stream_plan(nsub, nstages, buf, n.value, ctypes.byref(n)))
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def check_stream_plan(ops, nstreams: int, nevents: int) -> str | None:
    """None if the plan keeps the capture rules (dis_check_stream_plan), else
    the broken rule."""
    flat = [int(v) for op in ops for v in op]
    buf = (ctypes.c_int * max(1, len(flat)))(*flat)
    st = lib().dis_check_stream_plan(buf, len(ops), nstreams, nevents)
    return None if st == DIS_OK else lib().dis_last_error().decode()


def synth_pair(seed: int, width: int, height: int, with_gt: bool = False):
    """Deterministic synthetic u8 pair (and ground-truth flow) for seed."""
    I0 = np.empty((height, width), np.uint8)
    I1 = np.empty((height, width), np.uint8)
    gt = np.empty((height, width, 2), np.float32) if with_gt else None
    _check(lib().dis_synth_pair(seed, width, height, _ptr(I0), _ptr(I1), _ptr(gt) if with_gt else None))
    return (I0, I1, gt) if with_gt else (I0, I1)


class DenseInverseSearch:
    """One device context for W x H pairs (dis_create / dis_destroy)."""

    flow_dtype = np.dtype(np.float32)  # the engine's flow format (set_flow_format)
    frame_format = "gray"              # the engine's frame format (set_frame_format)
    _frame_channels = 1

    def __init__(self, params, width: int, height: int, max_batch: int = 1, device: int = 0,
                 flow_dtype=np.float32, frame_format="gray"):
        """flow_dtype: np.float32 (default) or np.float16 -- the format of every
        full-resolution flow the engine writes and reads (dis_set_flow_format).
        frame_format: "gray" (default), "bgr", "rgb", "bgra" or "rgba" -- what the
        frames of every calc call hold (dis_set_frame_format): H x W bytes, or
        H x W x 3 / 4 interleaved bytes that the engine reduces to gray itself."""
        self._ctx = ctypes.c_void_p()  # (close() works after a failed constructor)
        fmt = _flow_format(flow_dtype)  # raises before any device call
        ffmt = _frame_format(frame_format)
        if isinstance(params, (Preset, int)) and not isinstance(params, Params):
            params = preset_params(Preset(params), width, height)
        self.params = params
        self.width, self.height, self.max_batch = width, height, max_batch
        self.device = device
        _check(lib().dis_create(ctypes.byref(self._ctx), ctypes.byref(params._c()), width, height,
                                max_batch, device))
        if fmt != FLOW_F32:
            self.set_flow_format(flow_dtype)
        if ffmt != FRAME_GRAY8:
            self.set_frame_format(frame_format)

    def set_flow_format(self, flow_dtype) -> None:
        """dis_set_flow_format: np.float32 or np.float16 flows from the next call on."""
        fmt = _flow_format(flow_dtype)
        _check(lib().dis_set_flow_format(self._ctx, fmt))
        self.flow_dtype = _FLOW_DTYPES[fmt]

    def set_frame_format(self, frame_format) -> None:
        """dis_set_frame_format: "gray", "bgr", "rgb", "bgra" or "rgba" frames from the next call on."""
        fmt = _frame_format(frame_format)
        _check(lib().dis_set_frame_format(self._ctx, fmt))
        self.frame_format = next(k for k, v in _FRAME_FORMATS.items() if v == fmt)
        self._frame_channels = _FRAME_CHANNELS[fmt]

    def _frames(self, I0, I1):
        """The two frame batches of a calc call as contiguous u8 arrays, checked
        against the engine's size and frame format (before any library call):
        (n, H, W) gray, (n, H, W, C) colour -> (I0, I1, n, row bytes)."""
        I0 = np.ascontiguousarray(I0, dtype=np.uint8)
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        C = self._frame_channels
        want = (self.height, self.width) if C == 1 else (self.height, self.width, C)
        if I0.shape != I1.shape or I0.ndim != 1 + len(want) or I0.shape[1:] != want:
            raise DisError(DIS_ERR_INVALID_ARGUMENT,
                           f"frames must be {('n',) + want} for frame format {self.frame_format!r}, "
                           f"not {I0.shape} and {I1.shape}")
        return I0, I1, I0.shape[0], self.width * C

    def close(self) -> None:
        if self._ctx:
            lib().dis_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def init_plane_size(self):
        """(iw, ih) of one pair's init plane (dis_init_plane_size): half the
        padded frame's coarsest level, rounded up."""
        iw, ih = ctypes.c_int(), ctypes.c_int()
        _check(lib().dis_init_plane_size(self._ctx, ctypes.byref(iw), ctypes.byref(ih)))
        return iw.value, ih.value

    def _plane_shape(self):
        # the same size without a library call (shape checks raise before any)
        sf = 1 << self.params.coarsest_scale
        wc = (self.width + sf - 1) // sf
        hc = (self.height + sf - 1) // sf
        return (hc + 1) // 2, (wc + 1) // 2

    def _check_init(self, init, init_kind, n: int):
        """Validate an init array for n pairs -> (contiguous array, kind). A
        "fullres" init has the engine's flow dtype, a "coarse" one is float32
        (ValueError otherwise: a silent conversion would hide a format mix-up)."""
        if init_kind not in _INIT_KINDS or isinstance(init_kind, bool):
            raise DisError(DIS_ERR_INVALID_ARGUMENT, f"init_kind must be 'fullres' or 'coarse', not {init_kind!r}")
        kind = _INIT_KINDS[init_kind]
        want = self.flow_dtype if kind == INIT_FULLRES else np.dtype(np.float32)
        if self.flow_dtype != np.float32 or getattr(init, "dtype", None) == np.float16:
            if getattr(init, "dtype", None) != want:
                raise ValueError(f"init must be {want} for init_kind {init_kind!r} on a {self.flow_dtype} engine, "
                                 f"not {getattr(init, 'dtype', type(init).__name__)}")
        a = np.ascontiguousarray(init, dtype=want)
        hw = (self.height, self.width) if kind == INIT_FULLRES else self._plane_shape()
        if a.shape != (n,) + hw + (2,):
            raise DisError(DIS_ERR_INVALID_ARGUMENT,
                           f"init must be {(n,) + hw + (2,)} for init_kind {init_kind!r}, not {a.shape}")
        return a, kind

    def flow_to_init(self, flows: np.ndarray) -> np.ndarray:
        """Full-resolution (H, W, 2) or (n, H, W, 2) flows -> their init planes
        (ih, iw, 2) / (n, ih, iw, 2) (dis_flow_to_init: the reduction alone)."""
        if self.flow_dtype != np.float32 and getattr(flows, "dtype", None) != self.flow_dtype:
            raise ValueError(f"flows must be {self.flow_dtype} on a {self.flow_dtype} engine")
        f = np.ascontiguousarray(flows, dtype=self.flow_dtype)
        single = f.ndim == 3
        if single:
            f = f[None]
        if f.ndim != 4 or f.shape[1:] != (self.height, self.width, 2):
            raise DisError(DIS_ERR_INVALID_ARGUMENT, f"flows must be (n, {self.height}, {self.width}, 2)")
        out = np.empty((f.shape[0],) + self._plane_shape() + (2,), np.float32)
        _check(lib().dis_flow_to_init(self._ctx, f.shape[0], _ptr(f), _ptr(out), MEM_HOST, None))
        return out[0] if single else out

    def calc(self, I0: np.ndarray, I1: np.ndarray, init=None, init_kind="fullres") -> np.ndarray:
        """u8 H x W frames (host; H x W x C under a colour frame_format) -> H x W x 2
        flow (host) of the engine's
        flow_dtype (float32 unless the engine was made or set otherwise). init: the
        search's start, a full-resolution (H, W, 2) flow (init_kind "fullres",
        e.g. the previous pair's result) or an init plane (ih, iw, 2) ("coarse")."""
        return self.calc_batch(I0[None], I1[None], None if init is None else np.asarray(init)[None], init_kind)[0]

    def calc_batch(self, I0: np.ndarray, I1: np.ndarray, init=None, init_kind="fullres") -> np.ndarray:
        I0, I1, n, row = self._frames(I0, I1)
        if init is not None:
            init, kind = self._check_init(init, init_kind, n)
        flow = np.empty((n, self.height, self.width, 2), self.flow_dtype)
        if init is None:
            _check(lib().dis_calc_batch_u8(self._ctx, n, _ptr(I0), _ptr(I1), row,
                                           row * self.height, _ptr(flow), MEM_HOST, None))
        else:
            _check(lib().dis_calc_batch_init_u8(self._ctx, n, _ptr(I0), _ptr(I1), row,
                                                row * self.height, _ptr(init), kind, _ptr(flow),
                                                MEM_HOST, None))
        return flow

    def calc_device(self, n: int, I0_ptr: int, I1_ptr: int, flow_ptr: int, stream: int = 0,
                    stride: int = 0, pair_stride: int = 0, init_ptr: int = 0, init_kind="fullres") -> None:
        """Asynchronous calc on device-resident buffers (raw device pointers).
        init_ptr: n full-resolution flows ("fullres"; may be flow_ptr itself) or
        n init planes ("coarse") to start the search from."""
        if not init_ptr:
            _check(lib().dis_calc_batch_u8(self._ctx, n, I0_ptr, I1_ptr, stride, pair_stride, flow_ptr,
                                           MEM_DEVICE, stream or None))
            return
        if init_kind not in _INIT_KINDS or isinstance(init_kind, bool):
            raise DisError(DIS_ERR_INVALID_ARGUMENT, f"init_kind must be 'fullres' or 'coarse', not {init_kind!r}")
        _check(lib().dis_calc_batch_init_u8(self._ctx, n, I0_ptr, I1_ptr, stride, pair_stride, init_ptr,
                                            _INIT_KINDS[init_kind], flow_ptr, MEM_DEVICE, stream or None))

    def flow_to_init_device(self, n: int, flow_ptr: int, planes_ptr: int, stream: int = 0) -> None:
        """dis_flow_to_init on raw device pointers, asynchronous on `stream`."""
        _check(lib().dis_flow_to_init(self._ctx, n, flow_ptr, planes_ptr, MEM_DEVICE, stream or None))

    def track(self, frames, accumulate: bool = False):
        """Generator over an iterable of u8 H x W frames: yields the flow of
        each consecutive pair, warm-started from the flow of the pair before
        (the first pair is cold). accumulate=True yields (flow_k, acc_k,
        valid_k) instead: acc_k is the float32 flow from the first frame to the
        pair's second frame and valid_k its u8 map. acc_1 is the first pair's
        flow (valid_1 all 255); after that acc_k, valid_k =
        flow_compose(acc_{k-1}, flow_k, valid_a=valid_{k-1}), with flow_k in the
        engine's flow_dtype as it is."""
        prev_frame, prev_flow = None, None
        acc, valid = None, None
        for f in frames:
            if prev_frame is not None:
                prev_flow = self.calc(prev_frame, f, init=prev_flow)
                if not accumulate:
                    yield prev_flow
                else:
                    if acc is None:
                        acc = prev_flow.astype(np.float32)  # (exact for float16; a copy for float32)
                        valid = np.full(prev_flow.shape[:-1], 255, np.uint8)
                    else:
                        acc, valid = flow_compose(acc, prev_flow, valid_a=valid, with_valid=True, device=self.device)
                    yield prev_flow, acc, valid
            prev_frame = f

    def calc_bidir(self, I0: np.ndarray, I1: np.ndarray):
        """u8 H x W frames (host) -> (flow I0->I1, flow I1->I0), one pyramid."""
        fw, bw = self.calc_bidir_batch(I0[None], I1[None])
        return fw[0], bw[0]

    def calc_bidir_batch(self, I0: np.ndarray, I1: np.ndarray, consistency: bool = False,
                         alpha1: float = 0.01, alpha2: float = 0.5):
        """dis_calc_bidir_batch_u8 on host frames: (fw, bw), bit-equal to
        calc_batch(I0, I1) and calc_batch(I1, I0). consistency=True also returns
        (mask_fw, mask_bw): flow_consistency(fw, bw) and flow_consistency(bw, fw)."""
        I0, I1, n, row = self._frames(I0, I1)
        fw = np.empty((n, self.height, self.width, 2), self.flow_dtype)
        bw = np.empty((n, self.height, self.width, 2), self.flow_dtype)
        _check(lib().dis_calc_bidir_batch_u8(self._ctx, n, _ptr(I0), _ptr(I1), row,
                                             row * self.height, _ptr(fw), _ptr(bw), MEM_HOST, None))
        if not consistency:
            return fw, bw
        # (the check is f32-only: a float16 engine's masks come from the returned flows widened)
        wfw, wbw = fw, bw
        if self.flow_dtype != np.float32:
            wfw, wbw = flow_convert(fw, np.float32, self.device), flow_convert(bw, np.float32, self.device)
        return (fw, bw, flow_consistency(wfw, wbw, alpha1, alpha2, device=self.device),
                flow_consistency(wbw, wfw, alpha1, alpha2, device=self.device))

    def calc_filled(self, I0: np.ndarray, I1: np.ndarray, alpha1: float = 0.01, alpha2: float = 0.5,
                    with_level: bool = False):
        """u8 H x W frames (host) -> the forward flow with every vector that fails
        the forward-backward check replaced by push-pull from those that pass
        (calc_filled_batch on one pair); with_level: (flow, level)."""
        r = self.calc_filled_batch(I0[None], I1[None], alpha1, alpha2, with_level)
        return (r[0][0], r[1][0]) if with_level else r[0]

    def calc_filled_batch(self, I0: np.ndarray, I1: np.ndarray, alpha1: float = 0.01, alpha2: float = 0.5,
                          with_level: bool = False):
        """One calc_bidir_batch with its forward consistency mask, then
        flow_fill(fw, mask) in the engine's flow_dtype: a dense forward flow
        without occluded or inconsistent vectors. with_level: (flows, levels),
        levels as flow_fill's."""
        fw, _, mask, _ = self.calc_bidir_batch(I0, I1, consistency=True, alpha1=alpha1, alpha2=alpha2)
        return flow_fill(fw, mask, out_dtype=self.flow_dtype, with_level=with_level, device=self.device)

    def interpolate(self, I0: np.ndarray, I1: np.ndarray, ts, return_fill: bool = False):
        """The frames between u8 H x W frames I0 and I1 at every time of `ts`
        (each in [0, 1]): one calc_bidir, then one flow_interp per time with both
        flows in the engine's flow_dtype as they are (no conversion). Returns the
        list of frames; return_fill: the list of (frame, fill) pairs. On an engine
        with a colour frame_format I0 and I1 are H x W x C: the flows come from
        them, the same frames are interpolated, and the result is H x W x C."""
        ts = [_interp_time(t) for t in ts]  # raises before any device call
        fw, bw = self.calc_bidir(I0, I1)
        return [flow_interp(I0, I1, fw, t, bw=bw, return_fill=return_fill, device=self.device) for t in ts]

    def denoise(self, frames, radius: int = 1, sigma: float = None, weights=None) -> np.ndarray:
        """A sequence of T u8 frames (H x W; H x W x C on an engine with a colour
        frame_format) denoised in time: for frame t the flows to the up to
        2 * radius frames t - radius .. t + radius that exist (ascending, without
        t; end frames have fewer) come from calc_batch, max_batch pairs a call
        over the whole sequence, in the engine's flow_dtype as they are; then one
        temporal_denoise(frame t, those frames, those flows, sigma or weights)
        per frame, without masks. Returns the T denoised frames as one array; a
        frame without a neighbour (T == 1) is returned as it is."""
        table = _denoise_table(sigma, weights)  # raises before any device call
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or \
                not 1 <= radius <= DENOISE_MAX_NEIGHBOURS // 2:
            raise ValueError(f"radius must be an integer in [1, {DENOISE_MAX_NEIGHBOURS // 2}], not {radius!r}")
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        fr, _, T, _ = self._frames(fr, fr)
        pairs = [(t, j) for t in range(T) for j in range(max(t - radius, 0), min(t + radius, T - 1) + 1) if j != t]
        flows = []
        for b in range(0, len(pairs), self.max_batch):
            chunk = pairs[b:b + self.max_batch]
            flows.extend(self.calc_batch(fr[[t for t, _ in chunk]], fr[[j for _, j in chunk]]))
        out = np.empty_like(fr)
        for t in range(T):
            mine = [i for i, (a, _) in enumerate(pairs) if a == t]
            if not mine:
                out[t] = fr[t]
                continue
            out[t] = temporal_denoise(fr[t], [fr[pairs[i][1]] for i in mine], [flows[i] for i in mine],
                                      weights=table, device=self.device)
        return out

    def stabilize(self, frames, model="similarity", radius: int = 15, sigma=None, zoom: float = 1.0,
                  iterations: int = 3, threshold: float = 1.0, border="replicate", return_models: bool = False):
        """A sequence of N u8 frames (H x W; H x W x C on an engine with a colour
        frame_format) steadied: the flows of the N - 1 consecutive pairs (calc on
        device buffers, max_batch pairs a call, in the engine's flow_dtype as they
        are), fit_motion(model, iterations, threshold) of each on the device,
        stabilize_path(radius, sigma, zoom) of the (N - 1, 6) models on the host
        -- the only numbers that leave the device before the result -- and one
        warp_motion(border) of the frames as given by the corrections. Returns
        the N stabilised frames as one array; return_models: (frames, pair models
        (N - 1, 6), corrections (N, 6)). The device buffers are torch tensors on
        the engine's device, on the null stream."""
        mdl, its, thr = _motion_args(model, iterations, threshold)  # all raise before any device call
        _stabilize_args(radius, sigma, zoom)
        bd = _border(border)
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        fr, _, N, row = self._frames(fr, fr)
        import torch

        W, H, C = self.width, self.height, self._frame_channels
        dev = torch.device("cuda", self.device)
        dfr = torch.from_numpy(fr if fr.flags.writeable else fr.copy()).to(dev)  # (torch wants a writable source)
        pair = np.empty((N - 1, 6), np.float32)
        if N > 1:
            nb = min(self.max_batch, N - 1)
            dflow = torch.empty((nb, H, W, 2), dtype=torch.float16 if self.flow_dtype == np.float16 else torch.float32,
                                device=dev)
            dpar = torch.empty((N - 1, 6), dtype=torch.float32, device=dev)
            dws = torch.empty(fit_motion_workspace(nb, W, H) // 8, dtype=torch.float64, device=dev)
            for k in range(0, N - 1, nb):
                b = min(nb, N - 1 - k)
                self.calc_device(b, dfr[k].data_ptr(), dfr[k + 1].data_ptr(), dflow.data_ptr(), stride=row,
                                 pair_stride=row * H)
                fit_motion_device(dflow.data_ptr(), self.flow_dtype, b, W, H, dpar[k].data_ptr(), dws.data_ptr(),
                                  model=mdl, iterations=its, threshold=thr, device=self.device)
            pair = dpar.cpu().numpy()
        corr = stabilize_path(pair, W, H, radius, sigma, zoom)
        dcorr = torch.from_numpy(corr).to(dev)
        dout = torch.empty_like(dfr)
        warp_motion_device(dfr.data_ptr(), dcorr.data_ptr(), N, W, H, C, dout.data_ptr(), border=bd,
                           device=self.device)
        out = dout.cpu().numpy()
        return (out, pair, corr) if return_models else out

    def stabilize_homography(self, frames, radius: int = 15, sigma=None, zoom: float = 1.0, iterations: int = 3,
                             threshold: float = 1.0, border="replicate", return_models: bool = False):
        """stabilize with the eight-parameter model, for a camera that rotates:
        the same chain with fit_homography, stabilize_path_homography and
        warp_homography in the places of fit_motion, stabilize_path and
        warp_motion. return_models: (frames, pair models (N - 1, 8), corrections
        (N, 8))."""
        its, thr = _fit_args(iterations, threshold)  # all raise before any device call
        _stabilize_args(radius, sigma, zoom)
        bd = _border(border)
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        fr, _, N, row = self._frames(fr, fr)
        import torch

        W, H, C = self.width, self.height, self._frame_channels
        dev = torch.device("cuda", self.device)
        dfr = torch.from_numpy(fr if fr.flags.writeable else fr.copy()).to(dev)  # (torch wants a writable source)
        pair = np.empty((N - 1, 8), np.float32)
        if N > 1:
            nb = min(self.max_batch, N - 1)
            dflow = torch.empty((nb, H, W, 2), dtype=torch.float16 if self.flow_dtype == np.float16 else torch.float32,
                                device=dev)
            dpar = torch.empty((N - 1, 8), dtype=torch.float32, device=dev)
            dws = torch.empty(fit_homography_workspace(nb, W, H) // 8, dtype=torch.float64, device=dev)
            for k in range(0, N - 1, nb):
                b = min(nb, N - 1 - k)
                self.calc_device(b, dfr[k].data_ptr(), dfr[k + 1].data_ptr(), dflow.data_ptr(), stride=row,
                                 pair_stride=row * H)
                fit_homography_device(dflow.data_ptr(), self.flow_dtype, b, W, H, dpar[k].data_ptr(), dws.data_ptr(),
                                      iterations=its, threshold=thr, device=self.device)
            pair = dpar.cpu().numpy()
        corr = stabilize_path_homography(pair, W, H, radius, sigma, zoom)
        dcorr = torch.from_numpy(corr).to(dev)
        dout = torch.empty_like(dfr)
        warp_homography_device(dfr.data_ptr(), dcorr.data_ptr(), N, W, H, C, dout.data_ptr(), border=bd,
                               device=self.device)
        out = dout.cpu().numpy()
        return (out, pair, corr) if return_models else out

    def calc_bidir_device(self, n: int, I0_ptr: int, I1_ptr: int, fw_ptr: int, bw_ptr: int, stream: int = 0,
                          stride: int = 0, pair_stride: int = 0) -> None:
        """Asynchronous bidirectional calc on device-resident buffers (raw device pointers)."""
        _check(lib().dis_calc_bidir_batch_u8(self._ctx, n, I0_ptr, I1_ptr, stride, pair_stride, fw_ptr, bw_ptr,
                                             MEM_DEVICE, stream or None))

    def set_host_pipeline(self, chunk_pairs: int = 0) -> None:
        """dis_set_host_pipeline: pairs per chunk of a host-memory batch call
        (0 = auto, about 64 MB of flow); results are identical."""
        _check(lib().dis_set_host_pipeline(self._ctx, chunk_pairs))

    def host_pipeline_info(self) -> dict:
        """What the last host-memory call did (chunks, direct DMA of page-locked buffers)."""
        h = _HostInfo()
        _check(lib().dis_host_pipeline_info(self._ctx, ctypes.byref(h)))
        return {k: getattr(h, k) for k, _ in _HostInfo._fields_}

    def calc_batch_host(self, n: int, I0_ptr: int, I1_ptr: int, flow_ptr: int, stride: int = 0,
                        pair_stride: int = 0) -> None:
        """dis_calc_batch_u8 on raw host pointers (pageable or page-locked), synchronous."""
        _check(lib().dis_calc_batch_u8(self._ctx, n, I0_ptr, I1_ptr, stride, pair_stride, flow_ptr,
                                       MEM_HOST, None))

    def set_variant(self, variant: int) -> None:
        """dis_set_kernel_variant (include/dis_abi.h): 0 = auto (specialised kernels),
        1 = generic only, 2 / 3 / 4 / 5 = 4 / 2 / 8 / 1 lanes per patch, 6 = one wave
        per patch, 9 = 2 lanes per patch with the usable LDS tile capped at 24 pixels
        (test hook: most blocks take the fallback list and k_search8_fb); 7 and 8
        were removed in ABI v7."""
        _check(lib().dis_set_kernel_variant(self._ctx, variant))

    def set_concurrency(self, streams: int) -> None:
        """Sub-batch streams per calc (1..8); results are identical for any value."""
        _check(lib().dis_set_concurrency(self._ctx, streams))

    def set_precision(self, mode: int) -> None:
        """PRECISION_EXACT (default, bit-identical to the reference order) or
        PRECISION_FMA (contracted search arithmetic, within the stated tolerance)."""
        _check(lib().dis_set_precision(self._ctx, mode))

    def set_graphs(self, on: bool = True) -> None:
        """Replay batch calls as captured HIP graphs (default on); results are identical."""
        _check(lib().dis_set_graphs(self._ctx, int(on)))

    def set_debug(self, on: bool = True) -> None:
        _check(lib().dis_set_debug(self._ctx, int(on)))

    def debug_dump(self, stage: int, level: int, pair: int = 0) -> np.ndarray:
        cnt = ctypes.c_size_t()
        _check(lib().dis_stage_size(self._ctx, stage, level, ctypes.byref(cnt)))
        out = np.empty(cnt.value, np.float32)
        _check(lib().dis_debug_dump(self._ctx, stage, level, pair, _ptr(out), cnt.value))
        return out

    def fallback_blocks(self, level: int) -> int:
        """Patch blocks of `level` the last calc searched with the fallback
        kernel (start positions too spread for the LDS tile), all sub-batches."""
        return int(self.debug_dump(STAGE_FALLBACK, level)[0])

    def set_kernel_timing(self, on: bool = True) -> None:
        _check(lib().dis_set_kernel_timing(self._ctx, int(on)))

    def kernel_time(self, kernel: int):
        n = ctypes.c_int()
        ms = ctypes.c_double()
        _check(lib().dis_kernel_time(self._ctx, kernel, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value


def optical_flow_from_pyramids(img_first, img_first_dx, img_first_dy, img_second, img_padding: int,
                               width: int, height: int, coarsest_scale: int, finest_scale: int,
                               iterations: int, patch_size: int, patch_overlap: float,
                               patch_normalization: bool, img_second_dx=None, img_second_dy=None,
                               device: int = 0) -> np.ndarray:
    """OpticalFlowClass(...) (include/optical_flow.hpp:43-54) over padded host
    pyramids (lists of float32 2-D arrays, level 0..C). Returns the finest-level
    flow ((height>>F) x (width>>F) x 2)."""
    nl = coarsest_scale + 1

    def arr(planes):
        planes = [np.ascontiguousarray(p, dtype=np.float32) if p is not None else None for p in planes]
        ptrs = (ctypes.c_void_p * nl)(*[p.ctypes.data if p is not None else None for p in planes])
        return planes, ptrs

    keep = []
    ptrs = []
    for planes in (img_first, img_first_dx, img_first_dy, img_second,
                   img_second_dx or [None] * nl, img_second_dy or [None] * nl):
        k, p = arr(planes)
        keep.append(k)
        ptrs.append(ctypes.cast(p, ctypes.POINTER(ctypes.c_void_p)))
    out = np.empty(((height >> finest_scale), (width >> finest_scale), 2), np.float32)
    _check(lib().dis_flow_from_pyramids(*ptrs, img_padding, _ptr(out), width, height, coarsest_scale,
                                        finest_scale, iterations, patch_size, patch_overlap,
                                        int(patch_normalization), device))
    return out
