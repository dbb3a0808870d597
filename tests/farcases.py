"""The far cases of the context-free operators ("Far
offsets"): two batches of just over 2^31 pixels in ONE call, the buffers each
entry point takes at them, and which images of a batch a test looks at.

A kernel forms, per lane, a pixel index (row * W + x0, f * W * H), element
indices of twice that (float2 / half2 vectors), byte indices of up to eight
times that, and workspace offsets per field. One `int` or `unsigned` in such a
product is invisible below 2^31; above it the lane reads another image or
writes outside the buffer. So for every buffer of a call the probes are the
images around every crossing of 2^31 or a multiple of 2^32, counted in bytes,
in elements of the buffer and in pixels.

Pure integers (no numpy arrays, no device): tests/test_far_offsets_host.py
checks the plan without a GPU, tests/test_gpu_far_offsets.py runs it."""
from dataclasses import dataclass

import numpy as np

GIB = 1 << 30
MEMORY_CAP = 40 * GIB   # a test holds at most this much device memory at once
GUARD = 4096            # bytes of guard zone on either side of every output
TEMPORARIES = 3 * GIB   # what a test's device-side generation and comparisons hold on top of its buffers
EXTRA_PROBES = 16
SEED = 0x0FA2


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    n: int

    @property
    def image_pixels(self):
        return self.W * self.H

    @property
    def pixels(self):
        return self.n * self.W * self.H


# aligned: every vector load and store form applies (W % 16 == 0, tight strides
# that are multiples of 16) and the 2^30 and 2^31 pixel marks are image starts.
# ragged: no vector form applies (odd W, odd W * H) and the marks fall inside
# images. even: the ragged case of the 4:2:0 entry points, which refuse odd
# sides: W is no multiple of the 16-pixel strip, of 4 or of 8, and the marks
# fall inside images.
ALIGNED = Case("aligned", 256, 128, 65539)
RAGGED = Case("ragged", 253, 131, 64797)
EVEN = Case("even", 250, 130, 66080)
CASES = {c.name: c for c in (ALIGNED, RAGGED)}
YUV_CASES = {c.name: c for c in (ALIGNED, EVEN)}

# dis_flow_color: more fields than a launch's y extent holds, in both range modes
COLOR = Case("color", 16, 8, 65539)


@dataclass(frozen=True)
class Buffer:
    """One buffer of a call: image i begins at i * image_bytes. elem: bytes of
    the element the kernel indexes it by (1 u8, 2 f16, 4 f32 / u32, 8 keys and
    doubles). out: the call writes it (it gets guard zones)."""
    name: str
    image_bytes: int
    elem: int = 1
    out: bool = False

    def bytes(self, n):
        return n * self.image_bytes


def u8(name, case, channels=1, out=False):
    return Buffer(name, case.image_pixels * channels, 1, out)


ROW_PAD, IMAGE_PAD = 5, 7  # bytes after every row and every image of a padded stack: no stride keeps an alignment


def strided(name, rows, row_bytes, pad):
    """A u8 stack of `rows` rows of `row_bytes` samples an image, tight or padded:
    (stride, image_stride, Buffer). bytes() overstates a padded extent by the
    last image's padding, which the allocation simply holds."""
    stride = row_bytes + (ROW_PAD if pad else 0)
    image_stride = stride * rows + (IMAGE_PAD if pad else 0)
    return stride, image_stride, Buffer(name, image_stride, 1, False)


def padded_u8(name, case, channels):
    """the padded stack of W x H images of `channels` samples a pixel"""
    return strided(name, case.H, case.W * channels, True)


def flow(name, case, dtype, out=False):
    e = np.dtype(dtype).itemsize
    return Buffer(name, case.image_pixels * 2 * e, e, out)


def per_image(name, nbytes, elem, out=False):
    return Buffer(name, nbytes, elem, out)


def fill_cells(W, H):
    """cells of dis_flow_fill's levels above the field (8 bytes each)"""
    c = 0
    while W > 1 or H > 1:
        W, H = (W + 1) // 2, (H + 1) // 2
        c += W * H
    return c


def motion_ws_bytes(case, terms):
    chunks = (case.image_pixels + 16383) // 16384
    return (chunks * terms + 16) * 8


def thresholds(total):
    """2^31 and every multiple of 2^32 below `total` units"""
    t = [1 << 31] if total > (1 << 31) else []
    k = 1
    while (k << 32) < total:
        t.append(k << 32)
        k += 1
    return t


def crossings(case, buf):
    """[(unit, threshold, image)]: the image of `buf` that holds unit number
    `threshold`, for units of one byte, one element and one pixel's worth."""
    out = []
    units = {1: "byte", buf.elem: "element" if buf.elem > 1 else "byte"}
    px = buf.image_bytes // case.image_pixels if buf.image_bytes % case.image_pixels == 0 else 0
    if px:
        units[px] = "pixel" if px > 1 else "byte"
    for size, unit in sorted(units.items()):
        for t in thresholds(buf.bytes(case.n) // size):
            out.append((unit, t, (t * size) // buf.image_bytes))
    return out


def probe_images(case, buffers):
    """Sorted image indices: the ends of the batch, every image that contains,
    precedes or follows a crossing of any buffer, and EXTRA_PROBES more from a
    seeded generator."""
    n = case.n
    s = {0, 1, n - 2, n - 1}
    for b in buffers:
        for _, _, img in crossings(case, b):
            s.update((img - 1, img, img + 1))
    rng = np.random.default_rng(SEED)
    s.update(int(i) for i in rng.integers(0, n, EXTRA_PROBES))
    return sorted(i for i in s if 0 <= i < n)


def peak_bytes(case, buffers):
    """device bytes of a test's buffers with their guard zones (TEMPORARIES come on top)"""
    return sum(b.bytes(case.n) + 2 * GUARD for b in buffers)


def marks_inside_images(case):
    """neither the 2^30 nor the 2^31 pixel mark is an image start"""
    return all((1 << k) % case.image_pixels for k in (30, 31))


# ---- the buffers of every entry point's far call, by variant --------------------
# A variant is what changes an index type: the flow format, the channels, padded
# source strides (once per family that takes them). Formats are chosen to fit
# MEMORY_CAP: compose reads f16 and writes f32 (or reads f32 + f16 and writes
# f16), interp runs one channel without a backward flow (its workspace alone is
# 16 GiB), consistency checks a field against itself (fw and bw are both only
# read, so they may be one buffer: two f32 fields, the mask and err are 42 GiB).

F16, F32 = np.float16, np.float32


def plan(entry, variant, case):
    """The Buffers of `entry` (the C-ABI name without dis_) in `variant` at `case`."""
    c = case
    if entry == "flow_warp_u8":
        dt, C, pad = variant
        src = padded_u8("src", c, C)[2] if pad else u8("src", c, C)
        return [src, flow("flow", c, dt), u8("dst", c, C, True), u8("valid", c, 1, True)]
    if entry == "flow_interp_u8":
        dt, C, pad = variant
        im = lambda name: strided(name, c.H, c.W * C, pad)[2]
        return [im("I0"), im("I1"), flow("fw", c, dt), u8("dst", c, C, True), u8("fill", c, 1, True),
                per_image("workspace", c.image_pixels * 8, 8)]
    if entry == "flow_consistency":
        return [flow("fw", c, F32), u8("mask", c, 1, True), per_image("err", c.image_pixels * 4, 4, True)]
    if entry == "flow_convert":
        s_dt, d_dt = variant
        return [flow("src", c, s_dt), flow("dst", c, d_dt, True)]
    if entry == "flow_compose":
        a, b, o = variant
        return [flow("a", c, a), flow("b", c, b), flow("out", c, o, True), u8("valid_out", c, 1, True)]
    if entry == "flow_advect_points":
        (dt,) = variant
        pts = ADVECT_POINTS * 8
        return [flow("flow", c, dt), per_image("points", pts, 4), per_image("points_out", pts, 4, True),
                per_image("status", ADVECT_POINTS, 1, True)]
    if entry == "flow_fill":
        i, o = variant
        return [flow("flow", c, i), u8("mask", c), flow("out", c, o, True), u8("level", c, 1, True),
                per_image("workspace", fill_cells(c.W, c.H) * 8, 8)]
    if entry in ("flow_fit_motion", "flow_fit_homography"):
        (dt,) = variant
        k, terms = (6, 12) if entry == "flow_fit_motion" else (8, 27)
        return [flow("flow", c, dt), u8("mask", c), per_image("params", 4 * k, 4, True), per_image("info", 16, 4, True),
                u8("inliers", c, 1, True), per_image("workspace", motion_ws_bytes(c, terms), 8)]
    if entry in ("motion_to_flow", "homography_to_flow"):
        (dt,) = variant
        k = 6 if entry == "motion_to_flow" else 8
        return [per_image("params", 4 * k, 4), flow("out", c, dt, True)]
    if entry in ("warp_motion_u8", "warp_homography_u8"):
        C, pad = variant
        k = 6 if entry == "warp_motion_u8" else 8
        src = padded_u8("src", c, C)[2] if pad else u8("src", c, C)
        return [src, per_image("params", 4 * k, 4), u8("dst", c, C, True), u8("valid", c, 1, True)]
    if entry == "temporal_denoise_u8":
        dt, C, pad = variant
        mk = lambda name: padded_u8(name, c, C)[2] if pad else u8(name, c, C)
        return [mk("cur"), mk("neighbour"), flow("flow", c, dt), u8("mask", c), u8("dst", c, C, True),
                u8("support", c, 1, True)]
    if entry == "frames_to_gray_u8":
        C, pad = variant
        return [strided("src", c.H, c.W * C, pad)[2], u8("dst", c, 1, True)]
    if entry in ("yuv420_to_frames_u8", "frames_to_yuv420_u8"):
        # the padded variant pads what the call reads: the surface's three planes, or the frames
        C, pad = variant
        to_frames = entry == "yuv420_to_frames_u8"
        q = c.image_pixels // 4
        if to_frames:
            return [u8("frames", c, C, True), strided("y", c.H, c.W, pad)[2], strided("cb", c.H // 2, c.W // 2, pad)[2],
                    strided("cr", c.H // 2, c.W // 2, pad)[2]]
        return [strided("frames", c.H, c.W * C, pad)[2], u8("y", c, 1, True), per_image("cb", q, 1, True),
                per_image("cr", q, 1, True)]
    if entry == "flow_color":  # (the workspace, 128 bytes a field, is the library's own allocation)
        return [flow("flow", c, F32), u8("bgr", c, 3, True)]
    raise KeyError(entry)


ADVECT_POINTS = 64  # points per field

# entry -> the variants its far tests run
VARIANTS = {
    "flow_warp_u8": [(F16, 1, False), (F32, 4, False), (F16, 3, True)],
    "flow_color": [("automatic",), ("fixed",)],
    "flow_interp_u8": [(F16, 1, True)],
    "flow_consistency": [()],
    "flow_convert": [(F16, F32), (F32, F16)],
    "flow_compose": [(F16, F16, F32), (F32, F16, F16)],
    "flow_advect_points": [(F16,), (F32,)],
    "flow_fill": [(F16, F32), (F32, F16)],
    "flow_fit_motion": [(F16,), (F32,)],
    "motion_to_flow": [(F32,), (F16,)],
    "warp_motion_u8": [(1, False), (3, True), (4, False)],
    "flow_fit_homography": [(F16,), (F32,)],
    "homography_to_flow": [(F32,), (F16,)],
    "warp_homography_u8": [(1, True), (4, False)],
    "temporal_denoise_u8": [(F16, 4, False), (F32, 1, True)],
    "frames_to_gray_u8": [(1, True), (4, False)],
    "yuv420_to_frames_u8": [(1, False), (4, True)],
    "frames_to_yuv420_u8": [(1, True), (4, False)],
}


def cases_of(entry):
    return YUV_CASES if entry in ("yuv420_to_frames_u8", "frames_to_yuv420_u8") else CASES


def all_plans():
    """(entry, variant, case) of every far test (dis_flow_color has a test of many small fields besides)"""
    return [(e, v, c) for e, vs in VARIANTS.items() for v in vs for c in cases_of(e).values()]


def variant_id(v):
    return "-".join(np.dtype(x).name if isinstance(x, type) else x if isinstance(x, str) else
                    ("pad" if x is True else "tight" if x is False else f"c{x}") for x in v) or "plain"
