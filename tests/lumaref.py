"""NumPy restatement of the engine's colour-to-gray conversion (csrc/dis_luma.hip,
dis_frames_to_gray_u8): OpenCV's fixed-point Rec.601,

    gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14,

in uint32 arithmetic, alpha ignored. The coefficients sum to 2^14, so
R = G = B = v gives v, and the largest sum is 4,186,112: nothing wraps."""
import numpy as np

# dis_frame_format: name -> (enum value, channels, index of R, G, B in a pixel)
FORMATS = {
    "gray": (0, 1, None),
    "bgr": (1, 3, (2, 1, 0)),
    "rgb": (2, 3, (0, 1, 2)),
    "bgra": (3, 4, (2, 1, 0)),
    "rgba": (4, 4, (0, 1, 2)),
}
COLOUR = ("bgr", "rgb", "bgra", "rgba")


def channels(fmt):
    return FORMATS[fmt][1]


def luma(r, g, b):
    """The formula on arrays (or scalars) of samples 0..255 -> uint8."""
    r, g, b = (np.asarray(v).astype(np.uint32) for v in (r, g, b))
    return ((r * np.uint32(4899) + g * np.uint32(9617) + b * np.uint32(1868) + np.uint32(8192)) >> np.uint32(14)
            ).astype(np.uint8)


def to_gray(frames, fmt):
    """(..., H, W, C) u8 frames of format `fmt` -> (..., H, W) u8 gray; "gray"
    takes (..., H, W) and copies."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8
    _, C, order = FORMATS[fmt]
    if order is None:
        return a.copy()
    assert a.shape[-1] == C, (a.shape, fmt)
    return luma(a[..., order[0]], a[..., order[1]], a[..., order[2]])
