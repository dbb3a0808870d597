"""The perspective scene of the homography tests: tests/motionscene.py's 320 x
240 value-noise frame and its block moving on its own, with the camera map a
homography: motionscene's similarity (about 1 %) and a projective row p6 = 6e-5,
p7 = -4e-5 per pixel (d runs from 1 to about 1.02 across the frame), what a
hand-held camera's rotation does between two frames."""
import numpy as np

import motionscene

W, H = motionscene.W, motionscene.H
ENGINE = motionscene.ENGINE
_c = motionscene.TRUE_CENTRED
_cx, _cy = (W - 1) / 2.0, (H - 1) / 2.0
# the truth in frame coordinates: dis_flow_fit_homography's eight parameters
TRUE = np.array([_c[0] - _c[1] * _cx - _c[2] * _cy, _c[1], _c[2], _c[3] - _c[4] * _cx - _c[5] * _cy, _c[4], _c[5],
                 6e-5, -4e-5])
_cache = {}


def matrix():
    q = TRUE
    return np.array([[1 + q[1], q[2], q[0]], [q[4], 1 + q[5], q[3]], [q[6], q[7], 1.0]])


def true_field():
    """(H, W, 2) float64: the camera's flow at every pixel."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    M = matrix()
    d = M[2, 0] * xx + M[2, 1] * yy + M[2, 2]
    return np.stack([(M[0, 0] * xx + M[0, 1] * yy + M[0, 2]) / d - xx, (M[1, 0] * xx + M[1, 1] * yy + M[1, 2]) / d - yy], -1)


def frames():
    """(I0, I1) u8: I1(x + flow(x)) = I0(x) for the homography, except on the block."""
    if "frames" not in _cache:
        m = 40
        big = motionscene._noise(W + 2 * m, H + 2 * m, 5)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        I0 = motionscene._sample(big, xx + m, yy + m)
        Mi = np.linalg.inv(matrix())
        d = Mi[2, 0] * xx + Mi[2, 1] * yy + Mi[2, 2]
        sx, sy = (Mi[0, 0] * xx + Mi[0, 1] * yy + Mi[0, 2]) / d, (Mi[1, 0] * xx + Mi[1, 1] * yy + Mi[1, 2]) / d
        I1 = motionscene._sample(big, sx + m, sy + m)
        obj = motionscene._noise(120, 80, 9)  # 9600 of 76800 pixels
        I0[60:140, 40:160] = obj
        I1[54:134, 49:169] = obj
        out = tuple(np.clip(np.round(f), 0, 255).astype(np.uint8) for f in (I0, I1))
        for f in out:
            f.setflags(write=False)
        _cache["frames"] = out
    return _cache["frames"]


def oracle_flow(oracle):
    """The CPU oracle's flow of the pair at ENGINE's settings: computed once."""
    if "flow" not in _cache:
        I0, I1 = frames()
        C, F, ps, it, ov = ENGINE
        f = np.ascontiguousarray(oracle.calc_u8(np.ascontiguousarray(I0), np.ascontiguousarray(I1), C, F, ps, it, ov))
        f.setflags(write=False)
        _cache["flow"] = f
    return _cache["flow"]
