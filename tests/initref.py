"""NumPy restatement of the warm start's init plane (csrc/dis_init.hip,
include/dis_abi.h "Temporal warm start") -- tests only, bit-exact.

* ``sanitize``: components that are not finite or have |c| >= 1e9 become 0;
* ``flow_to_init``: a full-resolution (H, W, 2) flow extended to the padded
  frame (replicate) and halved C + 1 times, ((a + b) + (c + d)) * 0.125 per
  component, the last step's source indices clamped at an odd size;
* ``lookup``: the coarsest level's start 2 * I[ry >> 1][rx >> 1] as the
  ``init`` callable of ``pyref.search_level``.

numpy >= 2 (NEP 50): every operation below rounds once in float32.
"""
import numpy as np

f32 = np.float32


def padded_size(W, H, C):
    """(Wp, Hp, pad_left, pad_top): src/main.cpp:139-155."""
    sf = 1 << C
    padw = (sf - W % sf) % sf
    padh = (sf - H % sf) % sf
    return W + padw, H + padh, padw // 2, padh // 2


def plane_size(W, H, C):
    """(iw, ih) of the init plane of W x H frames with coarsest scale C."""
    Wp, Hp, _, _ = padded_size(W, H, C)
    return ((Wp >> C) + 1) // 2, ((Hp >> C) + 1) // 2


def sanitize(a):
    a = np.asarray(a, f32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(a) < f32(1e9)  # False for NaN and inf
    return np.where(ok, a, f32(0)).astype(f32)


def halve(P):
    """One step: (h, w, 2) -> (ceil(h / 2), ceil(w / 2), 2), indices clamped."""
    h, w = P.shape[:2]
    x0 = np.arange(0, w, 2)
    y0 = np.arange(0, h, 2)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    a, b = P[np.ix_(y0, x0)], P[np.ix_(y0, x1)]
    c, d = P[np.ix_(y1, x0)], P[np.ix_(y1, x1)]
    return (((a + b) + (c + d)) * f32(0.125)).astype(f32)


def flow_to_init(flow, C):
    """(H, W, 2) full-resolution flow -> (ih, iw, 2) init plane."""
    flow = sanitize(flow)
    H, W = flow.shape[:2]
    Wp, Hp, pl, pt = padded_size(W, H, C)
    xs = np.clip(np.arange(Wp) - pl, 0, W - 1)
    ys = np.clip(np.arange(Hp) - pt, 0, H - 1)
    P = flow[np.ix_(ys, xs)]
    for _ in range(C + 1):
        P = halve(P)
    return P


def lookup(plane):
    """init callable for pyref.search_level: (pid, rx, ry) -> 2 * I[ry >> 1][rx >> 1]."""
    plane = sanitize(plane)

    def init(pid, rx, ry):
        v = plane[int(ry) >> 1, int(rx) >> 1]
        return v[0] * f32(2), v[1] * f32(2)

    return init
