"""The camera-motion scene of the global-motion tests: a value-noise frame moved
by a similarity (scale 1.01, 0.6 degrees, translation (2.5, -1.75)) with a
textured block of 12.5 % of the frame moving on its own by (9, -6)."""
import numpy as np

W, H = 320, 240
ENGINE = (3, 1, 8, 12, 0.5)  # coarsest, finest, patch size, iterations, overlap
_S = 1.01 * np.cos(np.deg2rad(0.6)) - 1.0
_R = 1.01 * np.sin(np.deg2rad(0.6))
# the centred truth: u = 2.5 + s x' - r y', v = -1.75 + r x' + s y'
TRUE_CENTRED = np.array([2.5, _S, -_R, -1.75, _R, _S])
_cache = {}


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w))
    for o, amp in ((32, 60), (16, 40), (8, 25), (4, 15)):
        g = rng.uniform(-1, 1, (h // o + 3, w // o + 3))
        yy, xx = np.mgrid[0:h, 0:w] / o
        y0, x0 = yy.astype(int), xx.astype(int)
        a, b = xx - x0, yy - y0
        img += amp * ((1 - a) * (1 - b) * g[y0, x0] + a * (1 - b) * g[y0, x0 + 1] + (1 - a) * b * g[y0 + 1, x0]
                      + a * b * g[y0 + 1, x0 + 1])
    return img + 128


def _sample(img, px, py):
    h, w = img.shape
    px, py = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    a, b = px - x0, py - y0
    return (1 - a) * (1 - b) * img[y0, x0] + a * (1 - b) * img[y0, x1] + (1 - a) * b * img[y1, x0] + a * b * img[y1, x1]


def frames():
    """(I0, I1) u8: I1(x + flow(x)) = I0(x) for the similarity, except on the block."""
    if "frames" not in _cache:
        m = 40
        big = _noise(W + 2 * m, H + 2 * m, 5)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        xc, yc = xx - (W - 1) / 2, yy - (H - 1) / 2
        I0 = _sample(big, xx + m, yy + m)
        Ai = np.linalg.inv(np.array([[1 + _S, -_R], [_R, 1 + _S]]))
        dx, dy = xc - TRUE_CENTRED[0], yc - TRUE_CENTRED[3]
        sx, sy = Ai[0, 0] * dx + Ai[0, 1] * dy, Ai[1, 0] * dx + Ai[1, 1] * dy
        I1 = _sample(big, sx + (W - 1) / 2 + m, sy + (H - 1) / 2 + m)
        obj = _noise(120, 80, 9)  # 9600 of 76800 pixels
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
