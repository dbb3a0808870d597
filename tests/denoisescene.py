"""The seeded sequence of the temporal-denoising tests: a 192 x 128 value-noise
background that moves (4, 1.5) pixels a frame, a textured ellipse on it that
moves (-5, 3) pixels a frame, and Gaussian noise of a given sigma added to
every frame on its own. Clean and noisy frames as u8."""
import numpy as np

W, H = 192, 128
T = 5                      # frames of a sequence; the centre frame is T // 2
ENGINE = (3, 1, 8, 25, 0.625)  # coarsest, finest, patch size, iterations, overlap
SETTINGS = ((8.0, 1), (8.0, 2), (15.0, 3))  # (sigma, seed)
BG_V = (4.0, 1.5)
OBJ_V = (-5.0, 3.0)
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


def sequence(sigma, seed):
    """(clean, noisy): two u8 arrays (T, H, W), made once per (sigma, seed)."""
    key = (float(sigma), int(seed))
    if key not in _cache:
        m = 32
        big = _noise(W + 2 * m, H + 2 * m, 100 + seed)
        tex = _noise(W + 2 * m, H + 2 * m, 200 + seed)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        rng = np.random.default_rng(300 + seed)
        clean = np.empty((T, H, W))
        for t in range(T):
            d = t - T // 2
            f = _sample(big, xx + m - BG_V[0] * d, yy + m - BG_V[1] * d)
            cx, cy = W / 2 + OBJ_V[0] * d, H / 2 + OBJ_V[1] * d
            inside = ((xx - cx) / 34.0) ** 2 + ((yy - cy) / 22.0) ** 2 <= 1.0
            obj = 255.0 - _sample(tex, xx + m - OBJ_V[0] * d, yy + m - OBJ_V[1] * d)
            clean[t] = np.where(inside, obj, f)
        noisy = clean + rng.normal(0.0, sigma, clean.shape)
        out = tuple(np.clip(np.round(a), 0, 255).astype(np.uint8) for a in (clean, noisy))
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def oracle_flows(oracle, sigma, seed, radius):
    """The CPU oracle's flows from the noisy centre frame to its 2 * radius
    neighbours (ascending), at ENGINE's settings: (neighbour indices, flows),
    each flow computed once."""
    _, noisy = sequence(sigma, seed)
    c = T // 2
    C, F, ps, it, ov = ENGINE
    js = [j for j in range(c - radius, c + radius + 1) if j != c]
    flows = []
    for j in js:
        key = (float(sigma), int(seed), j)
        if key not in _cache:
            f = np.ascontiguousarray(oracle.calc_u8(np.ascontiguousarray(noisy[c]), np.ascontiguousarray(noisy[j]),
                                                    C, F, ps, it, ov))
            f.setflags(write=False)
            _cache[key] = f
        flows.append(_cache[key])
    return js, flows
