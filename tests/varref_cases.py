"""The shape matrix of the variational-refinement checks, shared by
tests/test_varref_host.py (CPU) and tests/test_gpu_varref.py (GPU) -- tests
only. Each shape sits where k_vr_lin / k_vr_sor (csrc/dis_varref.hip) change
path: at a tile edge +-1, at the first level with a border-free SOR tile, at
tile counts on both sides of the XCD remap's multiple of 8 (DESIGN.md 2 has
the table of which shape covers which path).

Everything here is computed once per process, shared and left unchanged
(arrays are read-only)."""
import numpy as np

import oracle_binding as ob

f32 = np.float32
PS, IT, OV, NORM = 8, 4, 0.5, 1


class Case:
    def __init__(self, name, W, H, C, F, batch=1):
        self.name, self.W, self.H, self.C, self.F, self.batch = name, W, H, C, F, batch

    def __repr__(self):
        return self.name


MATRIX = [
    #    name          W    H    C  F  batch
    Case("tiny",       24,  16,  3, 0),     # levels 24x16 .. 3x2: every derivative tap clamps on both sides
    Case("sub-tile",   9,   7,   0, 0),     # far below both tile sizes
    Case("lin-31x33",  31,  33,  0, 0),     # k_vr_lin's 32 x 32 tile +-1, odd and even W
    Case("lin-32x32",  32,  32,  0, 0),
    Case("lin-33x31",  33,  31,  0, 0),
    Case("lin-65x33",  65,  33,  0, 0),
    Case("sor-107x45", 107, 45,  0, 0),     # one 108 x 46 SOR tile -1, exactly, +1 (a second tile
    Case("sor-108x46", 108, 46,  0, 0),     # column and row of 1 output column / row)
    Case("sor-109x47", 109, 47,  0, 0),
    Case("9-tiles",    217, 93,  0, 0),     # one tile per XCD + an identity tail of 1
    Case("18-tiles",   217, 93,  0, 0, 2),  # tail of 2; the pair index crosses the remap
    Case("no-int",     226, 101, 0, 0),     # the last shape without sor_tile<true>
    Case("int-x-only", 227, 101, 0, 0),     # each dimension's bound of that choice on its own: one
    Case("int-y-only", 226, 102, 0, 0),     # row / one column short of an interior tile
    Case("interior",   227, 102, 0, 0),     # the first shape with it
    Case("16-tiles",   325, 139, 0, 0),     # tile counts that are multiples of 8
    Case("48-tiles",   325, 139, 0, 0, 3),  # (2 sub-batch streams)
    Case("ragged-c3",  203, 151, 3, 0),     # ragged padding; a refined level feeds the next start
    Case("c2f1-b2",    160, 120, 2, 1, 2),  # F = 1 upsamples a refined level
]
BY_NAME = {c.name: c for c in MATRIX}
INPUTS = ("synth", "steps", "same", "flat")
VR = (1, 3)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def inputs_of(case):
    """The inputs a case runs: all four, or synth and steps for a batch."""
    return INPUTS if case.batch == 1 else INPUTS[:2]


def level_shapes(case):
    """[(w, h)] of the refined levels F..C of a case."""
    Wp, Hp = ob.padded_size(case.W, case.H, case.C)[:2]
    return [(Wp >> l, Hp >> l) for l in range(case.F, case.C + 1)]


def all_level_shapes():
    """Every refined level shape of the matrix, once each, in matrix order."""
    out = []
    for c in MATRIX:
        for s in level_shapes(c):
            if s not in out:
                out.append(s)
    return out


def frames(case, kind):
    """-> (I0, I1) stacked u8 frames (batch, H, W) of one input kind; pair k of
    a batch differs from pair 0 (seed + k, pattern shifted by k)."""
    def make():
        import disflow
        W, H = case.W, case.H
        a, b = [], []
        for k in range(case.batch):
            if kind == "synth":
                i0, i1 = disflow.synth_pair(40 + k, W, H)
            elif kind == "steps":  # 0 / 255 blocks of 5 x 7 pixels; frame 2 = frame 1 rolled by (2, -3)
                yy, xx = np.mgrid[0:H, 0:W]
                i0 = ((((xx + k) // 5 + (yy + 2 * k) // 7) & 1) * 255).astype(np.uint8)
                i1 = np.roll(i0, (-3, 2), axis=(0, 1))
            elif kind == "same":
                i0 = np.random.default_rng(900 + k).integers(0, 256, (H, W)).astype(np.uint8)
                i1 = i0.copy()
            else:
                i0 = np.full((H, W), 97 + k, np.uint8)
                i1 = i0.copy()
            a.append(i0)
            b.append(i1)
        return _freeze(np.ascontiguousarray(np.stack(a)), np.ascontiguousarray(np.stack(b)))
    return _once(("frames", case.name, kind), make)


def pyramids(case, kind, k):
    """The oracle's padded pyramids of pair k: (Wp, Hp, P0, PX, PY, P1, py0, py1)."""
    def make():
        I0, I1 = frames(case, kind)
        out = ob.build_pyramids(I0[k], I1[k], case.C, PS)
        for planes in out[2:6]:
            _freeze(*planes)
        return out
    return _once(("pyr", case.name, kind, k), make)


def oracle_levels(case, kind, k, vr):
    """(flow at level F, {l: patch u}, {l: dense flow}) of the oracle's scale loop."""
    Wp, Hp, P0, PX, PY, P1, _, _ = pyramids(case, kind, k)
    return ob.flow_from_pyramids(P0, PX, PY, P1, PS, Wp, Hp, case.C, case.F, IT, PS, OV, NORM, capture=True, vr=vr)


# ---------------------------------------------------------------------------
# float level images and flows for the direct oracle / pyref comparison
# ---------------------------------------------------------------------------
FLOWS = ("smooth", "halves", "far", "const")


def _lattice(rng, w, h, amp, cells=3):
    """Value noise in [-amp, amp]: a (cells + 1)^2 lattice, bilinearly interpolated."""
    lat = rng.uniform(-amp, amp, (cells + 1, cells + 1))
    y, x = np.linspace(0, cells, h), np.linspace(0, cells, w)
    y0, x0 = np.minimum(y.astype(int), cells - 1), np.minimum(x.astype(int), cells - 1)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    g = lambda a, b: lat[a][:, b]
    return ((1 - fy) * (1 - fx) * g(y0, x0) + (1 - fy) * fx * g(y0, x0 + 1)
            + fy * (1 - fx) * g(y0 + 1, x0) + fy * fx * g(y0 + 1, x0 + 1))


def level_pair(w, h):
    """Two float32 planes in [0, 255]: value noise + per-pixel noise, the second
    an independent perturbation of the first (so the residuals are not small)."""
    def make():
        rng = np.random.default_rng(1000 * w + h)
        base = 128 + _lattice(rng, w, h, 90, 4)
        a = np.clip(base + rng.uniform(-35, 35, (h, w)), 0, 255).astype(f32)
        b = np.clip(base + _lattice(rng, w, h, 25, 3) + rng.uniform(-35, 35, (h, w)), 0, 255).astype(f32)
        return _freeze(a, b)
    return _once(("lvl", w, h), make)


def level_flow(w, h, kind):
    """One (h, w, 2) float32 flow: "smooth" value noise within +-3 px; "halves"
    per-pixel integer and half-pixel vectors within +-4 px; "far" value noise
    within +-20 px whose two outermost columns / rows (one below 4 pixels)
    point 20 px out of the frame on their side; "const" one vector everywhere."""
    def make():
        rng = np.random.default_rng(7000 * w + 13 * h + FLOWS.index(kind))
        if kind == "smooth":
            f = np.stack([_lattice(rng, w, h, 3), _lattice(rng, w, h, 3)], -1)
        elif kind == "halves":
            f = rng.integers(-8, 9, (h, w, 2)) * 0.5
        elif kind == "far":
            f = np.stack([_lattice(rng, w, h, 20), _lattice(rng, w, h, 20)], -1)
            bx, by = min(2, w // 2), min(2, h // 2)
            f[:, :bx, 0], f[:, w - bx:, 0] = -20.0, 20.0
            f[:by, :, 1], f[h - by:, :, 1] = -20.0, 20.0
        else:
            f = np.empty((h, w, 2))
            f[...] = (1.5, -2.25)
        return _freeze(np.ascontiguousarray(f, f32))[0]
    return _once(("flow", w, h, kind), make)
