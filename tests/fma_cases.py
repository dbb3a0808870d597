"""The case matrix of the level-by-level tolerance-mode check, shared by
tests/test_search64_host.py (CPU) and tests/test_gpu_fma_levels.py (GPU) --
tests only. All cases use patch size 8: the smallest shapes that still give
every level partial patch blocks (npw, nph no multiples of 8), ragged padding
and more than one block.

Everything here is computed once per process, shared and left unchanged
(arrays are read-only)."""
import numpy as np

import initref
import oracle_binding as ob
import pyref
import scenes
import searchref64 as s64
import test_oracle as helpers

f32 = np.float32
PS = 8


class Case:
    def __init__(self, name, gen, W, H, C, F, ov, norm, it, batch=1, vr=0, warm=False):
        self.name, self.gen, self.W, self.H, self.C, self.F = name, gen, W, H, C, F
        self.ov, self.norm, self.it, self.batch, self.vr, self.warm = ov, norm, it, batch, vr, warm

    def __repr__(self):
        return self.name


CASES = [
    #    name            generator                     W    H   C  F  overlap norm it
    Case("shift-it0",    ("shift", 5, 1.3, -0.8),      104, 72, 2, 0, 0.5,   1, 0),    # steps 4
    Case("shift-it3",    ("shift", 5, 1.3, -0.8),      104, 72, 2, 0, 0.5,   1, 3),
    Case("bigshift",     ("shift", 11, 9.5, -7.25),    160, 120, 2, 0, 0.5,  1, 12, batch=2),  # resets, OOB starts
    Case("scene31",      ("scene", 31),                203, 151, 3, 0, 0.75, 1, 3),    # steps 2; flat regions, occlusion
    Case("scene32-raw",  ("scene", 32),                160, 120, 3, 1, 0.625, 0, 3),   # steps 3; no normalisation
    Case("synth-ov0",    ("synth", 5),                 200, 136, 3, 2, 0.0,  1, 3),    # steps 8; LPP 1 falls back to 2
    Case("synth-dense",  ("synth", 50),                96, 80, 3, 1, 0.8,    1, 2),    # steps 1; densify + upsample back end
    Case("synth-vr",     ("synth", 60),                160, 120, 3, 1, 0.625, 1, 3, batch=2, vr=2),
    Case("synth-warm",   ("synth", 21),                128, 96, 2, 1, 0.5,   1, 3, warm=True),
    # grid steps 5, 6, 7 (overlaps exact in binary): tile strides 72 / 66 / 72 at 2 and 8 lanes per patch
    Case("shift-step5",  ("shift", 7, 1.3, -0.8),      104, 72, 2, 0, 0.375, 1, 3),    # steps 5
    Case("scene-step6",  ("scene", 33),                160, 120, 3, 1, 0.25, 1, 3),    # steps 6
    Case("synth-step7",  ("synth", 7),                 136, 104, 3, 0, 0.125, 1, 3),   # steps 7
]
STEPS = {"shift-step5": 5, "scene-step6": 6, "synth-step7": 7}  # the grid step a case is there for (asserted)
BY_NAME = {c.name: c for c in CASES}

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def frames(case):
    """-> (I0, I1) stacked u8 frames, (batch, H, W); pair k of a batch uses seed + k."""
    def make():
        import disflow
        out = []
        for k in range(case.batch):
            g = case.gen
            if g[0] == "shift":
                out.append(helpers.shifted_pair(g[1] + k, case.H, case.W, dx=g[2], dy=g[3]))
            elif g[0] == "scene":
                out.append(scenes.scene_pair(g[1] + k, case.W, case.H))
            else:
                out.append(disflow.synth_pair(g[1] + k, case.W, case.H))
        I0 = np.ascontiguousarray(np.stack([a for a, _ in out]))
        I1 = np.ascontiguousarray(np.stack([b for _, b in out]))
        _freeze(I0, I1)
        return I0, I1
    return _once(("frames", case.name), make)


def warm_plane(case):
    """The warm case's coarse init planes (batch, ih, iw, 2): value noise within
    +-1.5 px (a 4 x 3 lattice of uniform values, bilinearly interpolated)."""
    def make():
        iw, ih = initref.plane_size(case.W, case.H, case.C)
        rng = np.random.default_rng(77)
        lat = rng.uniform(-1.5, 1.5, (case.batch, 3, 4, 2))
        y, x = np.linspace(0, 2, ih), np.linspace(0, 3, iw)
        y0, x0 = np.minimum(y.astype(int), 1), np.minimum(x.astype(int), 2)
        fy, fx = (y - y0)[None, :, None, None], (x - x0)[None, None, :, None]
        g = lambda a, b: lat[:, a][:, :, b]
        p = ((1 - fy) * (1 - fx) * g(y0, x0) + (1 - fy) * fx * g(y0, x0 + 1)
             + fy * (1 - fx) * g(y0 + 1, x0) + fy * fx * g(y0 + 1, x0 + 1)).astype(f32)
        _freeze(p)
        return p
    return _once(("warm", case.name), make)


# tile_layout of dis_search8.hip per grid step, as the table in tests/test_gpu_fma_levels.py
# states it: (LPP 1 stride or None where LPP 1 does not fit and runs as LPP 2, LPP 2 stride,
# LPP 2 half-wave layout (0: 2 x 8, 1: 4 x 4 patches), LPP 4 stride, LPP 8 stride)
TILE_TABLE = {
    1: (100, 72, 1, 68, 72),
    2: (98, 66, 0, 66, 68),
    3: (100, 72, 1, 68, 72),
    4: (97, 65, 0, 65, 66),
    5: (100, 72, 1, 68, 72),
    6: (98, 66, 0, 66, 68),
    7: (100, 72, 1, 68, 72),
    8: (None, 65, 0, 65, 65),
}
LAUNCH_TS_STRIDES = (65, 66, 68, 72)  # the strides launch_ts holds as template constants


def tile_layout(st, lpp):
    """tile_bank_multiplicity / tile_layout of dis_search8.hip restated (not read from the
    library, which exports neither): the LDS tile row stride in (tile width, max stride]
    and, at 2 lanes per patch, the half-wave layout with the least worst-case bank
    multiplicity of a 32-lane group's reads at zero flow; ties keep the first candidate."""
    w, smax = (96, 128) if lpp == 1 else (64, 72)

    def multiplicity(quad, S):
        cnt = [0] * 32
        for l in range(32):
            if lpp == 1:
                gx, gy, off = l >> 3, l & 7, 0
            elif lpp == 2:
                p = l >> 1
                gx, gy, off = ((p & 3), (p >> 2) & 3, 4 * (l & 1)) if quad else (p >> 3, p & 7, 4 * (l & 1))
            elif lpp == 4:
                gx, gy, off = 0, l >> 2, l & 3
            else:
                gx, gy, off = 0, (l >> 4) * 2 + ((l >> 2) & 1), (l & 3) | (((l >> 3) & 1) << 2)
            cnt[(st * S * gy + st * gx + off) % 32] += 1
        return max(cnt)

    best = min(((multiplicity(q, S), q, S) for q in range(2 if lpp == 2 else 1) for S in range(w + 1, smax + 1)),
               key=lambda t: t[0])  # min keeps the first of equals: quad 0 before 1, strides ascending
    return best[2], best[1]


def lpp1_fits(st):
    """search8_lpp1_fits: the 16 x 8 block's I0 region in the 64 x 128 tile buffer."""
    return (15 * st + 11) * (7 * st + 10) <= 64 * 128


def steps(case):
    st = ob.steps(PS, case.ov)
    assert st == STEPS.get(case.name, st), (case.name, st)
    return st


def pyramids(case, k):
    """The oracle's padded pyramids of pair k: (Wp, Hp, P0, PX, PY, P1, py0, py1)."""
    def make():
        I0, I1 = frames(case)
        out = ob.build_pyramids(I0[k], I1[k], case.C, PS)
        for planes in out[2:6]:
            _freeze(*planes)
        return out
    return _once(("pyr", case.name, k), make)


def level_size(case, k, l):
    Wp, Hp = pyramids(case, k)[:2]
    return Wp >> l, Hp >> l


def pyref_init(init):
    if init is None:
        return None
    return lambda pid, rx, ry: (init[pid, 0], init[pid, 1])


def yardstick(case, k, l, init):
    """pyref.search_level (the reference-order float32 restatement the oracle
    is pinned to) on level l of pair k from the given per-patch start."""
    _, _, _, PX, PY, P1, _, _ = pyramids(case, k)
    w, h = level_size(case, k, l)
    u, _ = pyref.search_level(PX[l], PY[l], P1[l], PS, w, h, PS, steps(case), case.it, case.norm, pyref_init(init))
    return u


def reference(case, k, l, init, mode="f64", mutation=None, style=()):
    _, _, _, PX, PY, P1, _, _ = pyramids(case, k)
    w, h = level_size(case, k, l)
    return s64.search(PX[l], PY[l], P1[l], PS, w, h, PS, steps(case), case.it, case.norm, init, mode, mutation, style)


def level_check(case, k, l, init):
    """(Trace, yardstick set) of level l of pair k from `init`: the float64
    search, and [pyref.search_level's u, the float32 restatement of the
    2-lanes-per-patch tolerance-mode arithmetic's u] (DESIGN.md 2 on why the
    second is there). Cached by the start's bits, so kernel layouts that agree
    on a start share the work."""
    key = ("lvl", case.name, k, l, None if init is None else np.ascontiguousarray(init, f32).tobytes())
    return _once(key, lambda: (reference(case, k, l, init),
                               [yardstick(case, k, l, init), reference(case, k, l, init, "f32", None, s64.FMA_LPP2)]))


def fma_restatement(case, k, l, init, lpp2):
    """The tolerance-mode kernel's arithmetic restated in float32 numpy: the
    2-lanes-per-patch kernel's (the yardstick set's second member), or the
    1 / 4 / 8-lanes-per-patch kernels', whose sums keep Eigen's order."""
    if lpp2:
        return level_check(case, k, l, init)[1][1]
    key = ("eig", case.name, k, l, None if init is None else np.ascontiguousarray(init, f32).tobytes())
    return _once(key, lambda: reference(case, k, l, init, "f32", None, s64.FMA_LPP2[:3]))


def oracle_starts(case, k):
    """Per level l in C..F: the per-patch start (N, 2) float32 (None: zero) the
    exact pipeline gives level l -- from the oracle's exact dense field of the
    level above (refined when the case refines), or, warm case, the caller's
    init plane at the coarsest level and the exact densification below it."""
    def make():
        Wp, Hp, P0, PX, PY, P1, py0, py1 = pyramids(case, k)
        st, C, F = steps(case), case.C, case.F
        starts = {}
        if case.warm:
            assert case.vr == 0
            dense = initref.sanitize(warm_plane(case)[k])
            for l in range(C, F - 1, -1):
                w, h = Wp >> l, Hp >> l
                starts[l] = s64.start_from_dense(dense, w, h, st)
                u, geom = pyref.search_level(PX[l], PY[l], P1[l], PS, w, h, PS, st, case.it, case.norm,
                                             pyref_init(starts[l]))
                dense = pyref.densify(u, geom, w, h, PS, st)
        else:
            _, _, ds = ob.flow_from_pyramids(P0, PX, PY, P1, PS, Wp, Hp, C, F, case.it, PS, case.ov, case.norm,
                                             capture=True, vr=case.vr)
            for l in range(C, F - 1, -1):
                starts[l] = None if l == C else s64.start_from_dense(ds[l + 1], Wp >> l, Hp >> l, st)
        for a in starts.values():
            if a is not None:
                _freeze(a)
        return starts
    return _once(("starts", case.name, k), make)
