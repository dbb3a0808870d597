"""The shaky sequence of the stabilisation tests: N = 12 frames of 160 x 120 of a
value-noise scene under a pan of (1.5, 0.5) px per frame, a translation jitter
of +-3 px and a rotation jitter of +-0.4 degrees about the frame centre, seeded.
Frame k shows the scene at T_k x; the true model of the pair k -> k+1 is
T_{k+1}^-1 T_k (where the scene point under pixel x of frame k lies in frame
k+1)."""
import numpy as np

import motionscene

N, W, H = 12, 160, 120
MARGIN = 60
PAN = (1.5, 0.5)
ENGINE = motionscene.ENGINE
_cache = {}


def transforms():
    """T_0 .. T_{N-1}: 3 x 3 float64, frame pixel -> scene pixel."""
    if "T" not in _cache:
        rng = np.random.default_rng(11)
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        T = []
        for k in range(N):
            jx, jy = rng.uniform(-3, 3), rng.uniform(-3, 3)
            a = np.deg2rad(rng.uniform(-0.4, 0.4))
            c, s = np.cos(a), np.sin(a)
            tx, ty = cx + MARGIN + PAN[0] * k + jx, cy + MARGIN + PAN[1] * k + jy
            # R (x - centre) + centre + margin + pan + jitter
            T.append(np.array([[c, -s, tx - (c * cx - s * cy)], [s, c, ty - (s * cx + c * cy)], [0.0, 0.0, 1.0]]))
        _cache["T"] = T
    return _cache["T"]


def frames():
    """(N, H, W) u8, read-only."""
    if "frames" not in _cache:
        big = motionscene._noise(W + 2 * MARGIN, H + 2 * MARGIN, 7)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        out = []
        for T in transforms():
            sx = T[0, 0] * xx + T[0, 1] * yy + T[0, 2]
            sy = T[1, 0] * xx + T[1, 1] * yy + T[1, 2]
            out.append(np.clip(np.round(motionscene._sample(big, sx, sy)), 0, 255).astype(np.uint8))
        f = np.stack(out)
        f.setflags(write=False)
        _cache["frames"] = f
    return _cache["frames"]


def true_pair_matrices():
    """T_{k+1}^-1 T_k for k = 0 .. N-2, 3 x 3 float64."""
    T = transforms()
    return [np.linalg.inv(T[k + 1]) @ T[k] for k in range(N - 1)]


def true_pair_params():
    """The true pair models as dis_flow_fit_motion's six parameters, float32 (N-1, 6)."""
    return np.array([[A[0, 2], A[0, 0] - 1, A[0, 1], A[1, 2], A[1, 0], A[1, 1] - 1] for A in true_pair_matrices()],
                    np.float32)


def oracle_flows(oracle):
    """The CPU oracle's flows of the N - 1 consecutive pairs at ENGINE's settings: computed once."""
    if "flows" not in _cache:
        f = frames()
        C, F, ps, it, ov = ENGINE
        fl = np.stack([np.ascontiguousarray(oracle.calc_u8(np.ascontiguousarray(f[k]), np.ascontiguousarray(f[k + 1]),
                                                           C, F, ps, it, ov)) for k in range(N - 1)])
        fl.setflags(write=False)
        _cache["flows"] = fl
    return _cache["flows"]


def roughness(pair_matrices_true, corrections=None):
    """The RMS second difference (px) of the track of frame 0's centre point:
    its true position in frame k (the true pair models composed), seen through
    correction k (the stabilised frame shows frame k's pixel M_k y at y, so the
    point lands at M_k^-1 of its position); corrections None: the raw track."""
    import stabref

    p = np.array([(W - 1) / 2.0, (H - 1) / 2.0, 1.0])
    C = np.eye(3)
    track = []
    for k in range(N):
        if k:
            C = pair_matrices_true[k - 1] @ C
        q = C @ p
        if corrections is not None:
            q = np.linalg.inv(stabref.matrix(corrections[k])) @ q
        track.append(q[:2])
    t = np.array(track)
    d2 = t[2:] - 2 * t[1:-1] + t[:-2]
    return float(np.sqrt((d2 ** 2).sum(axis=1).mean()))
