"""Every context-free operator past 2^31 pixels in one call (tests/farcases.py,
DESIGN.md section 2 "Far offsets"). A test runs its entry point twice on
device pointers:

  identity  inputs that are random per image (made on the device, so no two
            images are equal and a wrapped index cannot read the right bytes
            by accident), configured so that the result is known without a
            reference, compared on the device over every byte;
  probes    random inputs with the special vectors (NaN, +-inf, +-1e9) in the
            probe images; the probe images' inputs and outputs come down and
            are compared bit for bit with the numpy restatements.

Every output lies between 4 KiB guard zones that must come back untouched, and
a byte plane with a closed value set is prefilled with a value outside the set,
which must be gone everywhere. A test frees its memory before it returns and
prints its wall time and peak device memory (pytest -s shows the lines).

Run one family per process (pytest -k <entry point>), each under a time limit."""
import time

import numpy as np
import pytest

import composeref
import denoiseref
import farcases as fc
import fbref
import fillref
import homographyref
import interpref
import lumaref
import motionref
import stabref
import warpref
import yuvref

pytestmark = pytest.mark.gpu

STEP = 1 << 27      # elements of one device-side pass: its temporaries stay within farcases.TEMPORARIES
UNSET = 77          # prefill of a closed-set byte plane: not 0, 1, 2, 255, a level or a count
GUARD_BYTE = 0xA5
DST_FILL = 0x4D

PLANS = fc.all_plans()
IDS = [f"{e}-{fc.variant_id(v)}-{c.name}" for e, v, c in PLANS]


class Dev:
    """The device buffers of one far call, each between two guard zones."""

    def __init__(self, torch, case, bufs):
        self.torch, self.case = torch, case
        self.W, self.H, self.n, self.P = case.W, case.H, case.n, case.image_pixels
        need = fc.peak_bytes(case, bufs) + fc.TEMPORARIES  # (<= MEMORY_CAP: tests/test_far_offsets_host.py)
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            pytest.skip(f"needs {need} bytes of device memory, {free} are free")
        torch.cuda.reset_peak_memory_stats()
        self.buf = {b.name: b for b in bufs}
        self.raw = {}
        for b in bufs:
            nb = b.bytes(case.n)
            raw = torch.empty(nb + 2 * fc.GUARD, dtype=torch.uint8, device="cuda:0")
            raw[:fc.GUARD] = GUARD_BYTE
            raw[fc.GUARD + nb:] = GUARD_BYTE
            self.raw[b.name] = raw

    def close(self):
        self.raw.clear()
        self.torch.cuda.empty_cache()

    # ---- views -------------------------------------------------------------
    def v(self, name, dtype=None):
        """the buffer without its guards, as uint8 or as `dtype` (a numpy or torch type)"""
        t = self.raw[name][fc.GUARD:fc.GUARD + self.buf[name].bytes(self.n)]
        return t if dtype is None else t.view(self.tdtype(dtype))

    def tdtype(self, dtype):
        torch = self.torch
        if isinstance(dtype, torch.dtype):
            return dtype
        return {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32,
                np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32}[np.dtype(dtype)]

    def ptr(self, name):
        return self.v(name).data_ptr()

    def images(self, name):
        return self.v(name).view(self.n, self.buf[name].image_bytes)

    # ---- device-side fills and comparisons, a pass of STEP elements at a time ----
    def _steps(self, count):
        return [slice(a, min(a + STEP, count)) for a in range(0, count, STEP)]

    def rand_u8(self, name):
        t = self.v(name)
        for s in self._steps(t.numel()):
            t[s].random_(0, 256)

    def rand_float(self, name, dtype, lo, hi):
        t = self.v(name, dtype)
        for s in self._steps(t.numel()):
            t[s].uniform_(lo, hi)

    def fill(self, name, byte):
        self.v(name).fill_(byte)

    def count_ne(self, a, b):
        """elements of the tensors a and b (one shape, flat) that differ"""
        bad = self.torch.zeros((), dtype=self.torch.int64, device="cuda:0")
        for s in self._steps(a.numel()):
            bad += (a[s] != b[s]).sum()
        return int(bad.item())

    def count_ne_const(self, name, value):
        t = self.v(name)
        bad = self.torch.zeros((), dtype=self.torch.int64, device="cuda:0")
        for s in self._steps(t.numel()):
            bad += (t[s] != value).sum()
        return int(bad.item())

    def count_eq_const(self, name, value):
        return self.v(name).numel() - self.count_ne_const(name, value)

    def image_steps(self, elems_per_image):
        per = max(1, STEP // elems_per_image)
        return [slice(a, min(a + per, self.n)) for a in range(0, self.n, per)]

    def rows(self, name, s, row, stride, image_stride, H=None):
        """images s of a strided u8 stack as (len, H, row): the samples without the padding"""
        H = H or self.H
        t = self.v(name).view(self.n, image_stride)[s]
        return t[:, :H * stride].view(t.shape[0], H, stride)[:, :, :row]

    def count_ne_rows(self, tight, strided, row, stride, image_stride):
        """samples in which the tight stack `tight` differs from the strided stack `strided`"""
        bad = self.torch.zeros((), dtype=self.torch.int64, device="cuda:0")
        for s in self.image_steps(self.H * row):
            bad += (self.rows(tight, s, row, row, self.H * row) != self.rows(strided, s, row, stride, image_stride)).sum()
        return int(bad.item())

    def guards_ok(self):
        for name, raw in self.raw.items():
            nb = self.buf[name].bytes(self.n)
            if not bool((raw[:fc.GUARD] == GUARD_BYTE).all().item() and (raw[fc.GUARD + nb:] == GUARD_BYTE).all().item()):
                return name
        return None

    # ---- the probe images -----------------------------------------------------
    def get(self, name, idx, dtype=np.uint8):
        """images idx of a buffer as a host array (len(idx), image_bytes / itemsize)"""
        i = self.torch.as_tensor(idx, device="cuda:0")
        return self.images(name)[i].cpu().numpy().view(dtype)

    def put(self, name, idx, host):
        i = self.torch.as_tensor(idx, device="cuda:0")
        a = np.ascontiguousarray(host).reshape(len(idx), -1).view(np.uint8)
        self.images(name)[i] = self.torch.from_numpy(a).to("cuda:0")

    def get_rows(self, name, idx, row, stride, image_stride, H=None):
        H = H or self.H
        g = self.get(name, idx)
        return np.ascontiguousarray(g[:, :H * stride].reshape(len(idx), H, stride)[:, :, :row])

    def upload(self, name, host):
        a = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
        self.v(name).copy_(self.torch.from_numpy(a))

    def sync(self):
        self.torch.cuda.synchronize()


def inject(flow):
    """the special vectors into every (H, W, 2) field of a (k, H, W, 2) array, in place"""
    k, H, W, _ = flow.shape
    with np.errstate(over="ignore"):
        sp = np.array([[np.nan, np.nan], [np.inf, 0.5], [0.5, -np.inf], [1e9, 0.0], [-1e9, 1.0], [np.nan, 0.0]]).astype(flow.dtype)
    at = [(0, 0), (1 % H, 2 % W), (2 % H, 1 % W), (3 % H, 3 % W), (H - 1, W - 1), (H // 2, W // 2)]
    for (y, x), val in zip(at, sp):
        flow[:, y, x] = val
    return flow


def same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.size == exp.size, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    g, e = got.reshape(-1).view(np.uint8), exp.reshape(-1).view(np.uint8)
    if not np.array_equal(g, e):
        bad = np.flatnonzero(g != e)
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at byte {int(bad[0])} of the probe images")


def src_strides(case, C, pad):
    """(stride, image_stride, arguments for the entry point) of a source stack"""
    if pad:
        stride, image_stride, _ = fc.padded_u8("src", case, C)
        return stride, image_stride, (stride, image_stride)
    return case.W * C, case.W * C * case.H, (0, 0)


def stack_of(name, rows, row, pad):
    """(stride, image_stride, the two stride arguments) of a u8 stack, tight or padded as farcases plans it"""
    stride, image_stride, _ = fc.strided(name, rows, row, pad)
    return stride, image_stride, ((stride, image_stride) if pad else (0, 0))


def images_of(rows, C):
    """(k, H, W * C) samples as the restatements take them: (k, H, W) or (k, H, W, C)"""
    k, H, WC = rows.shape
    return rows.reshape(k, H, WC) if C == 1 else rows.reshape(k, H, WC // C, C)


def random_models(case, k8, seed):
    """(n, 6 or 8) float32 models near the identity, one per image, with the specials in a few"""
    rng = np.random.default_rng(seed)
    p = np.zeros((case.n, k8), np.float32)
    p[:, [0, 3]] = rng.uniform(-3.0, 3.0, (case.n, 2))
    p[:, [1, 2, 4, 5]] = rng.uniform(-0.01, 0.01, (case.n, 4))
    if k8 == 8:
        p[:, 6:] = rng.uniform(-1e-5, 1e-5, (case.n, 2))
    return p


def special_models(p, probes):
    """NaN, inf and out-of-range models into four of the probe images (not the ends)"""
    mid = probes[2:-2]
    p[mid[0], 0] = np.nan
    p[mid[1], 4] = np.inf
    p[mid[2], 0] = 1e9
    p[mid[3], 3] = -2e9
    return p


def translations(case, dtype):
    """(n, 2) per-image translations, exact in float16, no two consecutive images alike"""
    i = np.arange(case.n)
    return np.stack([(i % 2048 - 1024) / 8.0, (i // 2048 - 16) / 8.0 + 0.125], 1).astype(np.float32)


# ---- the entry points ------------------------------------------------------------


def far_flow_warp_u8(d, dev, variant, probes):
    dt, C, pad = variant
    W, H, n = dev.W, dev.H, dev.n
    stride, istride, sarg = src_strides(dev.case, C, pad)

    def call():
        d.flow_warp_device(dev.ptr("src"), dev.ptr("flow"), dt, n, W, H, C, dev.ptr("dst"), dev.ptr("valid"), scale=1.0,
                           border="replicate", src_stride=sarg[0], src_image_stride=sarg[1])
        dev.sync()
    # identity: zero flow -> src
    dev.rand_u8("src")
    dev.v("flow").zero_()
    dev.fill("dst", DST_FILL)
    dev.fill("valid", UNSET)
    call()
    assert dev.count_ne_rows("dst", "src", W * C, stride, istride) == 0, "zero flow: dst differs from src"
    assert dev.count_ne_const("valid", 255) == 0, "zero flow: valid is not 255 everywhere"
    # probes
    dev.rand_float("flow", dt, -4.0, 4.0)
    fl = inject(dev.get("flow", probes, dt).reshape(-1, H, W, 2).copy())
    dev.put("flow", probes, fl)
    dev.fill("dst", DST_FILL)
    dev.fill("valid", UNSET)
    call()
    assert dev.count_eq_const("valid", UNSET) == 0, "valid keeps prefilled bytes"
    img = images_of(dev.get_rows("src", probes, W * C, stride, istride), C)
    exp, ev = warpref.warp(img, fl, 1.0, warpref.REPLICATE)
    same_bits(dev.get("dst", probes), exp, "dst")
    same_bits(dev.get("valid", probes), ev, "valid")


def _far_warp_model(d, dev, variant, probes, k8):
    C, pad = variant
    W, H, n = dev.W, dev.H, dev.n
    stride, istride, sarg = src_strides(dev.case, C, pad)
    fn = d.warp_motion_device if k8 == 6 else d.warp_homography_device
    ref = stabref.warp if k8 == 6 else homographyref.warp

    def call():
        fn(dev.ptr("src"), dev.ptr("params"), n, W, H, C, dev.ptr("dst"), dev.ptr("valid"), border="replicate",
           src_stride=sarg[0], src_image_stride=sarg[1])
        dev.sync()
    # identity: the zero model (no motion) -> src
    dev.rand_u8("src")
    dev.v("params").zero_()
    dev.fill("dst", DST_FILL)
    dev.fill("valid", UNSET)
    call()
    assert dev.count_ne_rows("dst", "src", W * C, stride, istride) == 0, "identity model: dst differs from src"
    assert dev.count_ne_const("valid", 255) == 0, "identity model: valid is not 255 everywhere"
    # probes: a model per image
    p = special_models(random_models(dev.case, k8, 11), probes)
    dev.upload("params", p)
    dev.fill("dst", DST_FILL)
    dev.fill("valid", UNSET)
    call()
    assert dev.count_eq_const("valid", UNSET) == 0, "valid keeps prefilled bytes"
    img = images_of(dev.get_rows("src", probes, W * C, stride, istride), C)
    exp, ev = ref(img, p[probes], warpref.REPLICATE)
    same_bits(dev.get("dst", probes), exp, "dst")
    same_bits(dev.get("valid", probes), ev, "valid")


def far_warp_motion_u8(d, dev, variant, probes):
    _far_warp_model(d, dev, variant, probes, 6)


def far_warp_homography_u8(d, dev, variant, probes):
    _far_warp_model(d, dev, variant, probes, 8)


def _far_model_flow(d, dev, variant, probes, k8):
    (dt,) = variant
    torch = dev.torch
    W, H, n, P = dev.W, dev.H, dev.n, dev.P
    fn = d.motion_to_flow_device if k8 == 6 else d.homography_to_flow_device
    ref = motionref.to_flow if k8 == 6 else homographyref.to_flow

    def call():
        fn(dev.ptr("params"), n, W, H, dev.ptr("out"), dt)
        dev.sync()
    # identity: a translation per image -> two constants per image
    tr = translations(dev.case, dt)
    p = np.zeros((n, k8), np.float32)
    p[:, 0], p[:, 3] = tr[:, 0], tr[:, 1]
    dev.upload("params", p)
    dev.fill("out", 0xFF)  # NaN in either format
    call()
    out = dev.v("out", dt).view(n, P, 2)
    want = torch.from_numpy(tr).to("cuda:0").to(dev.tdtype(dt))
    bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for s in dev.image_steps(2 * P):
        bad += (out[s] != want[s][:, None, :]).sum()
    assert int(bad.item()) == 0, "translations: a vector differs from its image's constant"
    # probes: a model per image
    p = special_models(random_models(dev.case, k8, 12), probes)
    dev.upload("params", p)
    dev.fill("out", 0xFF)
    call()
    same_bits(dev.get("out", probes, dt), ref(p[probes], W, H, dt), "out")


def far_motion_to_flow(d, dev, variant, probes):
    _far_model_flow(d, dev, variant, probes, 6)


def far_homography_to_flow(d, dev, variant, probes):
    _far_model_flow(d, dev, variant, probes, 8)


def far_flow_compose(d, dev, variant, probes):
    a_dt, b_dt, o_dt = variant
    torch = dev.torch
    W, H, n, P = dev.W, dev.H, dev.n, dev.P

    def call():
        d.flow_compose_device(dev.ptr("a"), a_dt, dev.ptr("b"), b_dt, n, W, H, dev.ptr("out"), o_dt,
                              valid_out_ptr=dev.ptr("valid_out"))
        dev.sync()
    # identity: b = 0 -> a (in out's format), every pixel valid: a points inwards, 1/16 to 1/2 a pixel
    # (never zero: -0 + 0 is +0, another bit pattern)
    a = dev.v("a", a_dt).view(n, H, W, 2)
    sx = torch.where(torch.arange(W, device="cuda:0") < W // 2, 1.0, -1.0).to(a.dtype)
    sy = torch.where(torch.arange(H, device="cuda:0") < H // 2, 1.0, -1.0).to(a.dtype)
    for s in dev.image_steps(2 * P):
        a[s].uniform_(0.0625, 0.5)
        a[s][..., 0] *= sx[None, None, :]
        a[s][..., 1] *= sy[None, :, None]
    dev.v("b").zero_()
    dev.fill("out", 0xFF)
    dev.fill("valid_out", UNSET)
    call()
    af, of = dev.v("a", a_dt), dev.v("out", o_dt)
    bits = torch.int16 if np.dtype(o_dt).itemsize == 2 else torch.int32
    bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for s in dev._steps(af.numel()):
        bad += (af[s].to(of.dtype).view(bits) != of[s].view(bits)).sum()
    assert int(bad.item()) == 0, "b = 0: out differs from a"
    assert dev.count_ne_const("valid_out", 255) == 0, "b = 0: valid_out is not 255 everywhere"
    # probes
    dev.rand_float("a", a_dt, -4.0, 4.0)
    dev.rand_float("b", b_dt, -4.0, 4.0)
    fa = inject(dev.get("a", probes, a_dt).reshape(-1, H, W, 2).copy())
    fb = inject(dev.get("b", probes, b_dt).reshape(-1, H, W, 2).copy())
    fb[:, H // 3, W // 3] = np.array([np.nan, 1.0], fb.dtype)
    dev.put("a", probes, fa)
    dev.put("b", probes, fb)
    dev.fill("out", 0xFF)
    dev.fill("valid_out", UNSET)
    call()
    assert dev.count_eq_const("valid_out", UNSET) == 0, "valid_out keeps prefilled bytes"
    exp, ev = composeref.compose(fa, fb, None, None, o_dt)
    same_bits(dev.get("out", probes, o_dt), exp, "out")
    same_bits(dev.get("valid_out", probes), ev, "valid_out")


def far_flow_advect_points(d, dev, variant, probes):
    (dt,) = variant
    torch = dev.torch
    W, H, n = dev.W, dev.H, dev.n
    K = fc.ADVECT_POINTS

    def call():
        d.advect_points_device(dev.ptr("flow"), dt, n, W, H, dev.ptr("points"), K, dev.ptr("points_out"), dev.ptr("status"))
        dev.sync()
    # identity: zero flow -> the points themselves (all inside, none -0), every status 255
    pts = dev.v("points", np.float32).view(n, K, 2)
    pts[..., 0].uniform_(0.0, float(W - 1))
    pts[..., 1].uniform_(0.0, float(H - 1))
    pts.clamp_(min=0.0)
    pts[..., 0].clamp_(max=float(W - 1))
    pts[..., 1].clamp_(max=float(H - 1))
    dev.v("flow").zero_()
    dev.fill("points_out", 0xFF)
    dev.fill("status", UNSET)
    call()
    assert dev.count_ne(dev.v("points", torch.int32), dev.v("points_out", torch.int32)) == 0, "zero flow: a point moved"
    assert dev.count_ne_const("status", 255) == 0, "zero flow: status is not 255 everywhere"
    # probes: a random field per image, points inside, outside and NaN
    dev.rand_float("flow", dt, -4.0, 4.0)
    fl = inject(dev.get("flow", probes, dt).reshape(-1, H, W, 2).copy())
    dev.put("flow", probes, fl)
    pp = dev.get("points", probes, np.float32).reshape(-1, K, 2).copy()
    pp[:, 0] = (-0.5, 3.0)
    pp[:, 1] = (float(W - 1), float(H - 1))
    pp[:, 2] = (np.nan, 1.0)
    pp[:, 3] = (float(W), 1.0)
    pp[:, 4] = (0.0, 0.0)
    dev.put("points", probes, pp)
    dev.fill("points_out", 0xFF)
    dev.fill("status", UNSET)
    call()
    assert dev.count_eq_const("status", UNSET) == 0, "status keeps prefilled bytes"
    exp, es = composeref.advect(pp, fl)
    same_bits(dev.get("points_out", probes, np.float32), exp, "points_out")
    same_bits(dev.get("status", probes), es, "status")


def far_flow_fill(d, dev, variant, probes):
    i_dt, o_dt = variant
    torch = dev.torch
    W, H, n = dev.W, dev.H, dev.n
    assert d.flow_fill_workspace(n, W, H) == dev.buf["workspace"].bytes(n)

    def call():
        d.flow_fill_device(dev.ptr("flow"), i_dt, n, W, H, dev.ptr("out"), dev.ptr("workspace"), o_dt,
                           mask_ptr=dev.ptr("mask"), level_ptr=dev.ptr("level"))
        dev.sync()
    # identity: a full mask over valid vectors -> the field itself (in out's format), level 0 everywhere
    dev.rand_float("flow", i_dt, -3.0, 3.0)
    dev.fill("mask", 255)
    dev.fill("out", 0xFF)
    dev.fill("level", UNSET)
    call()
    fi, fo = dev.v("flow", i_dt), dev.v("out", o_dt)
    bits = torch.int16 if np.dtype(o_dt).itemsize == 2 else torch.int32
    bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for s in dev._steps(fi.numel()):
        bad += (fi[s].to(fo.dtype).view(bits) != fo[s].view(bits)).sum()
    assert int(bad.item()) == 0, "full mask: out differs from the field"
    assert dev.count_ne_const("level", 0) == 0, "full mask: level is not 0 everywhere"
    # probes: a third of the vectors untrusted, the specials among them
    m = dev.v("mask")
    for s in dev._steps(m.numel()):
        m[s].random_(0, 3)
    fl = inject(dev.get("flow", probes, i_dt).reshape(-1, H, W, 2).copy())
    dev.put("flow", probes, fl)
    mk = dev.get("mask", probes).reshape(-1, H, W).copy()
    mk[len(mk) // 2] = 0  # one probe field without a trusted vector
    dev.put("mask", probes, mk)
    dev.fill("out", 0xFF)
    dev.fill("level", UNSET)
    call()
    assert dev.count_eq_const("level", UNSET) == 0, "level keeps prefilled bytes"
    exp, el = fillref.fill(fl, mk, o_dt)
    same_bits(dev.get("out", probes, o_dt), exp, "out")
    same_bits(dev.get("level", probes), el, "level")


def _far_fit(d, dev, variant, probes, k8):
    (dt,) = variant
    torch = dev.torch
    W, H, n, P = dev.W, dev.H, dev.n, dev.P
    ws = d.fit_motion_workspace(n, W, H) if k8 == 6 else d.fit_homography_workspace(n, W, H)
    assert ws == dev.buf["workspace"].bytes(n)

    def call(**kw):
        args = (dev.ptr("flow"), dt, n, W, H, dev.ptr("params"), dev.ptr("workspace"))
        rest = dict(mask_ptr=dev.ptr("mask"), info_ptr=dev.ptr("info"), inliers_ptr=dev.ptr("inliers"))
        if k8 == 6:
            d.fit_motion_device(*args, **kw, **rest)
        else:
            d.fit_homography_device(*args, **kw, **rest)
        dev.sync()
    # identity: every field a translation of its own, fully trusted -> the translation, every pixel an inlier
    tr = translations(dev.case, dt)
    fl = dev.v("flow", dt).view(n, P, 2)
    want = torch.from_numpy(tr).to("cuda:0")
    for s in dev.image_steps(2 * P):
        fl[s] = want[s].to(fl.dtype)[:, None, :]
    dev.fill("mask", 255)
    dev.fill("params", 0xFF)
    dev.fill("info", 0xFF)
    dev.fill("inliers", UNSET)
    if k8 == 6:
        call(model="translation", iterations=1, threshold=0.5)
    else:
        call(iterations=1, threshold=0.5)
    assert dev.count_ne_const("inliers", 255) == 0, "translations: a pixel is no inlier"
    got = dev.v("params", np.float32).view(n, k8).cpu().numpy()
    info = dev.v("info", np.int32).view(n, 4).cpu().numpy()
    assert (info == np.array([1, P, P, P], np.int32)).all(), "translations: info is not {1, W*H, W*H, W*H} everywhere"
    if k8 == 6:  # sums of equal values: exact
        exp = np.zeros((n, 6), np.float32)
        exp[:, 0], exp[:, 3] = tr[:, 0], tr[:, 1]
        same_bits(got, exp, "params of the translations")
    else:  # a least-squares fit of 8 parameters to an exact translation: to the rounding of its solve
        assert np.abs(got[:, [0, 3]] - tr).max() < 1e-3 and np.abs(got[:, [1, 2, 4, 5]]).max() < 1e-4 and \
            np.abs(got[:, 6:]).max() < 1e-5, "translations: params are not the translations"
    # probes: noisy fields, two thirds of the vectors trusted, against the restatement
    dev.rand_float("flow", dt, -1.0, 1.0)
    m = dev.v("mask")
    for s in dev._steps(m.numel()):
        m[s].random_(0, 3)
    fp = inject(dev.get("flow", probes, dt).reshape(-1, H, W, 2).copy())
    dev.put("flow", probes, fp)
    mk = dev.get("mask", probes).reshape(-1, H, W).copy()
    mk[len(mk) // 2] = 0  # one probe field without a trusted vector: the fit fails
    dev.put("mask", probes, mk)
    dev.fill("params", 0xFF)
    dev.fill("info", 0xFF)
    dev.fill("inliers", UNSET)
    if k8 == 6:
        call(model="affine", iterations=2, threshold=1.0)
        ep, ei, el = motionref.fit(fp, mk, "affine", 2, 1.0)
    else:
        call(iterations=2, threshold=1.0)
        ep, ei, el = homographyref.fit(fp, mk, 2, 1.0)
    assert dev.count_eq_const("inliers", UNSET) == 0, "inliers keeps prefilled bytes"
    same_bits(dev.get("params", probes, np.float32), np.asarray(ep, np.float32), "params")
    same_bits(dev.get("info", probes, np.uint32), np.asarray(ei, np.uint32), "info")
    same_bits(dev.get("inliers", probes), el, "inliers")


def far_flow_fit_motion(d, dev, variant, probes):
    _far_fit(d, dev, variant, probes, 6)


def far_flow_fit_homography(d, dev, variant, probes):
    _far_fit(d, dev, variant, probes, 8)


def far_temporal_denoise_u8(d, dev, variant, probes):
    dt, C, pad = variant
    W, H, n = dev.W, dev.H, dev.n
    stride, istride, sarg = src_strides(dev.case, C, pad)

    def call(table):
        d.temporal_denoise_device(dev.ptr("cur"), [dev.ptr("neighbour")], [dev.ptr("flow")], dt, n, W, H, C, dev.ptr("dst"),
                                  weights=table, mask_ptrs=[dev.ptr("mask")], support_ptr=dev.ptr("support"),
                                  stride=sarg[0], image_stride=sarg[1])
        dev.sync()
    # identity: all-zero weights -> cur, no neighbour takes part
    dev.rand_u8("cur")
    dev.rand_u8("neighbour")
    dev.rand_float("flow", dt, -4.0, 4.0)
    dev.fill("mask", 255)
    dev.fill("dst", DST_FILL)
    dev.fill("support", UNSET)
    call(np.zeros(256, np.float32))
    assert dev.count_ne_rows("dst", "cur", W * C, stride, istride) == 0, "zero weights: dst differs from cur"
    assert dev.count_ne_const("support", 0) == 0, "zero weights: support is not 0 everywhere"
    # probes: a wide table (random frames differ by ~85 on average), a third of the vectors switched off
    table = d.denoise_weights(60.0)
    m = dev.v("mask")
    for s in dev._steps(m.numel()):
        m[s].random_(0, 3)
    fl = inject(dev.get("flow", probes, dt).reshape(-1, H, W, 2).copy())
    dev.put("flow", probes, fl)
    dev.fill("dst", DST_FILL)
    dev.fill("support", UNSET)
    call(table)
    assert dev.count_eq_const("support", UNSET) == 0, "support keeps prefilled bytes"
    cur = images_of(dev.get_rows("cur", probes, W * C, stride, istride), C)
    nb = images_of(dev.get_rows("neighbour", probes, W * C, stride, istride), C)
    mk = dev.get("mask", probes).reshape(-1, H, W)
    exp, es = denoiseref.denoise(cur, [nb], [fl], table, [mk])
    same_bits(dev.get("dst", probes), exp, "dst")
    same_bits(dev.get("support", probes), es, "support")


def far_flow_interp_u8(d, dev, variant, probes):
    dt, C, pad = variant
    W, H, n = dev.W, dev.H, dev.n
    stride, istride, sarg = stack_of("I0", H, W * C, pad)
    assert d.flow_interp_workspace(n, W, H) == dev.buf["workspace"].bytes(n)

    def call(t):
        d.flow_interp_device(dev.ptr("I0"), dev.ptr("I1"), dev.ptr("fw"), dt, n, W, H, C, t, dev.ptr("dst"),
                             dev.ptr("workspace"), fill_ptr=dev.ptr("fill"), stride=sarg[0], image_stride=sarg[1])
        dev.sync()
    # identity: zero flow at t = 1 -> I1, every pixel a projected vector
    dev.rand_u8("I0")
    dev.rand_u8("I1")
    dev.v("fw").zero_()
    dev.fill("dst", DST_FILL)
    dev.fill("fill", UNSET)
    call(1.0)
    assert dev.count_ne_rows("dst", "I1", W * C, stride, istride) == 0, "t = 1: dst differs from I1"
    assert dev.count_ne_const("fill", 0) == 0, "t = 1: fill is not 0 everywhere"
    # probes
    dev.rand_float("fw", dt, -3.0, 3.0)
    fl = inject(dev.get("fw", probes, dt).reshape(-1, H, W, 2).copy())
    dev.put("fw", probes, fl)
    dev.fill("dst", DST_FILL)
    dev.fill("fill", UNSET)
    call(0.5)
    assert dev.count_eq_const("fill", UNSET) == 0, "fill keeps prefilled bytes"
    i0 = images_of(dev.get_rows("I0", probes, W * C, stride, istride), C)
    i1 = images_of(dev.get_rows("I1", probes, W * C, stride, istride), C)
    exp, ef, _ = interpref.interp(i0, i1, fl, 0.5)
    same_bits(dev.get("dst", probes), exp, "dst")
    same_bits(dev.get("fill", probes), ef, "fill")


def far_flow_color(d, dev, variant, probes):
    import oracle_binding as oracle
    (mode,) = variant
    torch = dev.torch
    W, H, n, P = dev.W, dev.H, dev.n, dev.P
    maxmotion = -1.0 if mode == "automatic" else 5.0

    def call():
        d.flow_color_device(dev.ptr("flow"), n, W, H, dev.ptr("bgr"), maxmotion)
        dev.sync()
    # identity: every field one vector of its own -> one colour an image, the oracle's for that vector (in
    # automatic range a constant field's range is its own radius, as a one-pixel field's is; in fixed range
    # pixels are independent, so one oracle call colours all n vectors)
    vec = np.random.default_rng(13).uniform(-9.0, 9.0, (n, 2)).astype(np.float32)
    fl = dev.v("flow", np.float32).view(n, P, 2)
    dvec = torch.from_numpy(vec).to("cuda:0")
    for s in dev.image_steps(2 * P):
        fl[s] = dvec[s][:, None, :]
    dev.fill("bgr", DST_FILL)
    call()
    if mode == "fixed":
        col = oracle.flow_color(vec.reshape(1, n, 2), maxmotion).reshape(n, 3)
    else:
        col = np.stack([oracle.flow_color(vec[i].reshape(1, 1, 2), maxmotion).reshape(3) for i in range(n)])
    dcol = torch.from_numpy(np.ascontiguousarray(col)).to("cuda:0")
    bgr = dev.v("bgr").view(n, P, 3)
    bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for s in dev.image_steps(3 * P):
        bad += (bgr[s] != dcol[s][:, None, :]).sum()
    assert int(bad.item()) == 0, "constant fields: a pixel differs from its image's colour"
    # probes: random fields, a range of its own in each probe field, the specials
    dev.rand_float("flow", np.float32, -6.0, 6.0)
    fp = dev.get("flow", probes, np.float32).reshape(-1, H, W, 2).copy()
    fp *= np.random.default_rng(14).uniform(0.01, 40.0, (len(probes), 1, 1, 1)).astype(np.float32)
    dev.put("flow", probes, inject(fp))
    dev.fill("bgr", DST_FILL)
    call()
    got = dev.get("bgr", probes).reshape(-1, H, W, 3)
    for k, i in enumerate(probes):
        assert np.array_equal(got[k], oracle.flow_color(fp[k], maxmotion)), f"field {i} differs from the oracle"


def far_flow_consistency(d, dev, variant, probes):
    W, H, n = dev.W, dev.H, dev.n

    def call():  # a field against itself: fw and bw are both only read
        d.flow_consistency_device(dev.ptr("fw"), dev.ptr("fw"), n, W, H, dev.ptr("mask"), dev.ptr("err"), 0.01, 0.5)
        dev.sync()
    # identity: two zero fields -> consistent everywhere, err 0
    dev.v("fw").zero_()
    dev.fill("mask", UNSET)
    dev.fill("err", 0xFF)
    call()
    assert dev.count_ne_const("mask", 255) == 0, "zero fields: mask is not 255 everywhere"
    assert dev.count_ne_const("err", 0) == 0, "zero fields: err is not +0 everywhere"
    # probes
    dev.rand_float("fw", np.float32, -2.0, 2.0)
    fl = inject(dev.get("fw", probes, np.float32).reshape(-1, H, W, 2).copy())
    dev.put("fw", probes, fl)
    dev.fill("mask", UNSET)
    dev.fill("err", 0xFF)
    call()
    assert dev.count_eq_const("mask", UNSET) == 0, "mask keeps prefilled bytes"
    em, ee = fbref.check(fl, fl, 0.01, 0.5)
    same_bits(dev.get("mask", probes), em, "mask")
    same_bits(dev.get("err", probes, np.float32), np.asarray(ee, np.float32), "err")


def far_flow_convert(d, dev, variant, probes):
    s_dt, d_dt = variant
    torch = dev.torch
    n, P = dev.n, dev.P
    count = 2 * n * P
    widen = np.dtype(s_dt).itemsize == 2
    if widen:  # every f16 bit pattern, random
        s16 = dev.v("src", torch.int16)
        for s in dev._steps(s16.numel()):
            s16[s].random_(-32768, 32768)
    else:  # floats across and beyond the f16 range; the probes get the specials and the small values
        dev.rand_float("src", np.float32, -70000.0, 70000.0)
        h = dev.get("src", probes, np.float32).copy()
        h[:, :8] = np.array([np.nan, np.inf, -np.inf, 65519.9, 65520.0, -1e9, 6e-8, -2.98e-8], np.float32)
        h[:, 8:4096] *= np.float32(1e-7)  # f16 subnormals and zeros of either sign
        dev.put("src", probes, h)
    dev.fill("dst", 0x4D)
    d.flow_convert_device(dev.ptr("src"), s_dt, dev.ptr("dst"), d_dt, count)
    dev.sync()
    # identity: the tensor's own conversion (exact when widening, to nearest even when narrowing; a NaN stays a NaN)
    src, dst = dev.v("src", s_dt), dev.v("dst", d_dt)
    bits = torch.int32 if widen else torch.int16
    bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for s in dev._steps(count):
        w = src[s].to(dst.dtype)
        bad += ((w.view(bits) != dst[s].view(bits)) & ~(w.isnan() & dst[s].isnan())).sum()
    assert int(bad.item()) == 0, "a value differs from the tensor's own conversion"
    # probes: numpy's conversion (NaNs compared as NaNs)
    h = dev.get("src", probes, s_dt)
    got = dev.get("dst", probes, d_dt)
    with np.errstate(over="ignore"):
        exp = h.astype(d_dt)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "NaNs of the probe images"
    zero = np.zeros((), d_dt)
    same_bits(np.where(nan, zero, got), np.where(nan, zero, exp), "dst")


def far_frames_to_gray_u8(d, dev, variant, probes):
    C, pad = variant
    W, H, n, P = dev.W, dev.H, dev.n, dev.P
    fmt = "gray" if C == 1 else "bgra"
    stride, istride, sarg = stack_of("src", H, W * C, pad)

    def call():
        d.frames_to_gray_device(dev.ptr("src"), fmt, n, W, H, dev.ptr("dst"), src_stride=sarg[0], src_image_stride=sarg[1])
        dev.sync()

    def pixels(s):  # images s of the source as (len, H, W, C)
        r = dev.rows("src", s, W * C, stride, istride)
        return r.view(r.shape[0], H, W, C)
    # identity: gray frames (C = 4: B = G = R, alpha random) -> the same bytes
    dev.rand_u8("src")
    if C == 4:
        for s in dev.image_steps(P * C):
            pixels(s)[..., 1] = pixels(s)[..., 0]
            pixels(s)[..., 2] = pixels(s)[..., 0]
    dev.fill("dst", DST_FILL)
    call()
    dst = dev.v("dst").view(n, H, W)
    bad = dev.torch.zeros((), dtype=dev.torch.int64, device="cuda:0")
    for s in dev.image_steps(P * C):
        bad += (dst[s] != pixels(s)[..., 0]).sum()
    assert int(bad.item()) == 0, "gray frames: dst differs from the frames"
    # probes: random colours
    dev.rand_u8("src")
    dev.fill("dst", DST_FILL)
    call()
    fr = images_of(dev.get_rows("src", probes, W * C, stride, istride), C)
    same_bits(dev.get("dst", probes), lumaref.to_gray(fr, fmt), "dst")


def far_frames_to_yuv420_u8(d, dev, variant, probes):
    C, pad = variant
    W, H, n, P = dev.W, dev.H, dev.n, dev.P
    fmt = "gray" if C == 1 else "bgra"
    stride, istride, sarg = stack_of("frames", H, W * C, pad)

    def call():
        d.frames_to_yuv420_device(dev.ptr("frames"), fmt, n, W, H, dev.ptr("y"), dev.ptr("cb"), dev.ptr("cr"), 1,
                                  matrix="bt601", range="full", src_stride=sarg[0], src_image_stride=sarg[1])
        dev.sync()

    def pixels(s):  # images s of the frames as (len, H, W, C)
        r = dev.rows("frames", s, W * C, stride, istride)
        return r.view(r.shape[0], H, W, C)
    # identity: gray frames (C = 4: B = G = R) with BT.601 full range -> Y the frames, chroma 128
    dev.rand_u8("frames")
    if C == 4:
        for s in dev.image_steps(P * C):
            pixels(s)[..., 1] = pixels(s)[..., 0]
            pixels(s)[..., 2] = pixels(s)[..., 0]
    for name in ("y", "cb", "cr"):
        dev.fill(name, UNSET)
    call()
    y = dev.v("y").view(n, H, W)
    bad = dev.torch.zeros((), dtype=dev.torch.int64, device="cuda:0")
    for s in dev.image_steps(P * C):
        bad += (y[s] != pixels(s)[..., 0]).sum()
    assert int(bad.item()) == 0, "gray frames: Y differs from the frames"
    assert dev.count_ne_const("cb", 128) == 0 and dev.count_ne_const("cr", 128) == 0, "gray frames: chroma is not 128"
    # probes: random colours
    dev.rand_u8("frames")
    for name in ("y", "cb", "cr"):
        dev.fill(name, UNSET)
    call()
    f = images_of(dev.get_rows("frames", probes, W * C, stride, istride), C)
    ey, ecb, ecr = yuvref.to_yuv420(f, fmt, "bt601", "full")
    same_bits(dev.get("y", probes), ey, "y")
    same_bits(dev.get("cb", probes), ecb, "cb")
    same_bits(dev.get("cr", probes), ecr, "cr")


def far_yuv420_to_frames_u8(d, dev, variant, probes):
    C, pad = variant
    W, H, n, P = dev.W, dev.H, dev.n, dev.P
    fmt = "gray" if C == 1 else "bgra"
    ys, yi, yarg = stack_of("y", H, W, pad)
    cs, ci, carg = stack_of("cb", H // 2, W // 2, pad)

    def call(matrix, range_):
        d.yuv420_to_frames_device(dev.ptr("y"), dev.ptr("cb"), dev.ptr("cr"), 1, n, W, H, dev.ptr("frames"), fmt,
                                  matrix=matrix, range=range_, alpha=200, y_stride=yarg[0], y_image_stride=yarg[1],
                                  c_stride=carg[0], c_image_stride=carg[1])
        dev.sync()
    # identity: neutral chroma with BT.601 full range -> B = G = R = Y (and the alpha)
    dev.rand_u8("y")
    dev.fill("cb", 128)
    dev.fill("cr", 128)
    dev.fill("frames", DST_FILL)
    call("bt601", "full")
    fr = dev.v("frames").view(n, H, W, C)
    bad = dev.torch.zeros((), dtype=dev.torch.int64, device="cuda:0")
    for s in dev.image_steps(P * C):
        y = dev.rows("y", s, W, ys, yi)
        for k in range(min(C, 3)):
            bad += (fr[s][..., k] != y).sum()
        if C == 4:
            bad += (fr[s][..., 3] != 200).sum()
    assert int(bad.item()) == 0, "neutral chroma: the frames differ from Y"
    # probes: random chroma, the limited range
    dev.rand_u8("cb")
    dev.rand_u8("cr")
    dev.fill("frames", DST_FILL)
    call("bt709", "limited")
    py = dev.get_rows("y", probes, W, ys, yi)
    pcb = dev.get_rows("cb", probes, W // 2, cs, ci, H // 2)
    pcr = dev.get_rows("cr", probes, W // 2, cs, ci, H // 2)
    exp = yuvref.to_frames(py, None if C == 1 else pcb, None if C == 1 else pcr, fmt, "bt709", "limited", 200)
    same_bits(dev.get("frames", probes), exp, "frames")


@pytest.mark.parametrize("entry,variant,case", PLANS, ids=IDS)
def test_far(disflow_mod, entry, variant, case):
    import torch
    t0 = time.perf_counter()
    bufs = fc.plan(entry, variant, case)
    probes = fc.probe_images(case, bufs)
    dev = Dev(torch, case, bufs)
    try:
        globals()["far_" + entry](disflow_mod, dev, variant, probes)
        assert dev.guards_ok() is None, f"the guard zones of {dev.guards_ok()} were written"
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        assert peak <= fc.MEMORY_CAP, f"held {peak} bytes of device memory"
        print(f"\nFAR {entry} {fc.variant_id(variant)} {case.name}: {time.perf_counter() - t0:.3f} s, "
              f"peak {peak / fc.GIB:.2f} GiB, {len(probes)} probe images")
    finally:
        dev.close()
        del dev


# ---- dis_flow_color with more fields than a launch's y extent ------------------------


@pytest.fixture(scope="module")
def color_fields():
    """COLOR.n random 16 x 8 fields, no two alike, the specials in the probe fields"""
    c = fc.COLOR
    rng = np.random.default_rng(fc.SEED)
    flow = rng.uniform(-6.0, 6.0, (c.n, c.H, c.W, 2)).astype(np.float32)
    flow *= rng.uniform(0.01, 40.0, (c.n, 1, 1, 1)).astype(np.float32)  # a range of its own per field
    probes = fc.probe_images(c, fc.plan("flow_color", (), c))
    probes = sorted(set(probes) | {65534, 65535, 65536, 65537})  # around the y extent of a launch
    flow[probes] = inject(flow[probes])
    return flow, probes


@pytest.mark.parametrize("maxmotion", [-1.0, 5.0], ids=["automatic", "fixed"])
def test_flow_color_many_fields(disflow_mod, oracle, color_fields, maxmotion):
    """n = 65,539 fields in one call, in both range modes: the probe fields against
    the oracle, and every field against the same call made in slices of 4,096
    fields (launches the y extent has always held)."""
    flow, probes = color_fields
    t0 = time.perf_counter()
    got = disflow_mod.flow_color(flow, maxmotion)
    assert got.shape == flow.shape[:3] + (3,)
    for i in probes:
        exp = oracle.flow_color(flow[i], maxmotion)
        assert np.array_equal(got[i], exp), f"field {i} differs from the oracle"
    for a in range(0, len(flow), 4096):
        part = disflow_mod.flow_color(flow[a:a + 4096], maxmotion)
        assert np.array_equal(got[a:a + 4096], part), f"fields {a}.. differ from the call in slices"
    print(f"\nFAR flow_color many fields {maxmotion}: {time.perf_counter() - t0:.3f} s")
