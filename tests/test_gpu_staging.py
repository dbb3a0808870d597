"""GPU tests of host-pointer staging through the raw C-ABI, where the CPU tests
cannot see: padded source stacks through warp and interpolation with the
optional buffers present and absent, and one context's shared staging buffers
across bidirectional, warm-started and plain calls. Every result is compared
bit for bit with the same call on device pointers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the smallest stack with a ragged row, a second image and both kinds of padding
N, W, H, C = 2, 37, 5, 3
STRIDE = W * C + 5
IMAGE_STRIDE = STRIDE * H + 7
EXTENT = (N - 1) * IMAGE_STRIDE + (H - 1) * STRIDE + W * C  # ends with the last sample
PX = N * W * H


def _stack(seed):
    return np.random.default_rng(seed).integers(0, 256, EXTENT, dtype=np.uint8)


def _flow(seed):
    return np.random.default_rng(seed).uniform(-6, 6, (N, H, W, 2)).astype(np.float32)


def _dev(torch, a):
    return torch.from_numpy(a).to("cuda:0")


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    assert np.array_equal(got, exp), f"{what}: {int((got != exp).sum())} of {got.size} values differ"


@pytest.mark.parametrize("optional", [True, False], ids=["all optional buffers", "no optional buffer"])
def test_warp_padded_host_stack_equals_the_device_call(disflow_mod, optional):
    import torch
    S, L = disflow_mod, disflow_mod.lib()
    src, flow = _stack(1), _flow(2)
    dst, valid = np.full(PX * C, 9, np.uint8), np.full(PX, 9, np.uint8)
    st = L.dis_flow_warp_u8(src.ctypes.data, STRIDE, IMAGE_STRIDE, C, flow.ctypes.data, S.FLOW_F32, N, W, H, 1.0,
                            S.BORDER_ZERO, dst.ctypes.data, valid.ctypes.data if optional else None, S.MEM_HOST, None, 0)
    assert st == S.DIS_OK, L.dis_last_error()
    tsrc, tflow = _dev(torch, src), _dev(torch, flow)
    tdst = torch.full((PX * C,), 9, dtype=torch.uint8, device="cuda:0")
    tvalid = torch.full((PX,), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = L.dis_flow_warp_u8(tsrc.data_ptr(), STRIDE, IMAGE_STRIDE, C, tflow.data_ptr(), S.FLOW_F32, N, W, H, 1.0,
                            S.BORDER_ZERO, tdst.data_ptr(), tvalid.data_ptr() if optional else None, S.MEM_DEVICE,
                            None, 0)
    assert st == S.DIS_OK, L.dis_last_error()
    torch.cuda.synchronize()
    _same(dst, tdst.cpu().numpy(), "dst")
    _same(valid, tvalid.cpu().numpy(), "valid")  # (both untouched when not asked for)
    assert (valid == 9).all() != optional
    assert (dst != 9).any() and (dst == 0).any()  # something was warped, and something left the frame


@pytest.mark.parametrize("optional", [True, False], ids=["all optional buffers", "no optional buffer"])
def test_interp_padded_host_stack_equals_the_device_call(disflow_mod, optional):
    import torch
    S, L = disflow_mod, disflow_mod.lib()
    I0, I1, fw, bw = _stack(3), _stack(4), _flow(5), _flow(6)
    dst, fill = np.full(PX * C, 9, np.uint8), np.full(PX, 9, np.uint8)
    st = L.dis_flow_interp_u8(I0.ctypes.data, I1.ctypes.data, STRIDE, IMAGE_STRIDE, C, fw.ctypes.data,
                              bw.ctypes.data if optional else None, S.FLOW_F32, N, W, H, 0.4, dst.ctypes.data,
                              fill.ctypes.data if optional else None, None, S.MEM_HOST, None, 0)
    assert st == S.DIS_OK, L.dis_last_error()
    t0, t1, tfw, tbw = (_dev(torch, a) for a in (I0, I1, fw, bw))
    tdst = torch.full((PX * C,), 9, dtype=torch.uint8, device="cuda:0")
    tfill = torch.full((PX,), 9, dtype=torch.uint8, device="cuda:0")
    tws = torch.empty(S.flow_interp_workspace(N, W, H) // 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = L.dis_flow_interp_u8(t0.data_ptr(), t1.data_ptr(), STRIDE, IMAGE_STRIDE, C, tfw.data_ptr(),
                              tbw.data_ptr() if optional else None, S.FLOW_F32, N, W, H, 0.4, tdst.data_ptr(),
                              tfill.data_ptr() if optional else None, tws.data_ptr(), S.MEM_DEVICE, None, 0)
    assert st == S.DIS_OK, L.dis_last_error()
    torch.cuda.synchronize()
    _same(dst, tdst.cpu().numpy(), "dst")
    _same(fill, tfill.cpu().numpy(), "fill")  # (both untouched when not asked for)
    assert (fill == 9).all() != optional
    assert (dst != 9).any()


def test_one_context_stages_bidir_warm_and_plain_host_calls(disflow_mod):
    # the bidirectional and the warm-started host calls share one pair of staging
    # buffers: each call in turn against the same call on device pointers on a
    # second context
    import torch
    S, L = disflow_mod, disflow_mod.lib()
    w, h, B = 64, 48, 3
    p = S.Params(coarsest_scale=2, finest_scale=0)
    pairs = [S.synth_pair(40 + k, w, h) for k in range(B)]
    I0 = np.stack([a for a, _ in pairs])
    I1 = np.stack([b for _, b in pairs])
    t0, t1 = _dev(torch, I0), _dev(torch, I1)
    host, dev = S.DenseInverseSearch(p, w, h, max_batch=B), S.DenseInverseSearch(p, w, h, max_batch=B)

    def flows(n):
        return np.full((n, h, w, 2), np.nan, np.float32), torch.full((n, h, w, 2), float("nan"), device="cuda:0")

    def ok(st):
        assert st == S.DIS_OK, L.dis_last_error()

    def same(a, t, what):
        torch.cuda.synchronize()
        _same(a.view(np.uint32), t.cpu().numpy().view(np.uint32), what)

    try:
        fw, tfw = flows(3)
        bw, tbw = flows(3)
        ok(L.dis_calc_bidir_batch_u8(host._ctx, 3, I0.ctypes.data, I1.ctypes.data, 0, 0, fw.ctypes.data,
                                     bw.ctypes.data, S.MEM_HOST, None))
        ok(L.dis_calc_bidir_batch_u8(dev._ctx, 3, t0.data_ptr(), t1.data_ptr(), 0, 0, tfw.data_ptr(), tbw.data_ptr(),
                                     S.MEM_DEVICE, None))
        same(fw, tfw, "1. bidirectional n = 3, forward")
        same(bw, tbw, "1. bidirectional n = 3, backward")
        assert np.isfinite(fw).all() and np.isfinite(bw).all() and not np.array_equal(fw, bw)

        warm, twarm = flows(2)
        ok(L.dis_calc_batch_init_u8(host._ctx, 2, I0.ctypes.data, I1.ctypes.data, 0, 0, fw.ctypes.data,
                                    S.INIT_FULLRES, warm.ctypes.data, S.MEM_HOST, None))
        ok(L.dis_calc_batch_init_u8(dev._ctx, 2, t0.data_ptr(), t1.data_ptr(), 0, 0, tfw.data_ptr(), S.INIT_FULLRES,
                                    twarm.data_ptr(), S.MEM_DEVICE, None))
        same(warm, twarm, "2. warm start n = 2 from the previous forward flow")
        assert np.isfinite(warm).all()

        fw1, tfw1 = flows(1)
        bw1, tbw1 = flows(1)
        ok(L.dis_calc_bidir_batch_u8(host._ctx, 1, I0[2].ctypes.data, I1[2].ctypes.data, 0, 0, fw1.ctypes.data,
                                     bw1.ctypes.data, S.MEM_HOST, None))
        ok(L.dis_calc_bidir_batch_u8(dev._ctx, 1, t0[2].data_ptr(), t1[2].data_ptr(), 0, 0, tfw1.data_ptr(),
                                     tbw1.data_ptr(), S.MEM_DEVICE, None))
        same(fw1, tfw1, "3. bidirectional n = 1, forward")
        same(bw1, tbw1, "3. bidirectional n = 1, backward")

        plain, tplain = flows(3)
        ok(L.dis_calc_batch_u8(host._ctx, 3, I0.ctypes.data, I1.ctypes.data, 0, 0, plain.ctypes.data, S.MEM_HOST, None))
        ok(L.dis_calc_batch_u8(dev._ctx, 3, t0.data_ptr(), t1.data_ptr(), 0, 0, tplain.data_ptr(), S.MEM_DEVICE, None))
        same(plain, tplain, "4. plain n = 3")
    finally:
        torch.cuda.synchronize()
        host.close()
        dev.close()
