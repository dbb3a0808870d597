// dis_warp.hip -- backward warp of u8 images by flow fields (dis_flow_warp_u8,
// include/dis_abi.h). No reference counterpart: the reference computes a flow
// and never applies it.
//
// For pixel (x, y) with flow (u, v) the source image is sampled bilinearly at
// (x + scale * u, y + scale * v): dis_consistency.hip's fb_pixel sampler (same
// taps, same weights, same order of sums) on image bytes, rounded to nearest
// even. An invalid vector (NaN or |c| >= 1e9) gives 0; a target outside the
// frame is clamped (DIS_BORDER_REPLICATE) or gives 0 (DIS_BORDER_ZERO). Every
// tap index is formed after the invalid test and the clamp, so it lies in the
// frame for every input. Every float operation is separately rounded
// (-ffp-contract=off), so tests/warpref.py restates it bit for bit.
//
// Each lane owns 4 consecutive pixels of a row: 16-byte flow loads (two for
// f32, one for f16), one dword tap for 4 channels, and dword (1 and 3
// channels) or 16-byte (4 channels) image stores plus one dword of mask, when
// pointers and W allow (chosen at run time, as k_fb_check's forms are); the
// scalar forms write the same bytes. No LDS, no atomics. The per-pixel
// sampler (warp_pixel) lives in dis_sample.h, which dis_interp.hip shares.
#include <cmath>
#include <cstdint>

#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kWarpThreads = 256;

struct WarpArgs {
    const uint8_t* src;
    const void* flow;  // float2 or __half2 vectors
    uint8_t* dst;
    uint8_t* valid;    // may be null
    long long items;   // n * H * cw lanes of work
    long long src_stride, src_image_stride;  // bytes
    int W, H, cw;      // cw = ceil(W / 4) lanes per row
    float scale;
    int zero_border;   // DIS_BORDER_ZERO
    int vec_flow;      // flow 16-byte aligned and W even (f16: W % 4 == 0): 16-byte loads of a lane's vectors
    int vec_tap;       // 4 channels: src and both strides 4-byte aligned, one dword per tap
    int vec_dst;       // dst 4-byte (4 channels: 16-byte) aligned and W % 4 == 0: dword / 16-byte stores
    int vec_valid;     // valid 4-byte aligned and W % 4 == 0: one dword per lane
};

template <int C, bool F16>
__global__ void __launch_bounds__(kWarpThreads) k_flow_warp(WarpArgs a)
{
    const long long t = (long long)blockIdx.x * kWarpThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // image * H + y
    const int x0 = (int)(t - row * a.cw) * 4;
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const long long p0 = row * a.W + x0;  // first pixel of this lane
    const uint8_t* const S = a.src + f * a.src_image_stride;
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    float2 q[4];
    if constexpr (F16) {
        const __half2* const fl = static_cast<const __half2*>(a.flow) + p0;
        if (a.vec_flow) {  // (W % 4 == 0: m == 4, p0 a multiple of 4)
            const uint4 h = *reinterpret_cast<const uint4*>(fl);
            const unsigned w[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __half2 hv;
                __builtin_memcpy(&hv, &w[i], 4);
                q[i] = widen2(hv);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < m) q[i] = widen2(fl[i]);
        }
    } else {
        const float2* const fl = static_cast<const float2*>(a.flow) + p0;
        if (a.vec_flow && m == 4) {  // (W even: p0 is, so both loads are 16-byte aligned)
            const float4* const v = reinterpret_cast<const float4*>(fl);
            const float4 lo = v[0], hi = v[1];
            q[0] = make_float2(lo.x, lo.y);
            q[1] = make_float2(lo.z, lo.w);
            q[2] = make_float2(hi.x, hi.y);
            q[3] = make_float2(hi.z, hi.w);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < m) q[i] = fl[i];
        }
    }
    unsigned o[4 * C];  // the lane's output bytes, in store order
    unsigned vd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        vd[i] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) o[C * i + c] = 0u;
        if (i < m)
            vd[i] = warp_pixel<C>(S, a.src_stride, x0 + i, y, a.W, a.H, q[i].x, q[i].y, a.scale, a.zero_border,
                                  a.vec_tap, &o[C * i]);
    }
    uint8_t* const d = a.dst + p0 * C;
    if (a.vec_dst) {  // (W % 4 == 0: m == 4, p0 * C a multiple of 4, of 16 with 4 channels)
        if constexpr (C == 4) {
            *reinterpret_cast<uint4*>(d) = make_uint4(pack4(o), pack4(o + 4), pack4(o + 8), pack4(o + 12));
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) reinterpret_cast<unsigned*>(d)[k] = pack4(o + 4 * k);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) {
#pragma unroll
                for (int c = 0; c < C; ++c) d[C * i + c] = (uint8_t)o[C * i + c];
            }
    }
    if (!a.valid) return;
    if (a.vec_valid) {
        *reinterpret_cast<unsigned*>(a.valid + p0) = pack4(vd);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.valid[p0 + i] = (uint8_t)vd[i];
    }
}

template <int C>
void launch_warp_c(const WarpArgs& a, bool f16, unsigned grid, hipStream_t s, Timing t)
{
    if (f16)
        DIS_LAUNCH(t, (k_flow_warp<C, true>), dim3(grid), dim3(kWarpThreads), 0, s, a);
    else
        DIS_LAUNCH(t, (k_flow_warp<C, false>), dim3(grid), dim3(kWarpThreads), 0, s, a);
}

}  // namespace

static_assert(kWarpThreads == kFlatThreads, "flow_warp_blocks (dis_args.h) counts blocks of 256 lanes");

hipError_t launch_flow_warp(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                            const void* flow, int f16, int n, int W, int H, float scale, int zero_border,
                            uint8_t* dst, uint8_t* valid, hipStream_t s, Timing t)
{
    const long long blocks = flow_warp_blocks(n, W, H);
    if (blocks < 1 || (channels != 1 && channels != 3 && channels != 4)) return hipErrorInvalidValue;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src), fa = reinterpret_cast<uintptr_t>(flow);
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), va = reinterpret_cast<uintptr_t>(valid);
    WarpArgs a{};
    a.src = src;
    a.flow = flow;
    a.dst = dst;
    a.valid = valid;
    a.W = W;
    a.H = H;
    a.cw = (W + 3) / 4;
    a.items = (long long)n * H * a.cw;
    a.src_stride = (long long)src_stride;
    a.src_image_stride = (long long)src_image_stride;
    a.scale = scale;
    a.zero_border = zero_border;
    a.vec_flow = ((fa & 15) == 0 && (W & (f16 ? 3 : 1)) == 0) ? 1 : 0;
    a.vec_tap = (channels == 4 && ((sa | src_stride | src_image_stride) & 3) == 0) ? 1 : 0;
    a.vec_dst = ((da & (channels == 4 ? 15 : 3)) == 0 && (W & 3) == 0) ? 1 : 0;
    a.vec_valid = (valid && (va & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)blocks;
    if (channels == 1)
        launch_warp_c<1>(a, f16 != 0, grid, s, t);
    else if (channels == 3)
        launch_warp_c<3>(a, f16 != 0, grid, s, t);
    else
        launch_warp_c<4>(a, f16 != 0, grid, s, t);
    return hipGetLastError();
}

}  // namespace dis
