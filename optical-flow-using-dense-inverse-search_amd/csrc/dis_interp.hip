// dis_interp.hip -- the frame between I0 and I1 at time t (dis_flow_interp_u8,
// include/dis_abi.h): the Middlebury interpolation algorithm (Baker et al.,
// IJCV 2011, section 3.3). No reference counterpart.
//
// k_interp_splat projects the forward flow to time t: every source pixel of I0
// whose vector is valid and whose target (x + u, y + v) lies in the frame
// offers itself to the up to four pixels around (x + t*u, y + t*v) with the key
//   bits(cost) << 32 | (y*W + x),  cost = sum_c |I0_c(x, y) - I1_c(x + u, y + v)|,
// by a 64-bit atomicMin (relaxed, agent scope, result unused) on the workspace,
// which the launcher has set to ~0. The bits of a non-negative float order as
// unsigned integers, so the minimum is the photoconsistent candidate, the lower
// source index among equal costs; keys of different sources differ, and a
// minimum does not depend on the order of arrival: every run leaves the same
// bytes. k_interp_blend reads each pixel's key, takes the winner's vector (or,
// in a hole, the backward flow's or the forward flow's own vector there) and
// samples both frames with dis_sample.h's warp_pixel, the warp's sampler.
// Every float operation is separately rounded (-ffp-contract=off), so
// tests/interpref.py restates both kernels bit for bit.
//
// A lane of the splat owns one source pixel, so that the lanes of a wave send
// their keys to consecutive targets wherever the flow is smooth: the atomics
// leave the L2 as 64-byte requests, and with 4 pixels per lane each request
// carried two keys where it now carries eight (2.7 times the splat's time on 32
// 1080p pairs). A lane of the blend owns 4 consecutive pixels of
// a row, as k_flow_warp's do, with the same run-time choice between vector and
// scalar loads and stores (the scalar forms write the same bytes). Target
// coordinates are tested against the frame as floats before they become
// indices; tap indices are warp_pixel's. No LDS.
#include <cmath>
#include <cstdint>

#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kInterpThreads = 256;
constexpr unsigned long long kNoKey = ~0ull;

struct InterpArgs {
    const uint8_t* I0;
    const uint8_t* I1;
    const void* fw;  // float2 or __half2 vectors
    const void* bw;  // the same, or null
    unsigned long long* keys;  // n * W * H
    uint8_t* dst;
    uint8_t* fill;     // may be null
    long long items;   // n * H * cw lanes of work
    long long wh;      // W * H
    long long pixels;  // n * W * H lanes of the splat
    long long stride, image_stride;  // bytes, of I0 and I1
    int W, H, cw;      // cw = ceil(W / 4) lanes per row
    float t, tb;       // tb = 1 - t
    int vec_flow;      // fw (and bw) 16-byte aligned and W even (f16: W % 4 == 0): 16-byte loads of a lane's vectors
    int vec_tap;       // 4 channels: I0, I1 and both strides 4-byte aligned, one dword per tap
    int vec_key;       // keys 16-byte aligned and W even: two 16-byte loads of a full lane's keys
    int vec_dst;       // dst 4-byte (4 channels: 16-byte) aligned and W % 4 == 0: dword / 16-byte stores
    int vec_fill;      // fill 4-byte aligned and W % 4 == 0: one dword per lane
};

__device__ __forceinline__ bool valid_vector(float u, float v) { return fabsf(u) < 1e9f && fabsf(v) < 1e9f; }  // false for NaN

template <bool F16>
__device__ __forceinline__ float2 load_flow1(const void* __restrict__ flow, long long p)
{
    if constexpr (F16)
        return widen2(static_cast<const __half2*>(flow)[p]);
    else
        return static_cast<const float2*>(flow)[p];
}

// One source pixel (x, y) of I0 (row A) with its vector (u, v): its key to the
// up to four targets around (x + t*u, y + t*v).
template <int C>
__device__ __forceinline__ void splat_pixel(const InterpArgs& a, const uint8_t* __restrict__ A,
                                            const uint8_t* __restrict__ B, unsigned long long* __restrict__ K, int x,
                                            int y, float u, float v)
{
    const float xm = (float)(a.W - 1), ym = (float)(a.H - 1);
    float s1[C];
    // zero border: an invalid vector or a target outside the frame returns before any tap
    if (!warp_pixel<C>(B, a.stride, x, y, a.W, a.H, u, v, 1.0f, 1, a.vec_tap, s1)) return;
    float cost = fabsf((float)A[C * x] - s1[0]);
#pragma unroll
    for (int c = 1; c < C; ++c) cost = cost + fabsf((float)A[C * x + c] - s1[c]);
    const unsigned long long key = ((unsigned long long)__float_as_uint(cost) << 32) | (unsigned)(y * a.W + x);
    const float tu = a.t * u, tv = a.t * v;
    const float tx = (float)x + tu, ty = (float)y + tv;
    const float fx[2] = {floorf(tx), ceilf(tx)};
    const float fy[2] = {floorf(ty), ceilf(ty)};
    const int nx = fx[1] != fx[0] ? 2 : 1, ny = fy[1] != fy[0] ? 2 : 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (j >= ny || k >= nx) continue;
            if (!(fx[k] >= 0.0f && fx[k] <= xm && fy[j] >= 0.0f && fy[j] <= ym)) continue;
            const long long target = (long long)(int)fy[j] * a.W + (int)fx[k];  // in [0, W*H)
            (void)__hip_atomic_fetch_min(K + target, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int C, bool F16>
__global__ void __launch_bounds__(kInterpThreads) k_interp_splat(InterpArgs a)
{
    const long long p = (long long)blockIdx.x * kInterpThreads + threadIdx.x;  // the source pixel, over all images
    if (p >= a.pixels) return;
    const long long row = p / a.W;  // image * H + y
    const int x = (int)(p - row * a.W);
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const float2 q = load_flow1<F16>(a.fw, p);
    splat_pixel<C>(a, a.I0 + f * a.image_stride + y * a.stride, a.I1 + f * a.image_stride, a.keys + f * a.wh, x, y, q.x,
                   q.y);
}

template <int C, bool F16, bool HAS_BW>
__global__ void __launch_bounds__(kInterpThreads) k_interp_blend(InterpArgs a)
{
    const long long t = (long long)blockIdx.x * kInterpThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // image * H + y
    const int x0 = (int)(t - row * a.cw) * 4;
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const long long p0 = row * a.W + x0;  // first pixel of this lane
    const uint8_t* const A = a.I0 + f * a.image_stride;
    const uint8_t* const B = a.I1 + f * a.image_stride;
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    const float xm = (float)(a.W - 1), ym = (float)(a.H - 1);
    unsigned long long key[4];
    if (a.vec_key && m == 4) {  // (W even: p0 is, so both loads are 16-byte aligned)
        const ulonglong2* const kv = reinterpret_cast<const ulonglong2*>(a.keys + p0);
        const ulonglong2 lo = kv[0], hi = kv[1];
        key[0] = lo.x;
        key[1] = lo.y;
        key[2] = hi.x;
        key[3] = hi.y;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) key[i] = a.keys[p0 + i];
    }
    float2 qb[4];
    if constexpr (HAS_BW) load_flow4<F16>(a.bw, p0, m, a.vec_flow, qb);
    unsigned o[4 * C];  // the lane's output bytes, in store order
    unsigned fd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        fd[i] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) o[C * i + c] = 0u;
        if (i >= m) continue;
        const int x = x0 + i;
        // the vector and the scale of the I1 sample; only_b: a hole filled from I1 alone
        float u = 0.0f, v = 0.0f, sb = a.tb;
        bool only_b = false;
        if (key[i] != kNoKey) {
            const float2 w = load_flow1<F16>(a.fw, f * a.wh + (long long)(key[i] & 0xffffffffull));  // a valid vector
            u = w.x;
            v = w.y;
        } else {
            fd[i] = 2u;
            if constexpr (HAS_BW) {
                const float bu = qb[i].x, bv = qb[i].y;
                if (valid_vector(bu, bv)) {
                    const float px = (float)x + (-a.tb) * bu, py = (float)y + (-a.tb) * bv;
                    if (px >= 0.0f && px <= xm && py >= 0.0f && py <= ym) {
                        only_b = true;
                        fd[i] = 1u;
                        u = bu;
                        v = bv;
                        sb = -a.tb;
                    }
                }
            }
            if (!only_b) {
                const float2 w = load_flow1<F16>(a.fw, p0 + i);
                if (valid_vector(w.x, w.y)) {
                    u = w.x;
                    v = w.y;
                }
            }
        }
        float s0[C], s1[C];
        const unsigned in1 = warp_pixel<C>(B, a.stride, x, y, a.W, a.H, u, v, sb, 0, a.vec_tap, s1);
        if (only_b) {
#pragma unroll
            for (int c = 0; c < C; ++c) o[C * i + c] = (unsigned)fminf(fmaxf(rintf(s1[c]), 0.0f), 255.0f);
            continue;
        }
        const unsigned in0 = warp_pixel<C>(A, a.stride, x, y, a.W, a.H, u, v, -a.t, 0, a.vec_tap, s0);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float both = a.tb * s0[c] + a.t * s1[c];
            const float r = in0 == in1 ? both : (in0 ? s0[c] : s1[c]);
            o[C * i + c] = (unsigned)fminf(fmaxf(rintf(r), 0.0f), 255.0f);
        }
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
    if (!a.fill) return;
    if (a.vec_fill) {
        *reinterpret_cast<unsigned*>(a.fill + p0) = pack4(fd);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.fill[p0 + i] = (uint8_t)fd[i];
    }
}

template <int C, bool F16>
void launch_interp_cf(const InterpArgs& a, unsigned grid, hipStream_t s, Timing ts, Timing tb)
{
    const unsigned splat_grid = (unsigned)((a.pixels + kInterpThreads - 1) / kInterpThreads);
    DIS_LAUNCH(ts, (k_interp_splat<C, F16>), dim3(splat_grid), dim3(kInterpThreads), 0, s, a);
    if (a.bw)
        DIS_LAUNCH(tb, (k_interp_blend<C, F16, true>), dim3(grid), dim3(kInterpThreads), 0, s, a);
    else
        DIS_LAUNCH(tb, (k_interp_blend<C, F16, false>), dim3(grid), dim3(kInterpThreads), 0, s, a);
}

template <int C>
void launch_interp_c(const InterpArgs& a, bool f16, unsigned grid, hipStream_t s, Timing ts, Timing tb)
{
    if (f16)
        launch_interp_cf<C, true>(a, grid, s, ts, tb);
    else
        launch_interp_cf<C, false>(a, grid, s, ts, tb);
}

}  // namespace

hipError_t launch_flow_interp(const uint8_t* I0, const uint8_t* I1, size_t stride, size_t image_stride, int channels,
                              const void* fw, const void* bw, int f16, int n, int W, int H, float t, uint8_t* dst,
                              uint8_t* fill, void* workspace, hipStream_t s, Timing t_splat, Timing t_blend)
{
    static_assert(kInterpThreads == kFlatThreads, "flow_warp_blocks and flow_interp_blocks (dis_args.h) count blocks of 256 lanes");
    const long long blocks = flow_warp_blocks(n, W, H);  // the blend: a lane per 4 pixels of a row, as the warp
    const long long wh = (long long)W * H;
    if (blocks < 1 || flow_interp_blocks(n, W, H) < 1 || wh > (1ll << 31) || (channels != 1 && channels != 3 && channels != 4)) return hipErrorInvalidValue;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(I0), a1 = reinterpret_cast<uintptr_t>(I1);
    const uintptr_t fa = reinterpret_cast<uintptr_t>(fw) | reinterpret_cast<uintptr_t>(bw);
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), la = reinterpret_cast<uintptr_t>(fill);
    const uintptr_t ka = reinterpret_cast<uintptr_t>(workspace);
    InterpArgs a{};
    a.I0 = I0;
    a.I1 = I1;
    a.fw = fw;
    a.bw = bw;
    a.keys = static_cast<unsigned long long*>(workspace);
    a.dst = dst;
    a.fill = fill;
    a.W = W;
    a.H = H;
    a.cw = (W + 3) / 4;
    a.items = (long long)n * H * a.cw;
    a.wh = wh;
    a.pixels = wh * n;
    a.stride = (long long)stride;
    a.image_stride = (long long)image_stride;
    a.t = t;
    a.tb = 1.0f - t;
    a.vec_flow = ((fa & 15) == 0 && (W & (f16 ? 3 : 1)) == 0) ? 1 : 0;
    a.vec_tap = (channels == 4 && ((a0 | a1 | stride | image_stride) & 3) == 0) ? 1 : 0;
    a.vec_key = ((ka & 15) == 0 && (W & 1) == 0) ? 1 : 0;
    a.vec_dst = ((da & (channels == 4 ? 15 : 3)) == 0 && (W & 3) == 0) ? 1 : 0;
    a.vec_fill = (fill && (la & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    const hipError_t e = hipMemsetAsync(workspace, 0xFF, sizeof(unsigned long long) * (size_t)wh * n, s);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)blocks;
    if (channels == 1)
        launch_interp_c<1>(a, f16 != 0, grid, s, t_splat, t_blend);
    else if (channels == 3)
        launch_interp_c<3>(a, f16 != 0, grid, s, t_splat, t_blend);
    else
        launch_interp_c<4>(a, f16 != 0, grid, s, t_splat, t_blend);
    return hipGetLastError();
}

}  // namespace dis
