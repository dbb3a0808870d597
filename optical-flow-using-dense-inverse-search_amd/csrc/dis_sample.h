// dis_sample.h -- the bilinear sampler of u8 images that dis_warp.hip,
// dis_interp.hip and dis_denoise.hip share, and dis_interp.hip's loads of a lane's four flow
// vectors (k_flow_warp keeps its own copy of those: calling load_flow4 there
// changes its emitted code, calling warp_pixel from here does not).
//
// warp_pixel is steps 1-5 of dis_flow_warp_u8 (include/dis_abi.h). Every tap
// index is formed after the invalid test and the clamp, so it lies in the frame
// for every input; every float operation is separately rounded
// (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dis_half.h"

namespace dis {

// One pixel: S = this pixel's source image, (u, v) its flow vector. Writes the
// C channels to o[] and returns 255 when the target lies inside the frame,
// else 0. Out = unsigned: the output bytes (rintf, ties to even, clamped to
// [0, 255]); Out = float: the unrounded sums. vec_tap (4 channels only): S and
// the stride are 4-byte aligned, one dword per tap.
template <int C, class Out>
__device__ __forceinline__ unsigned warp_pixel(const uint8_t* __restrict__ S, long long stride, int x, int y, int W,
                                               int H, float u, float v, float scale, int zero_border, int vec_tap,
                                               Out* o)
{
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0u;
    if (!(fabsf(u) < 1e9f && fabsf(v) < 1e9f)) return 0u;  // also NaN
    const float su = scale * u, sv = scale * v;
    float px = (float)x + su, py = (float)y + sv;  // finite: |scale| <= 1024
    const float xm = (float)(W - 1), ym = (float)(H - 1);
    const bool inside = px >= 0.0f && px <= xm && py >= 0.0f && py <= ym;
    if (!inside) {
        if (zero_border) return 0u;
        px = fminf(fmaxf(px, 0.0f), xm);
        py = fminf(fmaxf(py, 0.0f), ym);
    }
    const float x0 = floorf(px), y0 = floorf(py);
    const float a = px - x0, b = py - y0;
    const int ix0 = (int)x0, iy0 = (int)y0;  // in [0, W-1] x [0, H-1]
    const int ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);
    const float ia = 1.0f - a, ib = 1.0f - b;
    const float w00 = ia * ib, w01 = a * ib, w10 = ia * b, w11 = a * b;
    const uint8_t* const r0 = S + iy0 * stride;
    const uint8_t* const r1 = S + iy1 * stride;
    unsigned t00[C], t01[C], t10[C], t11[C];
    if (C == 4 && vec_tap) {
        const unsigned d00 = *reinterpret_cast<const unsigned*>(r0 + 4 * ix0);
        const unsigned d01 = *reinterpret_cast<const unsigned*>(r0 + 4 * ix1);
        const unsigned d10 = *reinterpret_cast<const unsigned*>(r1 + 4 * ix0);
        const unsigned d11 = *reinterpret_cast<const unsigned*>(r1 + 4 * ix1);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            t00[c] = (d00 >> (8 * c)) & 255u;
            t01[c] = (d01 >> (8 * c)) & 255u;
            t10[c] = (d10 >> (8 * c)) & 255u;
            t11[c] = (d11 >> (8 * c)) & 255u;
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            t00[c] = r0[C * ix0 + c];
            t01[c] = r0[C * ix1 + c];
            t10[c] = r1[C * ix0 + c];
            t11[c] = r1[C * ix1 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float s = ((w00 * (float)t00[c] + w01 * (float)t01[c]) + w10 * (float)t10[c]) + w11 * (float)t11[c];
        if constexpr (std::is_same<Out, float>::value)
            o[c] = s;
        else
            o[c] = (unsigned)fminf(fmaxf(rintf(s), 0.0f), 255.0f);
    }
    return inside ? 255u : 0u;
}

__device__ __forceinline__ unsigned pack4(const unsigned* b) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

// The m (1..4) flow vectors from pixel p0 on, widened to float2. vec: 16-byte
// loads (f32: `flow` 16-byte aligned and W even, taken when m == 4; f16: `flow`
// 16-byte aligned and W % 4 == 0, so m == 4 and p0 is a multiple of 4).
template <bool F16>
__device__ __forceinline__ void load_flow4(const void* __restrict__ flow, long long p0, int m, int vec, float2* q)
{
    if constexpr (F16) {
        const __half2* const fl = static_cast<const __half2*>(flow) + p0;
        if (vec) {
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
        const float2* const fl = static_cast<const float2*>(flow) + p0;
        if (vec && m == 4) {
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
}

}  // namespace dis
