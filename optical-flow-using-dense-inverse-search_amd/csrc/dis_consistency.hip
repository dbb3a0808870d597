// dis_consistency.hip -- forward-backward consistency of flow fields
// (dis_flow_consistency, include/dis_abi.h). No reference counterpart: the
// reference computes one direction and never checks it.
//
// For pixel (x, y) with fw(x, y) = (u, v) the backward field is sampled
// bilinearly at (x + u, y + v); the vector is consistent when following it and
// the backward vector found there leads back:
//   |fw + bw(x + fw)|^2 <= alpha1 * (|fw|^2 + |bw(x + fw)|^2) + alpha2.
// Targets outside the frame (and NaN vectors) give mask 0 and err +inf. Every
// float operation is separately rounded (-ffp-contract=off), in the order
// written in fb_pixel, so tests/fbref.py restates it bit for bit.
//
// Bandwidth-bound: 8 B of fw and ~8 B of bw read, 1 B (+ 4 B) written per
// pixel. Each lane owns 4 consecutive pixels of a row: two 16-byte fw loads,
// 8-byte bw taps, one dword of mask and one 16-byte err store when pointers
// and W allow (chosen at run time, as k_output's vec_store); no LDS, no
// atomics.
#include <cmath>
#include <cstdint>

#include "dis_kernels.h"

namespace dis {
namespace {

constexpr int kFbThreads = 256;

struct FbArgs {
    const float2* fw;
    const float2* bw;
    uint8_t* mask;
    float* err;  // may be null
    long long items;  // n * H * cw lanes of work
    int W, H, cw;     // cw = ceil(W / 4) lanes per row
    float alpha1, alpha2;
    int vec_fw;    // fw 16-byte aligned and W even: float4 loads of a lane's pixel pairs
    int vec_mask;  // mask 4-byte aligned and W % 4 == 0: one dword per lane
    int vec_err;   // err 16-byte aligned and W % 4 == 0: one float4 per lane
};

// One pixel: B = the backward field of this pixel's frame, (u, v) its forward
// vector. Returns the mask byte, *err the squared round-trip distance.
__device__ __forceinline__ unsigned fb_pixel(const float2* __restrict__ B, int x, int y, int W, int H, float u,
                                             float v, float alpha1, float alpha2, float* err)
{
    const float px = (float)x + u, py = (float)y + v;
    if (!(px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1))) {  // also NaN
        *err = INFINITY;
        return 0u;
    }
    const float x0 = floorf(px), y0 = floorf(py);
    const float a = px - x0, b = py - y0;
    const int ix0 = (int)x0, iy0 = (int)y0;
    const int ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);
    const float ia = 1.0f - a, ib = 1.0f - b;
    const float w00 = ia * ib, w01 = a * ib, w10 = ia * b, w11 = a * b;
    const float2 b00 = B[(long long)iy0 * W + ix0], b01 = B[(long long)iy0 * W + ix1];
    const float2 b10 = B[(long long)iy1 * W + ix0], b11 = B[(long long)iy1 * W + ix1];
    const float su = ((w00 * b00.x + w01 * b01.x) + w10 * b10.x) + w11 * b11.x;
    const float sv = ((w00 * b00.y + w01 * b01.y) + w10 * b10.y) + w11 * b11.y;
    const float dx = u + su, dy = v + sv;
    const float e = dx * dx + dy * dy;
    const float thr = alpha1 * ((u * u + v * v) + (su * su + sv * sv)) + alpha2;
    *err = e;
    return e <= thr ? 255u : 0u;
}

__global__ void __launch_bounds__(kFbThreads) k_fb_check(FbArgs a)
{
    const long long t = (long long)blockIdx.x * kFbThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // field * H + y
    const int x0 = (int)(t - row * a.cw) * 4;
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const long long p0 = row * a.W + x0;  // first pixel of this lane
    const float2* const B = a.bw + f * a.H * (long long)a.W;
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    float2 q[4];
    if (a.vec_fw && m == 4) {  // (W even: p0 is, so both loads are 16-byte aligned)
        const float4* const v = reinterpret_cast<const float4*>(a.fw + p0);
        const float4 lo = v[0], hi = v[1];
        q[0] = make_float2(lo.x, lo.y);
        q[1] = make_float2(lo.z, lo.w);
        q[2] = make_float2(hi.x, hi.y);
        q[3] = make_float2(hi.z, hi.w);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) q[i] = a.fw[p0 + i];
    }
    float e[4];
    unsigned mk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[i] = 0.0f;
        mk[i] = 0u;
        if (i < m) mk[i] = fb_pixel(B, x0 + i, y, a.W, a.H, q[i].x, q[i].y, a.alpha1, a.alpha2, &e[i]);
    }
    if (a.vec_mask) {  // (W % 4 == 0: m == 4)
        *reinterpret_cast<unsigned*>(a.mask + p0) = mk[0] | (mk[1] << 8) | (mk[2] << 16) | (mk[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.mask[p0 + i] = (uint8_t)mk[i];
    }
    if (!a.err) return;
    if (a.vec_err) {
        *reinterpret_cast<float4*>(a.err + p0) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.err[p0 + i] = e[i];
    }
}

}  // namespace

static_assert(kFbThreads == kFlatThreads, "flow_consistency_blocks (dis_args.h) counts blocks of 256 lanes");

hipError_t launch_flow_consistency(const float* fw, const float* bw, int n, int W, int H, float alpha1,
                                   float alpha2, uint8_t* mask, float* err, hipStream_t s, Timing t)
{
    FbArgs a{};
    a.fw = reinterpret_cast<const float2*>(fw);
    a.bw = reinterpret_cast<const float2*>(bw);
    a.mask = mask;
    a.err = err;
    a.W = W;
    a.H = H;
    a.cw = (W + 3) / 4;
    a.items = (long long)n * H * a.cw;
    a.alpha1 = alpha1;
    a.alpha2 = alpha2;
    a.vec_fw = ((reinterpret_cast<uintptr_t>(fw) & 15) == 0 && (W & 1) == 0) ? 1 : 0;
    a.vec_mask = ((reinterpret_cast<uintptr_t>(mask) & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    a.vec_err = (err && (reinterpret_cast<uintptr_t>(err) & 15) == 0 && (W & 3) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)flow_consistency_blocks(n, W, H);
    DIS_LAUNCH(t, k_fb_check, dim3(grid), dim3(kFbThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dis
