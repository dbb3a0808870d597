// dis_init.hip -- the init plane of a warm-started call (dis_calc_batch_init_u8,
// include/dis_abi.h). No reference counterpart: the reference starts its
// coarsest level from zero (src/patch_grid.cpp:45,80).
//
// A warm-started call behaves as if a level C+1 had produced a dense flow: the
// coarsest level's patches start at 2 * I[ry >> 1][rx >> 1], I the init plane
// of iw x ih = ceil(W_C / 2) x ceil(H_C / 2) float2 in level-(C+1) pixels.
//
// k_flow_to_init makes that plane from a full-resolution W x H flow: extend it
// to the padded frame (replicate), then halve K = C+1 times,
//   P_{j+1}(x, y) = ((a + b) + (c + d)) * 0.125f,
// a, b, c, d the 2 x 2 block of P_j (row-major), every operation separately
// rounded (-ffp-contract=off). Only the last step can meet an odd size; its
// source indices are clamped to W_C - 1 / H_C - 1. Every input component that
// is not finite or has |c| >= 1e9 counts as 0 (the searches' out-of-range test
// lets NaN through to the tap addressing; DESIGN.md "Temporal warm start").
// tests/initref.py restates all of it in NumPy, bit for bit.
//
// One launch, every input vector read once, no intermediate level in memory:
//   levels 1-2  in registers: a lane owns a 4 x 4 pixel block (16-byte loads
//               when the pointer, W and pad_left allow);
//   levels 3-5  across the wave: lanes in Morton order, so a level is two
//               xor-shuffles (a + b is the same sum in both lanes);
//   levels 6..K a wave walks its 32 x 32 regions in Morton order with a carry
//               stack in LDS (one slot row per level); the workgroup's 4 or 16
//               waves each own one sub-square of the 2^K tile and thread 0
//               joins them -- the last join with the clamped indices.
// K <= 5: no LDS; a workgroup is four independent regions and the lanes that
// hold a finished cell store it.
//
// H16 (DIS_FLOW_F16): the flow holds __half2 vectors, widened exactly on load
// (an interior block's row is two 8-byte loads); everything after the load is
// the same arithmetic on the same f32 values.
//
// k_init_copy is the DIS_INIT_COARSE form: the caller's planes copied into the
// context's with the same sanitising.
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "dis_half.h"
#include "dis_kernels.h"

namespace dis {
namespace {

struct InitArgs {
    const void* flow;    // n W x H fields of float2 (H16: __half2), pair stride W * H
    float2* plane;       // n iw x ih planes, pair stride iw * ih
    int W, H, Wp, Hp, pl, pt;
    int K;               // halvings (C + 1), 1..kMaxLevels - 1
    int WC, HC, iw, ih;  // level-C size, plane size
    int vec;             // flow 16-byte aligned (H16: 8-byte), W and pad_left even: two-vector loads of interior blocks
    int rgx, rgy;        // K <= 5: 32 x 32 regions covering iw * 2^K x ih * 2^K
};

constexpr int kInitMaxCarry = kMaxLevels;  // carry-stack rows (K - 5 - j <= kMaxLevels - 8)

__device__ __forceinline__ float sane(float c) { return fabsf(c) < 1e9f ? c : 0.0f; }  // NaN, inf: 0

__device__ __forceinline__ float2 box4(float2 a, float2 b, float2 c, float2 d)
{
    return make_float2(((a.x + b.x) + (c.x + d.x)) * 0.125f, ((a.y + b.y) + (c.y + d.y)) * 0.125f);
}

// the 2 x 2 mean with the right column (xok false) / bottom row (yok false)
// clamped onto the left / top one: the last halving at an odd size
__device__ __forceinline__ float2 box4_clamped(float2 a, float2 b, float2 c, float2 d, bool xok, bool yok)
{
    const float2 be = xok ? b : a, ce = yok ? c : a;
    const float2 de = xok ? (yok ? d : b) : (yok ? c : a);
    return box4(a, be, ce, de);
}

// P_0 at padded-frame pixel (x, y); zero outside the padded frame (only the
// clamped-away half of an odd last step lies there)
template <bool H16>
using FlowVec = std::conditional_t<H16, __half2, float2>;

__device__ __forceinline__ float2 load_vec(const float2* p) { return *p; }
__device__ __forceinline__ float2 load_vec(const __half2* p) { return widen2(*p); }

template <bool H16>
__device__ __forceinline__ float2 load_px(const InitArgs& a, const FlowVec<H16>* __restrict__ F, int x, int y)
{
    if (x >= a.Wp || y >= a.Hp) return make_float2(0.0f, 0.0f);
    const int sx = min(max(x - a.pl, 0), a.W - 1), sy = min(max(y - a.pt, 0), a.H - 1);
    const float2 v = load_vec(F + (long long)sy * a.W + sx);
    return make_float2(sane(v.x), sane(v.y));
}

__device__ __forceinline__ float2 shfl_xor2(float2 v, int m)
{
    return make_float2(__shfl_xor(v.x, m), __shfl_xor(v.y, m));
}

// One wave reduces the 32 x 32 padded-frame pixels at (RX, RY) by min(K, 5)
// levels. Lane l owns the 4 x 4 block at Morton position l. K <= 5: the lanes
// holding a finished cell store it and the return value is unused; K > 5: the
// region's level-5 value, valid in lane 0. Every lane of the wave must call it
// (shuffles).
template <bool H16>
__device__ __forceinline__ float2 reduce_region(const InitArgs& a, const FlowVec<H16>* __restrict__ F,
                                                float2* __restrict__ out, int RX, int RY, int lane)
{
    const int lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4);
    const int ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
    const int X0 = RX + 4 * lx, Y0 = RY + 4 * ly;
    const int K = a.K;
    float2 p[4][4];
    const int fx = X0 - a.pl, fy = Y0 - a.pt;
    if (a.vec && fx >= 0 && fy >= 0 && fx + 4 <= a.W && fy + 4 <= a.H) {
        // interior block: rows of two 16-byte loads (fx even, W even: aligned)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (H16) {  // two 8-byte loads
                const half2x2* const r = reinterpret_cast<const half2x2*>(F + (long long)(fy + j) * a.W + fx);
                const half2x2 lo = r[0], hi = r[1];
                const float2 v0 = widen2(lo.a), v1 = widen2(lo.b), v2 = widen2(hi.a), v3 = widen2(hi.b);
                p[j][0] = make_float2(sane(v0.x), sane(v0.y));
                p[j][1] = make_float2(sane(v1.x), sane(v1.y));
                p[j][2] = make_float2(sane(v2.x), sane(v2.y));
                p[j][3] = make_float2(sane(v3.x), sane(v3.y));
            } else {
                const float4* const r = reinterpret_cast<const float4*>(F + (long long)(fy + j) * a.W + fx);
                const float4 lo = r[0], hi = r[1];
                p[j][0] = make_float2(sane(lo.x), sane(lo.y));
                p[j][1] = make_float2(sane(lo.z), sane(lo.w));
                p[j][2] = make_float2(sane(hi.x), sane(hi.y));
                p[j][3] = make_float2(sane(hi.z), sane(hi.w));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) p[j][i] = load_px<H16>(a, F, X0 + i, Y0 + j);
    }
    // level 1 (the last one at K == 1: clamped per cell)
    float2 q[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ox = (X0 >> 1) + i, oy = (Y0 >> 1) + j;
            const bool xok = K != 1 || 2 * ox + 1 < a.WC, yok = K != 1 || 2 * oy + 1 < a.HC;
            q[j][i] = box4_clamped(p[2 * j][2 * i], p[2 * j][2 * i + 1], p[2 * j + 1][2 * i], p[2 * j + 1][2 * i + 1],
                                   xok, yok);
            if (K == 1 && ox < a.iw && oy < a.ih) out[(long long)oy * a.iw + ox] = q[j][i];
        }
    if (K == 1) return q[0][0];
    // the cell of the last level this block belongs to, and its clamps
    const int ox = X0 >> K, oy = Y0 >> K;
    const bool lxok = 2 * ox + 1 < a.WC, lyok = 2 * oy + 1 < a.HC;
    float2 v = box4_clamped(q[0][0], q[0][1], q[1][0], q[1][1], K != 2 || lxok, K != 2 || lyok);
    const int top = min(K, 5);
#pragma unroll
    for (int L = 3; L <= 5; ++L) {
        if (L > top) break;  // (wave-uniform)
        const bool last = L == K;
        const int mx = 1 << (2 * (L - 3)), my = mx << 1;
        // a + b in both lanes of a row pair, then (a + b) + (c + d) in all four;
        // clamped: b := a, (c + d) := (a + b) -- right where lane a reads them
        const float2 px = shfl_xor2(v, mx);
        const float2 s = (last && !lxok) ? make_float2(v.x + v.x, v.y + v.y) : make_float2(v.x + px.x, v.y + px.y);
        const float2 py = shfl_xor2(s, my);
        const float2 t = (last && !lyok) ? make_float2(s.x + s.x, s.y + s.y) : make_float2(s.x + py.x, s.y + py.y);
        v = make_float2(t.x * 0.125f, t.y * 0.125f);
    }
    if (K <= 5) {
        const int group = (1 << (2 * (K - 2))) - 1;  // lanes per finished cell - 1
        if ((lane & group) == 0 && ox < a.iw && oy < a.ih) out[(long long)oy * a.iw + ox] = v;
    }
    return v;
}

// K <= 5. grid: (ceil(rgx / 2), ceil(rgy / 2), n); 256 threads = 2 x 2 regions
template <bool H16>
__global__ void __launch_bounds__(256) k_flow_to_init_small(InitArgs a)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rx = blockIdx.x * 2 + (wave & 1), ry = blockIdx.y * 2 + (wave >> 1);
    if (rx >= a.rgx || ry >= a.rgy) return;  // whole wave
    const long long pair = blockIdx.z;
    reduce_region<H16>(a, static_cast<const FlowVec<H16>*>(a.flow) + pair * a.W * a.H, a.plane + pair * a.iw * a.ih,
                       rx * 32, ry * 32, lane);
}

// K >= 6. grid: (iw, ih, n), one 2^K tile per workgroup; NW = 4 (K == 6) or 16
// waves, wave w the tile's Morton sub-square w of side 2^(K - j), 4^j = NW
template <int NW, bool H16>
__global__ void __launch_bounds__(64 * NW) k_flow_to_init(InitArgs a)
{
    constexpr int J = NW == 4 ? 1 : 2;
    __shared__ float2 carry[NW][kInitMaxCarry][4];
    __shared__ float2 sub[NW];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ox = blockIdx.x, oy = blockIdx.y;
    const long long pair = blockIdx.z;
    const FlowVec<H16>* const F = static_cast<const FlowVec<H16>*>(a.flow) + pair * a.W * a.H;
    const int K = a.K, S = 1 << (K - J);
    // Morton position of the wave's sub-square in the tile
    const int sx = J == 1 ? (wave & 1) : ((wave & 1) | ((wave >> 1) & 2));
    const int sy = J == 1 ? (wave >> 1) : (((wave >> 1) & 1) | ((wave >> 2) & 2));
    const int SX = (ox << K) + sx * S, SY = (oy << K) + sy * S;
    // (Wp, Hp multiples of 2^(K-1) >= S: a sub-square lies inside the padded
    // frame or, in the clamped-away half of an odd last step, outside it)
    if (SX < a.Wp && SY < a.Hp) {
        const int nl = K - J - 5;  // levels above the regions inside the sub-square
        float2 res = make_float2(0.0f, 0.0f);
        for (int i = 0; i < (1 << (2 * nl)); ++i) {
            int rx = 0, ry = 0;
            for (int b = 0; b < nl; ++b) {
                rx |= ((i >> (2 * b)) & 1) << b;
                ry |= ((i >> (2 * b + 1)) & 1) << b;
            }
            float2 cur = reduce_region<H16>(a, F, nullptr, SX + 32 * rx, SY + 32 * ry, lane);
            if (lane == 0) {
                // binary-counter carries: four finished siblings make their parent
                int lvl = 0, idx = i;
                while (lvl < nl) {
                    carry[wave][lvl][idx & 3] = cur;
                    if ((idx & 3) != 3) break;
                    cur = box4(carry[wave][lvl][0], carry[wave][lvl][1], carry[wave][lvl][2], carry[wave][lvl][3]);
                    idx >>= 2;
                    ++lvl;
                }
                if (lvl == nl) res = cur;  // (the last region only)
            }
        }
        if (lane == 0) sub[wave] = res;
    } else if (lane == 0) {
        sub[wave] = make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float2 quad[4];
    if (J == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) quad[k] = sub[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) quad[k] = box4(sub[4 * k], sub[4 * k + 1], sub[4 * k + 2], sub[4 * k + 3]);
    }
    a.plane[pair * a.iw * a.ih + (long long)oy * a.iw + ox] =
        box4_clamped(quad[0], quad[1], quad[2], quad[3], 2 * ox + 1 < a.WC, 2 * oy + 1 < a.HC);
}

__global__ void __launch_bounds__(256) k_init_copy(const float* __restrict__ src, float* __restrict__ dst,
                                                   long long count)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[i] = sane(src[i]);
}

}  // namespace

void init_plane_size(const Geometry& g, int* iw, int* ih)
{
    *iw = (g.lv[g.C].W + 1) / 2;
    *ih = (g.lv[g.C].H + 1) / 2;
}

hipError_t launch_flow_to_init(const float* flow, float* planes, int n, const Geometry& g, hipStream_t s, Timing t,
                               int f16)
{
    InitArgs a{};
    a.flow = flow;
    a.plane = reinterpret_cast<float2*>(planes);
    a.W = g.W;
    a.H = g.H;
    a.Wp = g.Wp;
    a.Hp = g.Hp;
    a.pl = g.pad_left;
    a.pt = g.pad_top;
    a.K = g.C + 1;
    a.WC = g.lv[g.C].W;
    a.HC = g.lv[g.C].H;
    init_plane_size(g, &a.iw, &a.ih);
    a.vec = ((reinterpret_cast<uintptr_t>(flow) & (f16 ? 7 : 15)) == 0 && (g.W & 1) == 0 && (g.pad_left & 1) == 0) ? 1 : 0;
    if (a.K < 1 || a.K >= kMaxLevels || n < 1 || n > 65535) return hipErrorInvalidValue;
    if (a.K <= 5) {
        a.rgx = (int)((((long long)a.iw << a.K) + 31) / 32);
        a.rgy = (int)((((long long)a.ih << a.K) + 31) / 32);
        const dim3 grid((a.rgx + 1) / 2, (a.rgy + 1) / 2, n);
        if (grid.y > 65535) return hipErrorInvalidValue;
        if (f16)
            DIS_LAUNCH(t, k_flow_to_init_small<true>, grid, dim3(256), 0, s, a);
        else
            DIS_LAUNCH(t, k_flow_to_init_small<false>, grid, dim3(256), 0, s, a);
    } else {
        const dim3 grid(a.iw, a.ih, n);
        if (grid.y > 65535) return hipErrorInvalidValue;
        if (a.K == 6 && f16)
            DIS_LAUNCH(t, (k_flow_to_init<4, true>), grid, dim3(256), 0, s, a);
        else if (a.K == 6)
            DIS_LAUNCH(t, (k_flow_to_init<4, false>), grid, dim3(256), 0, s, a);
        else if (f16)
            DIS_LAUNCH(t, (k_flow_to_init<16, true>), grid, dim3(1024), 0, s, a);
        else
            DIS_LAUNCH(t, (k_flow_to_init<16, false>), grid, dim3(1024), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_init_copy(const float* src, float* dst, long long count, hipStream_t s, Timing t)
{
    if (count < 1 || (count + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    DIS_LAUNCH(t, k_init_copy, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, dst, count);
    return hipGetLastError();
}

}  // namespace dis
