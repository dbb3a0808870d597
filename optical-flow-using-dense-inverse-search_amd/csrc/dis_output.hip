// dis_output.hip -- the fused back end of the DIS path (the front end, the
// pyramid, is dis_pyramid.hip).
//
// K4+K5 (k_output): densify the finest searched level (src/patch_grid.cpp:
// 121-182) straight from the patch displacements into an LDS tile, then
// flow *= 2^F, cv::resize(INTER_LINEAR) and crop (src/main.cpp:191-198), so
// the finest dense field never round-trips through HBM.
//
// Arithmetic is exactly that of the stand-alone kernels in dis_kernels.hip
// (and of the oracle): same expressions, same order, -ffp-contract=off.
#include "dis_device.h"
#include "dis_half.h"
#include "dis_kernels.h"

#include <type_traits>

namespace dis {

namespace {

// full-resolution output tile per workgroup (measured: 64 rows beat 16 by
// 2.3 % of the step at F >= 1); at F == 0 32 rows: the level-0 window halves
// the LDS (paper mode 70 -> 39 KB, 2 -> 4 workgroups per CU, -6 % per SLOW
// step; reference mode 44 -> 24 KB, -1 %). Paper mode at F >= 1 with 32 rows
// measured 2 % slower (7 -> 8 workgroups per CU do not pay for the halo).
constexpr int kOutTW = 64, kOutTH = 64;
template <bool UPS>
constexpr int kOutTHf = UPS ? kOutTH : 32;  // rows of an output tile

// LDS shapes per instantiation: level-F window (F == 0 is the widest; F >= 1
// needs half the tile + the interpolation halo) and the staged patch block for
// K = ceil(ps/steps) covering patches per axis (steps >= ceil(8/K), ps = 8).
template <bool UPS, int TH>
struct OutShape {
    static constexpr int SW = UPS ? kOutTW / 2 + 3 : kOutTW + 3;
    static constexpr int SH = UPS ? TH / 2 + 3 : TH + 3;
};
template <bool UPS, int K, int TH>
struct OutPatch {
    static constexpr int st = (8 + K - 1) / K;
    static constexpr int PX = (OutShape<UPS, TH>::SW + 7) / st + 2;
    // odd stride (in float2): the densify's lanes read patches at different
    // column offsets xr.x, which an even stride maps onto the same LDS banks
    static constexpr int PY = ((OutShape<UPS, TH>::SH + 7) / st + 2) | 1;
};

// cv::resize INTER_LINEAR source index / fraction for destination index d at
// scale 2^F: s = (d + .5) * 2^-F - .5 (exact dyadic in float), clamped.
__device__ __forceinline__ void lin_coef(int d, int n_src, int F, int* i, float* f)
{
    float fx = (float)(2 * d + 1 - (1 << F)) * (1.0f / (float)(2 << F));
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) {
        fx = 0;
        sx = 0;
    }
    if (sx >= n_src - 1) {
        fx = 0;
        sx = n_src - 1;
    }
    *i = sx;
    *f = fx;
}


// paper mode: I1 of level F over every tap the window's weighted votes can
// reach (floats; F == 0 has the twice wider window), staged when it fits, at a
// fixed row stride (a vote's lower taps at constant LDS offsets). F >= 1:
// 48 x 50 keeps the workgroup at 23 KB of LDS, 7 per CU (56 x 56: 26 KB, 6 per
// CU, measured 6 % slower); a window whose flows spread wider than ~11 level-F
// pixels reads I1 globally instead (same values); F == 0 (32-row tiles):
// 80 x 48 (the box is at least 67 x 35)
template <bool UPS>
constexpr int kPaperStage = UPS ? 48 * 50 : 80 * 48;
template <bool UPS>
constexpr int kPaperSS = UPS ? 48 : 80;

// one float4 (two output pixels) of the flow. (Streaming, non-temporal
// stores made the one-stream kernel trace faster -- the next call's pyramid
// no longer evicted -- but the two-sub-batch step 2-3 % slower: DESIGN.md 3.)
__device__ __forceinline__ void store_flow2(float2* dst, float2 o0, float2 o1)
{
    *reinterpret_cast<float4*>(dst) = make_float4(o0.x, o0.y, o1.x, o1.y);
}
// DIS_FLOW_F16: the same two pixels narrowed, one 8-byte store
__device__ __forceinline__ void store_flow2(__half2* dst, float2 o0, float2 o1)
{
    *reinterpret_cast<half2x2*>(dst) = half2x2{narrow2(o0), narrow2(o1)};
}

// Output rows of an interior tile at F == 1 (every tap unclamped, every column
// two-tap, the tile inside W x H). lin_coef then reduces to
// i = (d - 1) >> 1, f = 0.75 (d even) / 0.25 (d odd) for a destination index d,
// so with the thread's rows and columns starting at even y / x the taps are
// static given the parities YP = (pad_top - 1) & 1, XP = (pad_left - 1) & 1,
// and each source row's horizontal interpolation -- the same expression as
// the general path, hence the same value -- is formed once and shared by the
// (up to four) output rows that read it.
template <int YP, int XP, int SW, int RPT, class OT>
__device__ __forceinline__ void out_rows_f1(const OutputArgs& a, const float2* dense, int i0, int j0, int px, int py,
                                            int pair)
{
    constexpr int LP = XP ^ 1;                               // pad_left & 1 = parity of x = px + pad_left
    constexpr float xf0 = LP ? 0.25f : 0.75f, xf1 = LP ? 0.75f : 0.25f;
    constexpr int o1 = LP ? 0 : 1;                           // source column of pixel 1 - that of pixel 0
    constexpr int NR = (RPT - 1 + YP) / 2 + 2;               // source rows of the thread's RPT output rows
    const int c0 = ((px + a.pad_left - 1) >> 1) - i0;
    const int rs = ((py + a.pad_top - 1) >> 1) - j0;
    float2 h0[NR], h1[NR];
#pragma unroll
    for (int t = 0; t < NR; ++t) {
        const float2* row = dense + (rs + t) * SW + c0;
        const float2 sa = row[0], sb = row[1];
        h0[t] = make_float2(sa.x * (1.f - xf0) + sb.x * xf0, sa.y * (1.f - xf0) + sb.y * xf0);
        if constexpr (o1) {
            const float2 sc = row[2];
            h1[t] = make_float2(sb.x * (1.f - xf1) + sc.x * xf1, sb.y * (1.f - xf1) + sc.y * xf1);
        } else {
            h1[t] = make_float2(sa.x * (1.f - xf1) + sb.x * xf1, sa.y * (1.f - xf1) + sb.y * xf1);
        }
    }
    OT* dst = reinterpret_cast<OT*>(a.flow) + (size_t)pair * a.W * a.H + (size_t)py * a.W + px;
#pragma unroll
    for (int d = 0; d < RPT; ++d) {
        const int t = (d + YP) >> 1;                         // yi - (first source row)
        const float yf = ((d + YP) & 1) ? 0.75f : 0.25f;     // y + pad_top even -> 0.75
        const float b0 = 1.f - yf, b1 = yf;
        const float2 o0 = make_float2(h0[t].x * b0 + h0[t + 1].x * b1, h0[t].y * b0 + h0[t + 1].y * b1);
        const float2 oo = make_float2(h1[t].x * b0 + h1[t + 1].x * b1, h1[t].y * b0 + h1[t + 1].y * b1);
        store_flow2(dst + (size_t)d * a.W, o0, oo);
    }
}

}  // namespace

// grid (ceil(W/64), ceil(H/16), batch), block 256 (2x2 output pixels per thread).
// 1) stage the patch displacements covering this tile's level-F window in LDS
//    (one round of loads), 2) densify the window into LDS (src/patch_grid.cpp:
//    121-182), 3) F == 0: crop; F >= 1: scale by 2^F, resize, crop.
// K = ceil(ps / steps) bounds the covering patches per axis, so the gather is
// an unrolled, predicated K x K loop (no divergent loops).
// OT is the output's vector type: float2, or __half2 for DIS_FLOW_F16 (the
// flows narrowed in the stores, dis_half.h; a.flow then points at __half2).
template <bool UPSAMPLE, int K, bool kPaper = false, class OT = float2>
__global__ void __launch_bounds__(256) k_output(OutputArgs a)
{
    constexpr int kTH = kOutTHf<UPSAMPLE>;
    constexpr int kOutSW = OutShape<UPSAMPLE, kTH>::SW, kOutSH = OutShape<UPSAMPLE, kTH>::SH;
    constexpr int kOutPX = OutPatch<UPSAMPLE, K, kTH>::PX, kOutPY = OutPatch<UPSAMPLE, K, kTH>::PY;
    __shared__ float2 pu[(kOutPX + K + 2) * kOutPY];  // + the padding the unmasked taps may read
    __shared__ float rtab[K * K + 1];                  // RN(1 / (0.5 n)), n covering patches
    __shared__ float2 dense[kOutSW * kOutSH];
    __shared__ int2 cr[kOutSW], rr[kOutSH];
    __shared__ float s1[kPaper ? kPaperStage<UPSAMPLE> : 1];  // paper mode: staged I1 (see below)
    __shared__ int pbox[5];
    // paper mode: window columns / rows sorted by their covering-patch count,
    // and per column class v (count v): first pixel index, first sorted
    // column, columns, RCP(columns) bits (see the densify loop)
    __shared__ unsigned char csort[kPaper ? kOutSW : 1], rsort[kPaper ? kOutSH : 1];
    __shared__ int4 ctab[K + 1];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * kOutTW, oy = blockIdx.y * kTH;
    const int pair = blockIdx.z;
    const float2* u = a.u + (size_t)pair * a.u_stride;
    if (kPaper && tid == 0) {
        pbox[0] = pbox[1] = 0x7fffffff;
        pbox[2] = pbox[3] = -0x7fffffff;
        pbox[4] = 0;
    }

    // level-F window of this tile
    int i0, i1, j0, j1;
    if (UPSAMPLE) {
        float f;
        lin_coef(ox + a.pad_left, a.wF, a.F, &i0, &f);
        lin_coef(min(ox + kOutTW - 1, a.W - 1) + a.pad_left, a.wF, a.F, &i1, &f);
        lin_coef(oy + a.pad_top, a.hF, a.F, &j0, &f);
        lin_coef(min(oy + kTH - 1, a.H - 1) + a.pad_top, a.hF, a.F, &j1, &f);
        i1 = min(i1 + 1, a.wF - 1);
        j1 = min(j1 + 1, a.hF - 1);
    } else {
        i0 = ox + a.pad_left;
        j0 = oy + a.pad_top;
        i1 = min(ox + kOutTW - 1, a.W - 1) + a.pad_left;
        j1 = min(oy + kTH - 1, a.H - 1) + a.pad_top;
    }
    const int rw = i1 - i0 + 1, rh = j1 - j0 + 1;
    // patches whose footprint meets the window
    const int st = a.steps, hp = a.hp;
    const float rst = __builtin_amdgcn_rcpf((float)st);
    const int ga = max(0, floordiv_r(i0 - a.offw - hp + st, rst)), gb = min(a.npw - 1, floordiv_r(i1 - a.offw + hp, rst));
    const int ha = max(0, floordiv_r(j0 - a.offh - hp + st, rst)), hb = min(a.nph - 1, floordiv_r(j1 - a.offh + hp, rst));
    const int PW = gb - ga + 1, PH = hb - ha + 1;  // <= kOutPX x kOutPY (output_fits)
    float umin_x = INFINITY, umin_y = INFINITY, umax_x = -INFINITY, umax_y = -INFINITY;  // paper mode
    bool u_nan = false;  // paper mode: a staged patch with a NaN displacement (see the I1 box below)
    {
        constexpr int NL = (kOutPX * kOutPY + 255) / 256;
        float2 v[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int k = tid + 256 * j;
            const int cx = k / kOutPY, cy = k % kOutPY;
            const bool in = cx < PW && cy < PH;
            v[j] = in ? u[(ga + cx) * a.nph + ha + cy] : make_float2(0.f, 0.f);
            if (kPaper && in) {
                umin_x = fminf(umin_x, v[j].x);
                umax_x = fmaxf(umax_x, v[j].x);
                umin_y = fminf(umin_y, v[j].y);
                umax_y = fmaxf(umax_y, v[j].y);
                u_nan |= v[j].x != v[j].x || v[j].y != v[j].y;
            }
        }
        // new_u = u * 0.5 (src/patch_grid.cpp:156), formed once per patch (paper mode: u itself)
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (tid + 256 * j < kOutPX * kOutPY)
                pu[tid + 256 * j] = kPaper ? v[j] : make_float2(v[j].x * 0.5f, v[j].y * 0.5f);
    }
    if constexpr (kPaper) {
        // I0 of the window, parked in the .x of each pixel's dense slot (the
        // pixel's densify reads it there before writing the slot), the loads
        // issued together with the patch staging's
        // (lane = column, wave + 4 j = row: no index division; lanes and rows
        // past the window reload its last column / row and store nothing)
        const float* I0 = a.img0 + (size_t)pair * a.plane_stride;
        constexpr int NR = (kOutSH + 3) / 4;
        const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
        for (int cb = 0; cb < kOutSW; cb += 64) {
            const int c = cb + lane;
            const float* col = I0 + (size_t)j0 * a.wF + i0 + min(c, rw - 1);
            float v0[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) v0[j] = col[(size_t)min(wv + 4 * j, rh - 1) * a.wF];
#pragma unroll
            for (int j = 0; j < NR; ++j)
                if (wv + 4 * j < rh && c < rw) dense[(wv + 4 * j) * kOutSW + c].x = v0[j];
        }
    }
    if (!kPaper && tid >= 64 && tid - 64 <= K * K) {
        const int n = tid - 64;
        rtab[n] = n ? 1.0f / (0.5f * (float)n) : 0.0f;
    }
    // covering patch ranges per window column / row (one floordiv pair each)
    if (tid < rw) {
        const int px = i0 + tid;
        cr[tid] = make_int2(max(floordiv_r(px - a.offw - hp + st, rst), ga) - ga,
                            min(floordiv_r(px - a.offw + hp, rst), gb) - ga);
    }
    if (tid >= 128 && tid - 128 < rh) {
        const int py = j0 + tid - 128;
        rr[tid - 128] = make_int2(max(floordiv_r(py - a.offh - hp + st, rst), ha) - ha,
                                  min(floordiv_r(py - a.offh + hp, rst), hb) - ha);
    }
    __syncthreads();
    // paper mode: sort the window's columns (wave 0) and rows (wave 1) by
    // covering-patch count, a stable counting sort by ballots. The densify
    // below walks the window class by class, so the lanes of a wave share
    // their counts and the K x K vote loop skips the empty slots wave-wide
    // (unsorted, a wave's lanes mix the counts 2 and 3 of steps 3 and every
    // lane issued all 9 slots for 7.1 votes on average).
    if constexpr (kPaper) {
        if (tid < 128) {
            const bool cols = tid < 64;
            const int n = cols ? rw : rh, lane = tid & 63;
            unsigned char* out = cols ? csort : rsort;
            auto cls = [&](int i) {
                if (i >= n) return -1;
                const int2 e = cols ? cr[i] : rr[i];
                return max(e.y - e.x + 1, 0);
            };
            int cnt[K + 1];
#pragma unroll
            for (int v = 0; v <= K; ++v) cnt[v] = 0;
            for (int b = 0; b < n; b += 64) {
                const int v = cls(b + lane);
#pragma unroll
                for (int w = 0; w <= K; ++w) cnt[w] += __popcll(__ballot(v == w));
            }
            int base[K + 1];
            base[0] = 0;
#pragma unroll
            for (int v = 1; v <= K; ++v) base[v] = base[v - 1] + cnt[v - 1];
            if (cols && lane <= K) {
                int b0 = 0, c0 = 0;
#pragma unroll
                for (int v = 0; v <= K; ++v)
                    if (v == lane) {
                        b0 = base[v];
                        c0 = cnt[v];
                    }
                ctab[lane] = make_int4(b0 * rh, b0, c0, __float_as_int(__builtin_amdgcn_rcpf((float)max(c0, 1))));
            }
            for (int b = 0; b < n; b += 64) {
                const int v = cls(b + lane);
#pragma unroll
                for (int w = 0; w <= K; ++w) {
                    const unsigned long long m = __ballot(v == w);
                    if (v == w)
                        out[base[w] + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                            (unsigned char)(b + lane);
                    base[w] += __popcll(m);
                }
            }
        }
    }
    // paper mode: every vote samples I1 (bilinear, replicate border) at
    // X = clamp(RN(x + u.x), -1, W) for a window pixel x and a staged patch's
    // u, so its taps floor(X), floor(X) + 1 lie in [max(i0 + floor(min u.x),
    // -1), min(i1 + floor(max u.x) + 1, W) + 1] (likewise in y). Staged in LDS
    // by logical position, each entry the replicate-clamped pixel the global
    // read would return, when that box fits; else the votes read I1 globally.
    int bx0 = 0, by0 = 0, sws = 0;
    bool staged = false;
    if constexpr (kPaper) {
        auto fl = [](float v) { return (int)fminf(fmaxf(floorf(v), -1048576.0f), 1048576.0f); };
        int m0 = umin_x <= umax_x ? fl(umin_x) : 0x7fffffff, m1 = umin_y <= umax_y ? fl(umin_y) : 0x7fffffff;
        int m2 = umin_x <= umax_x ? fl(umax_x) : -0x7fffffff, m3 = umin_y <= umax_y ? fl(umax_y) : -0x7fffffff;
        // The staged taps' LDS index comes from v_med3 clamps, which do not
        // clamp NaN, and fminf / fmaxf above skip NaN. The search never leaves
        // a NaN displacement (it resets them like outliers), but should one
        // reach this kernel, the whole tile takes the global (replicate-
        // clamped) reads instead of the stage (pbox[4]).
        const bool wave_nan = __ballot(u_nan) != 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m0 = min(m0, __shfl_xor(m0, o));
            m1 = min(m1, __shfl_xor(m1, o));
            m2 = max(m2, __shfl_xor(m2, o));
            m3 = max(m3, __shfl_xor(m3, o));
        }
        if ((tid & 63) == 0) {
            if (wave_nan) pbox[4] = 1;
            atomicMin(&pbox[0], m0);
            atomicMin(&pbox[1], m1);
            atomicMax(&pbox[2], m2);
            atomicMax(&pbox[3], m3);
        }
        __syncthreads();
        if (pbox[0] != 0x7fffffff) {
            bx0 = max(i0 + pbox[0], -1);
            by0 = max(j0 + pbox[1], -1);
            const int bx1 = min(i1 + pbox[2] + 1, a.wF) + 1, by1 = min(j1 + pbox[3] + 1, a.hF) + 1;
            sws = bx1 - bx0 + 1;
            const int shs = by1 - by0 + 1;
            staged = !pbox[4] && sws > 0 && shs > 0 && sws <= kPaperSS<UPSAMPLE> && shs * kPaperSS<UPSAMPLE> <= kPaperStage<UPSAMPLE>;
            if (staged) {  // every load issued before the first store: one memory latency
                // lane = column, wave + 4 j = row (as the I0 window above)
                constexpr int SS = kPaperSS<UPSAMPLE>, NR = (kPaperStage<UPSAMPLE> / SS + 3) / 4;
                const float* I1 = a.img1 + (size_t)pair * a.plane_stride;
                const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
                for (int cb = 0; cb < SS; cb += 64) {
                    const int c = cb + lane;
                    const float* col = I1 + clampi(bx0 + min(c, sws - 1), 0, a.wF - 1);
                    float v1[NR];
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        v1[j] = col[(size_t)clampi(by0 + min(wv + 4 * j, shs - 1), 0, a.hF - 1) * a.wF];
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        if (wv + 4 * j < shs && c < sws) s1[(wv + 4 * j) * SS + c] = v1[j];
                }
            }
        }
        __syncthreads();
    }
    const float sc = a.sc;
    const float rrw = __builtin_amdgcn_rcpf((float)rw);  // k / rw by floordiv_r (exact, |k| < 2^20)
    int pxc[K + 1];  // paper mode: first pixel index of each column class
#pragma unroll
    for (int v = 0; v <= K; ++v) pxc[v] = kPaper ? ctab[v].x : 0;
    // paper mode, staged: a tap's LDS index fma(floor Y, stride, floor X)
    // (integers below 2^24: exact) from s1b = s1 - (by0 * stride + bx0)
    constexpr int kSS = kPaperSS<UPSAMPLE>;
    const float* s1b = s1 - (by0 * kSS + bx0);
    // the staged / global choice (block-uniform) outside the pixel loop
    auto densify = [&](auto staged_c) {
        constexpr bool kStaged = decltype(staged_c)::value;
        for (int k = tid; k < rw * rh; k += 256) {
            int r, c;
            if constexpr (kPaper) {
                // pixel k of the class-major order: class z (the last whose first
                // index <= k), then sorted row / sorted column within the class
                int z = 0;
#pragma unroll
                for (int v = 1; v <= K; ++v) z += k >= pxc[v] ? 1 : 0;
                const int4 e = ctab[z];
                const int l = k - e.x;
                const int rs = floordiv_r(l, __int_as_float(e.w));
                c = csort[e.y + l - rs * e.z];
                r = rsort[rs];
            } else {
                r = floordiv_r(k, rrw);
                c = k - r * rw;
            }
            // dense value: contributions in patch-id order, f from +0; masked
            // terms add +0, an exact no-op (f is never -0)
            const int2 xr = cr[c], yr = rr[r];
            float fx = 0.0f, fy = 0.0f, w = 0.0f;
            if constexpr (kPaper) {
                // SURVEY 8f row 4 (oracle densify_paper): weight 1/max(1, |I1(x+u) - I0(x)|)
                const int xg = i0 + c, yg = j0 + r;  // level-F pixel
                const float* I1 = a.img1 + (size_t)pair * a.plane_stride;
                const float i0v = dense[r * kOutSW + c].x;  // I0(x), staged above
                const float xf = (float)xg, yf = (float)yg;
#pragma unroll
                for (int i = 0; i < K; ++i)
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((xr.x + i <= xr.y) && (yr.x + j <= yr.y)) {
                            const float2 t = pu[(xr.x + i) * kOutPY + yr.x + j];
                            float d;
                            if constexpr (kStaged) {  // bilinear_replicate's expressions on the staged taps
                                const float X = clamp_m1(xf + t.x, (float)a.wF);
                                const float Y = clamp_m1(yf + t.y, (float)a.hF);
                                const float fx0 = floorf(X), fy0 = floorf(Y);
                                const float ax = X - fx0, ay = Y - fy0;
                                const float* q = s1b + (int)__builtin_fmaf(fy0, (float)kSS, fx0);
                                const float top = (1.0f - ax) * q[0] + ax * q[1];
                                const float bot = (1.0f - ax) * q[kSS] + ax * q[kSS + 1];
                                d = ((1.0f - ay) * top + ay * bot) - i0v;
                            } else {
                                d = bilinear_replicate(I1, a.wF, a.hF, xf + t.x, yf + t.y) - i0v;
                            }
                            const float cw = recip_max1(d);  // correctly rounded (dis_device.h)
                            fx = fx + cw * t.x;
                            fy = fy + cw * t.y;
                            w = w + cw;
                        }
                    }
            } else {
                // covering patches per axis (<= K), read at constant offsets from the
                // first one (the LDS array is padded for the taps past the range)
                const int nx = max(xr.y - xr.x + 1, 0), ny = max(yr.y - yr.x + 1, 0);
                const float2* pb = pu + xr.x * kOutPY + yr.x;
#pragma unroll
                for (int i = 0; i < K; ++i)
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const bool ok = i < nx && j < ny;
                        const float2 t = pb[i * kOutPY + j];
                        fx = fx + (ok ? t.x : 0.0f);
                        fy = fy + (ok ? t.y : 0.0f);
                    }
                // the reference's weight sum of 0.5 per covering patch, exactly
                const int n = nx * ny;
                w = 0.5f * (float)n;
                // fx / w correctly rounded from the tabulated RN(1 / w) (div_pre);
                // tiny nonzero numerators, whose remainders could underflow, take
                // the IEEE division below
                const bool tiny = (fx != 0.0f && fabsf(fx) < 0x1p-100f) || (fy != 0.0f && fabsf(fy) < 0x1p-100f);
                if (n > 0 && !tiny) {
                    const float rcp = rtab[n];
                    fx = div_pre(fx, w, rcp);
                    fy = div_pre(fy, w, rcp);
                    w = 0.0f;  // done
                }
            }
            if (w > 0) {
                fx = fx / w;
                fy = fy / w;
            }
            // flowout *= sc_fct (src/main.cpp:194) before the resize
            dense[r * kOutSW + c] = UPSAMPLE ? make_float2(fx * sc, fy * sc) : make_float2(fx, fy);
        }
    };
    if (kPaper && staged)
        densify(std::true_type{});
    else
        densify(std::false_type{});
    __syncthreads();

    constexpr int RPT = kTH / 8;  // output rows per thread
    const int px = ox + (tid & 31) * 2, py = oy + (tid >> 5) * RPT;
    if constexpr (UPSAMPLE) {
        const int xh = ox + kOutTW - 1 + a.pad_left, yh = oy + kTH - 1 + a.pad_top;
        if (a.F == 1 && a.vec_store && ox + kOutTW <= a.W && oy + kTH <= a.H && ox + a.pad_left >= 1 &&
            oy + a.pad_top >= 1 && ((xh - 1) >> 1) + 1 <= a.wF - 1 && ((yh - 1) >> 1) + 1 <= a.hF - 1 &&
            xh < a.xmax) {  // uniform: an interior tile
            switch (((a.pad_top - 1) & 1) * 2 + ((a.pad_left - 1) & 1)) {
                case 0: out_rows_f1<0, 0, kOutSW, RPT, OT>(a, dense, i0, j0, px, py, pair); break;
                case 1: out_rows_f1<0, 1, kOutSW, RPT, OT>(a, dense, i0, j0, px, py, pair); break;
                case 2: out_rows_f1<1, 0, kOutSW, RPT, OT>(a, dense, i0, j0, px, py, pair); break;
                default: out_rows_f1<1, 1, kOutSW, RPT, OT>(a, dense, i0, j0, px, py, pair); break;
            }
            return;
        }
    }
#pragma unroll
    for (int dy = 0; dy < RPT; ++dy) {
        const int y = py + dy;
        if (y >= a.H) continue;
        float2 o[2];
        if (UPSAMPLE) {
            int yi;
            float yf;
            lin_coef(y + a.pad_top, a.hF, a.F, &yi, &yf);
            const int r0 = yi - j0, r1 = min(yi + 1, a.hF - 1) - j0;
            const float b0 = 1.f - yf, b1 = yf;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int xx = px + dx + a.pad_left;
                int xi;
                float xf;
                lin_coef(xx, a.wF, a.F, &xi, &xf);
                const bool two = xx < a.xmax;
                const int c0 = xi - i0;
                float h[2][2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float2* row = dense + (k ? r1 : r0) * kOutSW;
                    const float2 s0 = row[c0];
                    if (two) {
                        const float2 s1 = row[c0 + 1];
                        h[k][0] = s0.x * (1.f - xf) + s1.x * xf;
                        h[k][1] = s0.y * (1.f - xf) + s1.y * xf;
                    } else {
                        h[k][0] = s0.x;
                        h[k][1] = s0.y;
                    }
                }
                o[dx] = make_float2(h[0][0] * b0 + h[1][0] * b1, h[0][1] * b0 + h[1][1] * b1);
            }
        } else {
            const float2* row = dense + (y - oy) * kOutSW + (px - ox);
            o[0] = row[0];
            o[1] = row[1];
        }
        OT* dst = reinterpret_cast<OT*>(a.flow) + (size_t)pair * a.W * a.H + (size_t)y * a.W + px;
        if (px + 1 < a.W) {
            if (a.vec_store) {
                store_flow2(dst, o[0], o[1]);
            } else {
                store_flow1(dst, o[0]);
                store_flow1(dst + 1, o[1]);
            }
        } else if (px < a.W) {
            store_flow1(dst, o[0]);
        }
    }
}

bool output_fits(const OutputArgs& a)
{
    // patch size 8 (the fast path), at most 4 covering patches per axis
    // (steps >= 2); the LDS shapes above are derived from exactly that
    return a.hp == 4 && a.steps >= 2;
}

template <int K, class OT>
static void launch_output_k(const OutputArgs& a, dim3 grid, hipStream_t s, Timing t)
{
    if (a.paper) {
        if (a.F == 0)
            DIS_LAUNCH(t, (k_output<false, K, true, OT>), grid, dim3(256), 0, s, a);
        else
            DIS_LAUNCH(t, (k_output<true, K, true, OT>), grid, dim3(256), 0, s, a);
    } else if (a.F == 0) {
        DIS_LAUNCH(t, (k_output<false, K, false, OT>), grid, dim3(256), 0, s, a);
    } else {
        DIS_LAUNCH(t, (k_output<true, K, false, OT>), grid, dim3(256), 0, s, a);
    }
}

hipError_t launch_output(const OutputArgs& a, int batch, hipStream_t s, Timing t, int f16)
{
    if (!output_fits(a)) return hipErrorInvalidValue;
    const int th = a.F == 0 ? kOutTHf<false> : kOutTHf<true>;
    dim3 grid((a.W + kOutTW - 1) / kOutTW, (a.H + th - 1) / th, batch);
    switch ((2 * a.hp + a.steps - 1) / a.steps) {  // K = ceil(ps / steps)
#define DIS_CASE(KK)                                        \
    case KK:                                                \
        if (f16)                                            \
            launch_output_k<KK, __half2>(a, grid, s, t);    \
        else                                                \
            launch_output_k<KK, float2>(a, grid, s, t);     \
        break;
        DIS_CASE(1)
        DIS_CASE(2)
        DIS_CASE(3)
        DIS_CASE(4)
#undef DIS_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dis
