// dis_warpmotion.hip -- backward warp of u8 images by motion models
// (dis_warp_motion_u8, include/dis_abi.h): what dis_motion_to_flow followed by
// dis_flow_warp_u8 writes, without the field. No reference counterpart.
//
// For pixel (x, y) of image i the vector is u = (p0 + p1*x) + p2*y, v = (p3 +
// p4*x) + p5*y in f32 (k_motion_flow's arithmetic; the canonical NaN when a
// parameter is not finite), and the pixel is dis_sample.h's warp_pixel at
// scale 1: the same bytes as the chain. Every float operation is separately
// rounded (-ffp-contract=off), so tests/stabref.py restates it bit for bit.
//
// A block owns a 64 x 16 tile of one image, a lane 4 consecutive pixels of a
// row; the stores are k_flow_warp's (dword / 16-byte when pointers and W allow).
// With 1 and 4 channels that is all (the direct form). With 3 channels, where a
// tap is three byte loads, a block has three routes to the same bytes (the
// measurements that chose this are in DESIGN.md 3m):
//   staged: an affine map sends the tile to a parallelogram, so the block takes
//           the bounding box of its four corner targets (floor - 1 .. floor + 2,
//           the targets clamped to the frame as the sampler clamps them), and
//           when the box fits kStageDwords of LDS it loads the box with coalesced
//           row reads and takes its taps from LDS;
//   lane:   a pixel of a staged block whose clamped tap indices do not all lie in
//           the box reads global memory, so every LDS index lies in the box for
//           every input. The f32 vector is only nearly affine: with large
//           parameters that cancel (p0 = -5e8, p2 = 5e8 on row 1) the partial sum
//           p0 + p1*x is rounded to a multiple of 32, and targets inside the
//           frame land tens of pixels beyond the corners' box;
//   direct: a block whose box does not fit, or whose corner vectors are not all
//           valid, is k_flow_warp with the vector computed in registers.
// `routes` (null in the library's calls) counts the three for the tests.
// The LDS image keeps each box row as dwords from the dword that holds the
// box's first byte (relative to the row start), pitch odd: a half-wave holds
// two tile rows whose lanes step by 3 dwords, and an odd pitch keeps the two
// rows' banks apart; the taps are byte reads, neighbours sharing dwords.
#include <cmath>
#include <cstdint>

#include "dis_args.h"
#include "dis_kernels.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kWmThreads = 256;                // 16 lanes x 16 rows
constexpr int kStageDwords = 4096;             // 16 KB: up to 8 blocks a CU
constexpr unsigned kWmNanBits = 0x7fc00000u;

struct WarpMotionArgs {
    const uint8_t* src;
    const float* params;  // six per image
    uint8_t* dst;
    uint8_t* valid;       // may be null
    long long src_stride, src_image_stride;  // bytes
    int W, H;
    int tiles_x, tiles;   // tiles of a row of tiles, of an image
    int zero_border;      // DIS_BORDER_ZERO
    int vec_row;          // src and both strides 4-byte aligned: (3 channels) dword staging loads, (4) one dword per tap
    int vec_dst;          // dst 4-byte (4 channels: 16-byte) aligned and W % 4 == 0: dword / 16-byte stores
    int vec_valid;        // valid 4-byte aligned and W % 4 == 0: one dword per lane
    unsigned* routes;     // null, or three counters: staged blocks, direct blocks, pixels of the lane route
};

// The staged box of a block: pixels bx0..bx1 x by0..by1, bo = the byte offset
// in a source row of the image's first dword, pitch in dwords.
struct Box {
    int bx0, bx1, by0, by1, bo, pitch;
};

__device__ __forceinline__ float2 model_vector(const float* p, int x, int y)
{
    const float fx = (float)x, fy = (float)y;
    return make_float2((p[0] + p[1] * fx) + p[2] * fy, (p[3] + p[4] * fx) + p[5] * fy);
}

// warp_pixel (dis_sample.h) at scale 1 with the taps taken from the staged box
// when all four lie in it: the same operations in the same order (kept apart
// from warp_pixel, whose callers' emitted code must not change).
template <int C>
__device__ __forceinline__ unsigned staged_pixel(const uint8_t* __restrict__ S, long long stride,
                                                 const uint8_t* __restrict__ L, const Box& bx, int x, int y, int W,
                                                 int H, float u, float v, int zero_border, unsigned* routes, unsigned* o)
{
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0u;
    if (!(fabsf(u) < 1e9f && fabsf(v) < 1e9f)) return 0u;  // also NaN
    const float su = 1.0f * u, sv = 1.0f * v;
    float px = (float)x + su, py = (float)y + sv;
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
    unsigned t00[C], t01[C], t10[C], t11[C];
    if (ix0 >= bx.bx0 && ix1 <= bx.bx1 && iy0 >= bx.by0 && iy1 <= bx.by1) {
        // byte C*ix + c - bo of box row iy - by0: in [0, 4*pitch) for bx0 <= ix <= bx1
        const int l0 = (iy0 - bx.by0) * bx.pitch * 4 - bx.bo, l1 = (iy1 - bx.by0) * bx.pitch * 4 - bx.bo;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            t00[c] = L[l0 + C * ix0 + c];
            t01[c] = L[l0 + C * ix1 + c];
            t10[c] = L[l1 + C * ix0 + c];
            t11[c] = L[l1 + C * ix1 + c];
        }
    } else {
        if (routes) atomicAdd(routes + 2, 1u);
        const uint8_t* const r0 = S + iy0 * stride;
        const uint8_t* const r1 = S + iy1 * stride;
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
        o[c] = (unsigned)fminf(fmaxf(rintf(s), 0.0f), 255.0f);
    }
    return inside ? 255u : 0u;
}

// The staged form's LDS image; the direct form has none.
template <bool STAGED>
__device__ __forceinline__ unsigned* stage_memory()
{
    if constexpr (STAGED) {
        __shared__ unsigned lds[kStageDwords];
        return lds;
    } else {
        return nullptr;
    }
}

// STAGED = false: the direct form alone (no LDS): 1 and 4 channels, and what
// the A/B measures the staged form against. STAGED = true: 3 channels.
template <int C, bool STAGED>
__global__ void __launch_bounds__(kWmThreads) k_warp_motion(WarpMotionArgs a)
{
    unsigned* const lds = stage_memory<STAGED>();
    const long long f = blockIdx.x / (unsigned)a.tiles;
    const int tile = (int)(blockIdx.x - f * a.tiles);
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int X0 = tx * kWarpMotionTileW, Y0 = ty * kWarpMotionTileH;
    const int x0 = X0 + (int)(threadIdx.x & 15u) * 4, y = Y0 + (int)(threadIdx.x >> 4);
    const uint8_t* const S = a.src + f * a.src_image_stride;
    float p[6];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        p[i] = a.params[f * 6 + i];
        finite = finite && fabsf(p[i]) <= 3.40282347e38f;  // false for NaN and the infinities
    }
    // the block's route: the same for all of its lanes
    bool stage = false;
    Box bx{};
    if constexpr (STAGED) {
        const int X1 = min(X0 + kWarpMotionTileW - 1, a.W - 1), Y1 = min(Y0 + kWarpMotionTileH - 1, a.H - 1);
        const int cxs[4] = {X0, X1, X0, X1}, cys[4] = {Y0, Y0, Y1, Y1};
        float lox = 0.0f, hix = 0.0f, loy = 0.0f, hiy = 0.0f;
        stage = finite;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2 q = model_vector(p, cxs[k], cys[k]);
            stage = stage && fabsf(q.x) < 1e9f && fabsf(q.y) < 1e9f;
            const float px = (float)cxs[k] + q.x, py = (float)cys[k] + q.y;
            lox = k ? fminf(lox, px) : px;
            hix = k ? fmaxf(hix, px) : px;
            loy = k ? fminf(loy, py) : py;
            hiy = k ? fmaxf(hiy, py) : py;
        }
        if (stage) {  // (the four targets are finite, |.| < 2^31)
            const float xm = (float)(a.W - 1), ym = (float)(a.H - 1);
            bx.bx0 = (int)fminf(fmaxf(floorf(lox) - 1.0f, 0.0f), xm);
            bx.bx1 = (int)fminf(fminf(fmaxf(floorf(hix), 0.0f), xm) + 2.0f, xm);  // (a clamped target's second tap is one further)
            bx.by0 = (int)fminf(fmaxf(floorf(loy) - 1.0f, 0.0f), ym);
            bx.by1 = (int)fminf(fminf(fmaxf(floorf(hiy), 0.0f), ym) + 2.0f, ym);
            // at most 64 * 2^24 bytes a row and 2^24 rows: compared as long long
            const long long be = (long long)(bx.bx1 + 1) * C;
            const long long bo = ((long long)bx.bx0 * C) & ~3ll;
            const long long pitch = ((be - bo + 3) >> 2) | 1;
            const long long rows = bx.by1 - bx.by0 + 1;
            stage = pitch * rows <= kStageDwords;
            bx.bo = (int)bo;  // (used only when the box fits: then below 2^31, W * C <= 2^26)
            bx.pitch = (int)pitch;
        }
        if (stage) {
            const int total = bx.pitch * (bx.by1 - bx.by0 + 1);
            const int row_bytes = a.W * C, be = (bx.bx1 + 1) * C;
            for (int i = (int)threadIdx.x; i < total; i += kWmThreads) {
                const int r = i / bx.pitch, off = bx.bo + 4 * (i - r * bx.pitch);
                const uint8_t* const g = S + (bx.by0 + r) * a.src_stride + off;
                unsigned w = 0u;
                if (off < be) {  // (else the pad dword of an odd pitch)
                    if (a.vec_row && off + 4 <= row_bytes) {
                        w = *reinterpret_cast<const unsigned*>(g);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (off + k < row_bytes) w |= (unsigned)g[k] << (8 * k);
                    }
                }
                lds[i] = w;
            }
            __syncthreads();
        }
    }
    if (a.routes && threadIdx.x == 0) atomicAdd(a.routes + (stage ? 0 : 1), 1u);
    if (y >= a.H || x0 >= a.W) return;
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    const long long p0 = (f * a.H + y) * a.W + x0;
    unsigned o[4 * C];  // the lane's output bytes, in store order
    unsigned vd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        vd[i] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) o[C * i + c] = 0u;
        if (i < m) {
            const float nanv = __uint_as_float(kWmNanBits);
            const float2 q = finite ? model_vector(p, x0 + i, y) : make_float2(nanv, nanv);
            if (STAGED && stage)
                vd[i] = staged_pixel<C>(S, a.src_stride, reinterpret_cast<const uint8_t*>(lds), bx, x0 + i, y, a.W, a.H,
                                        q.x, q.y, a.zero_border, a.routes, &o[C * i]);
            else
                vd[i] = warp_pixel<C>(S, a.src_stride, x0 + i, y, a.W, a.H, q.x, q.y, 1.0f, a.zero_border, a.vec_row,
                                      &o[C * i]);
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
void launch_wm_c(const WarpMotionArgs& a, bool direct, unsigned grid, hipStream_t s, Timing t)
{
    if constexpr (C == 3) {
        if (!direct) {
            DIS_LAUNCH(t, (k_warp_motion<C, true>), dim3(grid), dim3(kWmThreads), 0, s, a);
            return;
        }
    }
    DIS_LAUNCH(t, (k_warp_motion<C, false>), dim3(grid), dim3(kWmThreads), 0, s, a);
}

}  // namespace

hipError_t launch_warp_motion(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                              const float* params, int n, int W, int H, int zero_border, uint8_t* dst, uint8_t* valid,
                              hipStream_t s, Timing t, int direct_only, unsigned* routes)
{
    const long long blocks = warp_motion_blocks(n, W, H);
    if (blocks < 1 || (channels != 1 && channels != 3 && channels != 4)) return hipErrorInvalidValue;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src);
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), va = reinterpret_cast<uintptr_t>(valid);
    WarpMotionArgs a{};
    a.src = src;
    a.params = params;
    a.dst = dst;
    a.valid = valid;
    a.src_stride = (long long)src_stride;
    a.src_image_stride = (long long)src_image_stride;
    a.W = W;
    a.H = H;
    a.tiles_x = (W + kWarpMotionTileW - 1) / kWarpMotionTileW;
    a.tiles = a.tiles_x * ((H + kWarpMotionTileH - 1) / kWarpMotionTileH);
    a.zero_border = zero_border;
    a.routes = routes;
    a.vec_row = (((sa | src_stride | src_image_stride) & 3) == 0) ? 1 : 0;
    a.vec_dst = ((da & (channels == 4 ? 15 : 3)) == 0 && (W & 3) == 0) ? 1 : 0;
    a.vec_valid = (valid && (va & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)blocks;
    if (channels == 1)
        launch_wm_c<1>(a, direct_only != 0, grid, s, t);
    else if (channels == 3)
        launch_wm_c<3>(a, direct_only != 0, grid, s, t);
    else
        launch_wm_c<4>(a, direct_only != 0, grid, s, t);
    return hipGetLastError();
}

}  // namespace dis
