// dis_yuv.hip -- 8-bit 4:2:0 video surfaces (NV12, NV21, I420, YV12) to
// interleaved 8-bit frames and back: dis_yuv420_to_frames_u8 and
// dis_frames_to_yuv420_u8 (include/dis_abi.h), their kernels and their entry
// points. The arithmetic is integers only, in signed 32 bits with floor shifts
// (tests/yuvref.py restates it and derives the table below from the standards'
// rationals): with u = Cb - 128, v = Cr - 128 and c = yy * (Y - yoff) + 8192,
//   R = clamp((c + rv*v) >> 14), G = clamp((c + gu*u + gv*v) >> 14), B = clamp((c + bu*u) >> 14)
// for the pixels of a 2 x 2 block (nearest chroma), and back
//   Y = yoff + ((ky . (R,G,B) + 8192) >> 14)                       per pixel,
//   Cb = clamp((kcb . (sR,sG,sB) + (128 << 16) + (1 << 15)) >> 16)  per block
// over the block's sums, Cr likewise: the average and the conversion round
// once. Every operand fits 24 signed bits and every sum stays below 2^25, so
// the 24-bit multiplies are exact.
//
// dis_luma.hip's shape: one streaming launch each, no LDS, no barriers. A lane
// owns a strip of 16 pixels x 2 rows: two 16-byte Y groups, eight chroma pairs,
// two packed groups of 16 * C bytes. A full strip moves each of the three sides
// in its vector form when that side's bases and strides allow it (Y and packed
// frames: multiples of 16, 16-byte loads / stores; interleaved chroma, Cb and Cr
// one byte apart with c_step 2: multiples of 16, one 16-byte group at the lower
// pointer; planar chroma, c_step 1: multiples of 8, one 8-byte group a plane),
// every load issued before the first is consumed, and byte by byte otherwise;
// a row's last, partial strip always goes byte by byte. The packed stores of
// k_yuv420_to_frames are transposed inside each quad of lanes first (quad_group),
// so that four lanes store 64 contiguous bytes an instruction: a lane storing its
// own groups writes 16 bytes in every 48 or 64, which measured 0.76 - 0.83 of a
// copy's rate where the transposed stores reach 0.90 - 0.97. All
// forms move the same bytes, and none touches a byte after a row's last sample
// in any plane.
#include <cstdint>

#include "dis_args.h"
#include "dis_kernels.h"
#include "dis_stage.h"

namespace dis {
namespace {

constexpr int kStrip = kYuvStripW;

// the rows of the table, index matrix * 2 + range (DIS_YUV_LIMITED 0, DIS_YUV_FULL 1)
struct ToRgb {
    int yoff, yy, rv, gu, gv, bu;
};
struct ToYuv {
    int yoff, ky[3], kcb[3], kcr[3];  // each over (R, G, B)
};
constexpr ToRgb kToRgb[4] = {{16, 19077, 26149, -6419, -13320, 33050},   // BT.601 limited
                             {0, 16384, 22970, -5638, -11700, 29032},    // BT.601 full
                             {16, 19077, 29372, -3494, -8731, 34610},    // BT.709 limited
                             {0, 16384, 25802, -3069, -7670, 30402}};    // BT.709 full
constexpr ToYuv kToYuv[4] = {{16, {4207, 8260, 1604}, {-2428, -4768, 7196}, {7196, -6026, -1170}},
                             {0, {4899, 9617, 1868}, {-2765, -5427, 8192}, {8192, -6860, -1332}},
                             {16, {2991, 10064, 1016}, {-1649, -5547, 7196}, {7196, -6536, -660}},
                             {0, {3483, 11718, 1183}, {-1877, -6315, 8192}, {8192, -7441, -751}}};

enum { kChromaBytes = 0, kChromaInterleaved = 1, kChromaPlanar = 2 };

struct YuvArgs {
    uint8_t* y;   // the surface: read by k_yuv420_to_frames, written by k_frames_to_yuv420
    uint8_t* cb;
    uint8_t* cr;
    uint8_t* p;   // the packed frames: the other way round
    long long items;  // n * (H / 2) * cw lanes of work
    long long y_stride, y_image_stride, c_stride, c_image_stride, p_stride, p_image_stride;  // bytes
    int W, H2, cw;    // H2 = H / 2 strip rows, cw = ceil(W / 16) strips a row
    int c_step;
    int vec_y, vec_p;  // the side's bases and strides are multiples of 16
    int vec_c;         // kChroma*: how a full strip moves its eight chroma pairs
    int cr_first;      // kChromaInterleaved: Cr is the lower byte of a pair (NV21)
    int alpha;
    ToRgb to_rgb;
    ToYuv to_yuv;
};

__device__ __forceinline__ unsigned byte_of(const unsigned* w, int j) { return (w[j >> 2] >> ((j & 3) * 8)) & 0xffu; }
__device__ __forceinline__ void put_byte(unsigned* w, int j, unsigned v) { w[j >> 2] |= v << ((j & 3) * 8); }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// where a lane's strip lies
struct Strip {
    long long img;
    int by, x0, m;  // block row, first pixel, pixels (16, or fewer in a row's last strip; even)
};
__device__ __forceinline__ Strip strip_of(const YuvArgs& a, long long t)
{
    const long long row = t / a.cw;  // image * H2 + block row
    Strip s;
    s.x0 = (int)(t - row * a.cw) * kStrip;
    s.img = row / a.H2;
    s.by = (int)(row - s.img * a.H2);
    s.m = min(kStrip, a.W - s.x0);
    return s;
}

// the chroma terms of a block
struct ChromaTerms {
    int r, g, b;
};
__device__ __forceinline__ ChromaTerms chroma_terms(const ToRgb& k, int cb, int cr)
{
    const int u = cb - 128, v = cr - 128;
    return {__mul24(k.rv, v), __mul24(k.gu, u) + __mul24(k.gv, v), __mul24(k.bu, u)};
}

// the C samples of one pixel (C = 1: gray) into s[0..C)
template <int C, bool RFIRST>
__device__ __forceinline__ void pixel_of(const ToRgb& k, int yv, const ChromaTerms& t, int alpha, unsigned* s)
{
    const int c = __mul24(k.yy, yv - k.yoff) + 8192;
    if constexpr (C == 1) {
        s[0] = (unsigned)clamp255(c >> 14);
    } else {
        const unsigned r = (unsigned)clamp255((c + t.r) >> 14), g = (unsigned)clamp255((c + t.g) >> 14),
                       b = (unsigned)clamp255((c + t.b) >> 14);
        s[0] = RFIRST ? r : b;
        s[1] = g;
        s[2] = RFIRST ? b : r;
        if constexpr (C == 4) s[3] = (unsigned)alpha;
    }
}

// Group 4 * J + l of the 4 * C 16-byte groups that the four lanes of a quad hold (o: this lane's C groups), for
// lane l of the quad: group g of the quad is group g % C of lane g / C. Every lane of the quad must be active.
template <int C, int J>
__device__ __forceinline__ uint4 quad_group(const unsigned* o, int l)
{
    constexpr int kCtrl = ((4 * J) / C) | (((4 * J + 1) / C) << 2) | (((4 * J + 2) / C) << 4) | (((4 * J + 3) / C) << 6);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < C; ++g) {
        const bool mine = (4 * J + l) % C == g;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned v = (unsigned)__builtin_amdgcn_update_dpp(0, (int)o[4 * g + k], kCtrl, 0xf, 0xf, false);  // quad_perm
            w[k] = mine ? v : w[k];
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int C, bool RFIRST>
__global__ void __launch_bounds__(kYuvThreads) k_yuv420_to_frames(YuvArgs a)
{
    const long long t = (long long)blockIdx.x * kYuvThreads + threadIdx.x;
    if (t >= a.items) return;
    const Strip s = strip_of(a, t);
    const uint8_t* const Y0 = a.y + s.img * a.y_image_stride + 2ll * s.by * a.y_stride + s.x0;
    const uint8_t* const Yr[2] = {Y0, Y0 + a.y_stride};
    uint8_t* const P0 = a.p + s.img * a.p_image_stride + 2ll * s.by * a.p_stride + (long long)s.x0 * C;
    uint8_t* const Pr[2] = {P0, P0 + a.p_stride};
    const long long coff = s.img * a.c_image_stride + s.by * a.c_stride + (long long)(s.x0 >> 1) * a.c_step;
    const ToRgb k = a.to_rgb;
    // the four lanes of a quad hold four full strips of one row (strips a row: a multiple of 4; none of the four partial)
    const bool quad = C > 1 && (a.cw & 3) == 0 && ((s.x0 / kStrip) | 3) < a.W / kStrip;
    if (s.m == kStrip) {
        // (x0 is a multiple of 16: a side whose bases and strides are, is aligned here, and the strip ends inside the row)
        unsigned yw[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, u[2] = {0u, 0u}, v[2] = {0u, 0u};
        if (a.vec_y) {
            const uint4 q0 = *reinterpret_cast<const uint4*>(Yr[0]), q1 = *reinterpret_cast<const uint4*>(Yr[1]);
            yw[0][0] = q0.x, yw[0][1] = q0.y, yw[0][2] = q0.z, yw[0][3] = q0.w;
            yw[1][0] = q1.x, yw[1][1] = q1.y, yw[1][2] = q1.z, yw[1][3] = q1.w;
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < kStrip; ++i) put_byte(yw[r], i, Yr[r][i]);
        }
        if constexpr (C > 1) {  // (a gray target reads no chroma: cb and cr may be null)
            if (a.vec_c == kChromaInterleaved) {
                const uint4 q = *reinterpret_cast<const uint4*>((a.cr_first ? a.cr : a.cb) + coff);
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
                unsigned lo[2] = {0u, 0u}, hi[2] = {0u, 0u};  // the lower and the upper bytes of the pairs
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    put_byte(lo, i, byte_of(w, 2 * i));
                    put_byte(hi, i, byte_of(w, 2 * i + 1));
                }
                u[0] = a.cr_first ? hi[0] : lo[0], u[1] = a.cr_first ? hi[1] : lo[1];
                v[0] = a.cr_first ? lo[0] : hi[0], v[1] = a.cr_first ? lo[1] : hi[1];
            } else if (a.vec_c == kChromaPlanar) {
                const uint2 qu = *reinterpret_cast<const uint2*>(a.cb + coff),
                            qv = *reinterpret_cast<const uint2*>(a.cr + coff);
                u[0] = qu.x, u[1] = qu.y, v[0] = qv.x, v[1] = qv.y;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    put_byte(u, i, a.cb[coff + i * a.c_step]);
                    put_byte(v, i, a.cr[coff + i * a.c_step]);
                }
            }
        }
        ChromaTerms ct[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ct[i] = chroma_terms(k, (int)byte_of(u, i), (int)byte_of(v, i));
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            unsigned o[4 * C];  // the row's 16 * C bytes, in store order
#pragma unroll
            for (int j = 0; j < 4 * C; ++j) o[j] = 0u;
#pragma unroll
            for (int i = 0; i < kStrip; ++i) {
                unsigned px[C];
                pixel_of<C, RFIRST>(k, (int)byte_of(yw[r], i), ct[i >> 1], a.alpha, px);
#pragma unroll
                for (int j = 0; j < C; ++j) put_byte(o, C * i + j, px[j]);
            }
            if (a.vec_p && quad) {
                // The four lanes' 4 * C groups of 16 bytes are one contiguous piece of the row. Store
                // instruction j writes its groups 4j .. 4j + 3, one a lane: 64 contiguous bytes a quad, where
                // each lane storing its own groups would write 16 bytes in every 16 * C. Group g is group
                // g % C of lane g / C: for each of a lane's C groups one quad_perm move, and each lane keeps
                // the one it wants.
                const int l = (int)(threadIdx.x & 3);
                uint4* const d = reinterpret_cast<uint4*>(Pr[r] - l * (kStrip * C));
                d[l] = quad_group<C, 0>(o, l);
                if constexpr (C > 1) d[4 + l] = quad_group<C, 1>(o, l);
                if constexpr (C > 2) d[8 + l] = quad_group<C, 2>(o, l);
                if constexpr (C > 3) d[12 + l] = quad_group<C, 3>(o, l);
            } else if (a.vec_p) {
                uint4* const d = reinterpret_cast<uint4*>(Pr[r]);
#pragma unroll
                for (int j = 0; j < C; ++j) d[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < kStrip * C; ++j) Pr[r][j] = (uint8_t)byte_of(o, j);
            }
        }
        return;
    }
    // a row's last, partial strip: block by block
    for (int i = 0; i < s.m; i += 2) {
        ChromaTerms ct = {0, 0, 0};
        if constexpr (C > 1) ct = chroma_terms(k, a.cb[coff + (i >> 1) * a.c_step], a.cr[coff + (i >> 1) * a.c_step]);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                unsigned px[C];
                pixel_of<C, RFIRST>(k, Yr[r][i + dx], ct, a.alpha, px);
#pragma unroll
                for (int j = 0; j < C; ++j) Pr[r][(i + dx) * C + j] = (uint8_t)px[j];
            }
    }
}

// a pixel's (R, G, B) of its samples s0, s1, s2 (C = 1: all three are s0)
template <int C, bool RFIRST>
__device__ __forceinline__ void rgb_of(unsigned s0, unsigned s1, unsigned s2, int* rgb)
{
    if constexpr (C == 1) {
        rgb[0] = rgb[1] = rgb[2] = (int)s0;
    } else {
        rgb[0] = (int)(RFIRST ? s0 : s2);
        rgb[1] = (int)s1;
        rgb[2] = (int)(RFIRST ? s2 : s0);
    }
}
__device__ __forceinline__ unsigned luma_of(const ToYuv& k, const int* rgb)
{
    return (unsigned)(k.yoff + ((__mul24(k.ky[0], rgb[0]) + __mul24(k.ky[1], rgb[1]) + __mul24(k.ky[2], rgb[2]) + 8192) >> 14));
}
// a chroma sample of a block's sums
__device__ __forceinline__ unsigned chroma_of(const int* kc, const int* sum)
{
    return (unsigned)clamp255((__mul24(kc[0], sum[0]) + __mul24(kc[1], sum[1]) + __mul24(kc[2], sum[2]) + (128 << 16) + (1 << 15)) >> 16);
}

template <int C, bool RFIRST>
__global__ void __launch_bounds__(kYuvThreads) k_frames_to_yuv420(YuvArgs a)
{
    const long long t = (long long)blockIdx.x * kYuvThreads + threadIdx.x;
    if (t >= a.items) return;
    const Strip s = strip_of(a, t);
    uint8_t* const Y0 = a.y + s.img * a.y_image_stride + 2ll * s.by * a.y_stride + s.x0;
    uint8_t* const Yr[2] = {Y0, Y0 + a.y_stride};
    const uint8_t* const P0 = a.p + s.img * a.p_image_stride + 2ll * s.by * a.p_stride + (long long)s.x0 * C;
    const uint8_t* const Pr[2] = {P0, P0 + a.p_stride};
    const long long coff = s.img * a.c_image_stride + s.by * a.c_stride + (long long)(s.x0 >> 1) * a.c_step;
    const ToYuv k = a.to_yuv;
    constexpr int S1 = C > 1 ? 1 : 0, S2 = C > 1 ? 2 : 0;  // where a pixel's second and third samples are
    if (s.m == kStrip) {
        unsigned w[2][4 * C];
        if (a.vec_p) {
            uint4 q[2][C];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < C; ++j) q[r][j] = reinterpret_cast<const uint4*>(Pr[r])[j];  // every load first
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    w[r][4 * j] = q[r][j].x, w[r][4 * j + 1] = q[r][j].y;
                    w[r][4 * j + 2] = q[r][j].z, w[r][4 * j + 3] = q[r][j].w;
                }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int j = 0; j < 4 * C; ++j) w[r][j] = 0u;
#pragma unroll
                for (int j = 0; j < kStrip * C; ++j) put_byte(w[r], j, Pr[r][j]);
            }
        }
        unsigned yo[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, u[2] = {0u, 0u}, v[2] = {0u, 0u};
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            int sum[3] = {0, 0, 0};
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int i = 2 * b + dx;
                    int rgb[3];
                    rgb_of<C, RFIRST>(byte_of(w[r], C * i), byte_of(w[r], C * i + S1), byte_of(w[r], C * i + S2), rgb);
                    put_byte(yo[r], i, luma_of(k, rgb));
                    sum[0] += rgb[0], sum[1] += rgb[1], sum[2] += rgb[2];
                }
            put_byte(u, b, chroma_of(k.kcb, sum));
            put_byte(v, b, chroma_of(k.kcr, sum));
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (a.vec_y) {
                *reinterpret_cast<uint4*>(Yr[r]) = make_uint4(yo[r][0], yo[r][1], yo[r][2], yo[r][3]);
            } else {
#pragma unroll
                for (int i = 0; i < kStrip; ++i) Yr[r][i] = (uint8_t)byte_of(yo[r], i);
            }
        }
        if (a.vec_c == kChromaInterleaved) {
            const unsigned lo[2] = {a.cr_first ? v[0] : u[0], a.cr_first ? v[1] : u[1]};  // the pairs' lower bytes
            const unsigned hi[2] = {a.cr_first ? u[0] : v[0], a.cr_first ? u[1] : v[1]};
            unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                put_byte(o, 2 * i, byte_of(lo, i));
                put_byte(o, 2 * i + 1, byte_of(hi, i));
            }
            *reinterpret_cast<uint4*>((a.cr_first ? a.cr : a.cb) + coff) = make_uint4(o[0], o[1], o[2], o[3]);
        } else if (a.vec_c == kChromaPlanar) {
            *reinterpret_cast<uint2*>(a.cb + coff) = make_uint2(u[0], u[1]);
            *reinterpret_cast<uint2*>(a.cr + coff) = make_uint2(v[0], v[1]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                a.cb[coff + i * a.c_step] = (uint8_t)byte_of(u, i);
                a.cr[coff + i * a.c_step] = (uint8_t)byte_of(v, i);
            }
        }
        return;
    }
    // a row's last, partial strip: block by block
    for (int i = 0; i < s.m; i += 2) {
        int sum[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const uint8_t* const p = Pr[r] + (i + dx) * C;
                int rgb[3];
                rgb_of<C, RFIRST>(p[0], p[S1], p[S2], rgb);
                Yr[r][i + dx] = (uint8_t)luma_of(k, rgb);
                sum[0] += rgb[0], sum[1] += rgb[1], sum[2] += rgb[2];
            }
        a.cb[coff + (i >> 1) * a.c_step] = (uint8_t)chroma_of(k.kcb, sum);
        a.cr[coff + (i >> 1) * a.c_step] = (uint8_t)chroma_of(k.kcr, sum);
    }
}

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// One launch of either direction on device pointers whose sizes, strides and
// extents the entry points have checked (l: the resolved strides).
hipError_t launch_yuv420(bool to_frames, uint8_t* y, uint8_t* cb, uint8_t* cr, const Yuv420Layout& l, int c_step,
                         int matrix, int range, int n, int W, int H, uint8_t* p, size_t p_stride, size_t p_image_stride,
                         int format, int alpha, hipStream_t s)
{
    const long long blocks = yuv420_blocks(n, W, H);
    const int C = frame_format_channels(format);
    if (blocks < 1 || !C) return hipErrorInvalidValue;
    YuvArgs a{};
    a.y = y, a.cb = cb, a.cr = cr, a.p = p;
    a.W = W, a.H2 = H / 2, a.cw = (W + kStrip - 1) / kStrip;
    a.items = (long long)n * a.H2 * a.cw;
    a.y_stride = (long long)l.y_stride, a.y_image_stride = (long long)l.y_image_stride;
    a.c_stride = (long long)l.c_stride, a.c_image_stride = (long long)l.c_image_stride;
    a.p_stride = (long long)p_stride, a.p_image_stride = (long long)p_image_stride;
    a.c_step = c_step;
    a.alpha = alpha;
    a.to_rgb = kToRgb[matrix * 2 + range];
    a.to_yuv = kToYuv[matrix * 2 + range];
    // (a stack of one image never applies its image stride; a surface of two rows never its chroma row stride)
    const size_t one = n > 1 ? ~size_t(0) : 0, rows = H > 2 ? ~size_t(0) : 0;
    a.vec_y = ((addr(y) | l.y_stride | (l.y_image_stride & one)) & 15) == 0;
    a.vec_p = ((addr(p) | p_stride | (p_image_stride & one)) & 15) == 0;
    const size_t c_strides = (l.c_stride & rows) | (l.c_image_stride & one);
    a.vec_c = kChromaBytes;
    if (cb && cr) {
        if (c_step == 2 && (cb + 1 == cr || cr + 1 == cb)) {
            a.cr_first = cr < cb;
            if ((((a.cr_first ? addr(cr) : addr(cb)) | c_strides) & 15) == 0) a.vec_c = kChromaInterleaved;
        } else if (c_step == 1 && ((addr(cb) | addr(cr) | c_strides) & 7) == 0) {
            a.vec_c = kChromaPlanar;
        }
    }
    const dim3 grid((unsigned)blocks), block(kYuvThreads);
    const Timing t{};
#define DIS_YUV_LAUNCH(K)                                                                         \
    switch (format) {                                                                             \
        case DIS_FRAME_GRAY8: DIS_LAUNCH(t, (K<1, true>), grid, block, 0, s, a); break;           \
        case DIS_FRAME_BGR8: DIS_LAUNCH(t, (K<3, false>), grid, block, 0, s, a); break;           \
        case DIS_FRAME_RGB8: DIS_LAUNCH(t, (K<3, true>), grid, block, 0, s, a); break;            \
        case DIS_FRAME_BGRA8: DIS_LAUNCH(t, (K<4, false>), grid, block, 0, s, a); break;          \
        default: DIS_LAUNCH(t, (K<4, true>), grid, block, 0, s, a); break;                        \
    }
    if (to_frames) {
        DIS_YUV_LAUNCH(k_yuv420_to_frames)
    } else {
        DIS_YUV_LAUNCH(k_frames_to_yuv420)
    }
#undef DIS_YUV_LAUNCH
    return hipGetLastError();
}

// Host pointers: the whole extents of the planes (first image's first byte to
// last image's last sample), merged where they share bytes or touch -- the
// planes of an NV12 or I420 surface of several images lie inside each other's
// extents -- so that every host byte has one device copy.
struct HostSpan {
    uintptr_t lo, hi;
    uint8_t* dev;
};
int merge_spans(const PlaneStack* r, int count, int n, HostSpan* out)
{
    int m = 0;
    for (int k = 0; k < count; ++k)
        if (r[k].p && r[k].image_bytes)
            out[m++] = {r[k].p, r[k].p + (size_t)(n - 1) * r[k].image_stride + r[k].image_bytes, nullptr};
    for (bool again = true; again;) {
        again = false;
        for (int i = 0; i < m && !again; ++i)
            for (int j = i + 1; j < m && !again; ++j)
                if (out[i].lo <= out[j].hi && out[j].lo <= out[i].hi) {
                    out[i].lo = out[i].lo < out[j].lo ? out[i].lo : out[j].lo;
                    out[i].hi = out[i].hi > out[j].hi ? out[i].hi : out[j].hi;
                    out[j] = out[--m];
                    again = true;
                }
    }
    return m;
}
uint8_t* device_of(const HostSpan* sp, int m, const void* host)
{
    const uintptr_t p = addr(host);
    for (int i = 0; i < m; ++i)
        if (p && p >= sp[i].lo && p < sp[i].hi && sp[i].dev) return sp[i].dev + (p - sp[i].lo);
    return nullptr;
}

// what both entry points check alike; *C: the format's channels
const char* check_common(int frame_format, int matrix, int range, int alpha, dis_mem where, int* C)
{
    *C = frame_format_channels(frame_format);
    if (!*C) return "frame_format must be a dis_frame_format";
    if (matrix != DIS_YUV_BT601 && matrix != DIS_YUV_BT709) return "matrix must be DIS_YUV_BT601 or DIS_YUV_BT709";
    if (range != DIS_YUV_LIMITED && range != DIS_YUV_FULL) return "range must be DIS_YUV_LIMITED or DIS_YUV_FULL";
    if (alpha < 0 || alpha > 255) return "alpha must be in [0, 255]";
    if (where != DIS_MEM_HOST && where != DIS_MEM_DEVICE) return "bad dis_mem";
    return nullptr;
}

}  // namespace
}  // namespace dis

extern "C" {

dis_status dis_yuv420_to_frames_u8(const uint8_t* y, size_t y_stride, size_t y_image_stride, const uint8_t* cb,
                                   const uint8_t* cr, size_t c_stride, size_t c_image_stride, int c_step, int matrix,
                                   int range, int n, int width, int height, uint8_t* dst, size_t dst_stride,
                                   size_t dst_image_stride, int frame_format, int alpha, dis_mem where, void* stream,
                                   int device)
{
    using namespace dis;
    int C;
    DIS_ARG(check_common(frame_format, matrix, range, alpha, where, &C));
    if (C == 1) cb = cr = nullptr;  // a gray target reads no chroma
    if (!y || !dst || (C > 1 && (!cb || !cr))) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    Yuv420Layout l;
    DIS_ARG(check_yuv420_layout(n, width, height, c_step, y_stride, y_image_stride, c_stride, c_image_stride, &l));
    if (yuv420_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    ImageStack om;
    DIS_ARG(check_image_stack(width, height, C, n, dst_stride, dst_image_stride, &om));
    PlaneStack r[4] = {{addr(y), l.y_image_stride, l.y_bytes, "y"}};
    const int nin = 1 + yuv420_chroma_planes(addr(cb), addr(cr), c_step, l, r + 1);
    r[nin] = {addr(dst), om.image_stride, (size_t)(height - 1) * om.stride + (size_t)width * C, "dst"};
    PairMessage why;
    DIS_ARG(check_plane_stacks(r, nin, nin + 1, n, &why));
    if (dis_status st = use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* const y_ = const_cast<uint8_t*>(y);
    uint8_t* const cb_ = const_cast<uint8_t*>(cb);
    uint8_t* const cr_ = const_cast<uint8_t*>(cr);
    if (where == DIS_MEM_DEVICE) {
        DIS_HIP(launch_yuv420(true, y_, cb_, cr_, l, c_step, matrix, range, n, width, height, dst, om.stride,
                              om.image_stride, frame_format, alpha, s));
        return DIS_OK;
    }
    // the surface is staged as it lies; the frames go up as they are and come down
    // whole, so the caller's padding keeps its bytes
    HostStage st(s);
    HostSpan sp[3];
    const int m = merge_spans(r, nin, n, sp);
    for (int i = 0; i < m; ++i)
        sp[i].dev = const_cast<uint8_t*>(st.in(reinterpret_cast<const uint8_t*>(sp[i].lo), sp[i].hi - sp[i].lo));
    uint8_t* const ddst = st.out(dst, om.bytes);
    return st.finish(
        [&] {
            const hipError_t e = hipMemcpyAsync(ddst, dst, om.bytes, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return e;
            return launch_yuv420(true, device_of(sp, m, y), device_of(sp, m, cb), device_of(sp, m, cr), l, c_step,
                                 matrix, range, n, width, height, ddst, om.stride, om.image_stride, frame_format,
                                 alpha, s);
        },
        "4:2:0 to frames conversion");
}

dis_status dis_frames_to_yuv420_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int frame_format,
                                   int matrix, int range, int n, int width, int height, uint8_t* y, size_t y_stride,
                                   size_t y_image_stride, uint8_t* cb, uint8_t* cr, size_t c_stride,
                                   size_t c_image_stride, int c_step, dis_mem where, void* stream, int device)
{
    using namespace dis;
    int C;
    DIS_ARG(check_common(frame_format, matrix, range, 0, where, &C));
    if (!src || !y || !cb || !cr) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    Yuv420Layout l;
    DIS_ARG(check_yuv420_layout(n, width, height, c_step, y_stride, y_image_stride, c_stride, c_image_stride, &l));
    if (yuv420_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    ImageStack im;
    DIS_ARG(check_image_stack(width, height, C, n, src_stride, src_image_stride, &im));
    PlaneStack r[4] = {{addr(src), im.image_stride, (size_t)(height - 1) * im.stride + (size_t)width * C, "src"},
                       {addr(y), l.y_image_stride, l.y_bytes, "y"}};
    const int count = 2 + yuv420_chroma_planes(addr(cb), addr(cr), c_step, l, r + 2);
    PairMessage why;
    DIS_ARG(check_plane_stacks(r, 1, count, n, &why));
    if (dis_status st = use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* const src_ = const_cast<uint8_t*>(src);
    if (where == DIS_MEM_DEVICE) {
        DIS_HIP(launch_yuv420(false, y, cb, cr, l, c_step, matrix, range, n, width, height, src_, im.stride,
                              im.image_stride, frame_format, 0, s));
        return DIS_OK;
    }
    // the frames are staged as they lie; the surface goes up as it is and comes
    // down whole, so the padding and the bytes between the planes keep theirs
    HostStage st(s);
    const uint8_t* const dsrc = st.in(src, im.bytes);
    HostSpan sp[3];
    const int m = merge_spans(r + 1, count - 1, n, sp);
    for (int i = 0; i < m; ++i) sp[i].dev = st.out(reinterpret_cast<uint8_t*>(sp[i].lo), sp[i].hi - sp[i].lo);
    return st.finish(
        [&] {
            for (int i = 0; i < m; ++i) {
                const hipError_t e = hipMemcpyAsync(sp[i].dev, reinterpret_cast<const void*>(sp[i].lo),
                                                    sp[i].hi - sp[i].lo, hipMemcpyHostToDevice, s);
                if (e != hipSuccess) return e;
            }
            return launch_yuv420(false, device_of(sp, m, y), device_of(sp, m, cb), device_of(sp, m, cr), l, c_step,
                                 matrix, range, n, width, height, const_cast<uint8_t*>(dsrc), im.stride,
                                 im.image_stride, frame_format, 0, s);
        },
        "frames to 4:2:0 conversion");
}

}  // extern "C"
