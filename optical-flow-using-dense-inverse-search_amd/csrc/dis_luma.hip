// dis_luma.hip -- interleaved 8-bit colour frames to 8-bit gray
// (dis_frames_to_gray_u8, and the front stage of a context whose frame format
// is not DIS_FRAME_GRAY8; include/dis_abi.h). The reference gets gray frames
// from cv::imread(..., GRAYSCALE) (src/main.cpp:115-116); this is that
// conversion's arithmetic, OpenCV's fixed-point Rec.601 with a 14-bit shift,
//   gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14,
// which cli/png.hpp (png::detail::luma) and tests/lumaref.py restate. Integers
// only: the coefficients sum to 2^14 (R = G = B = v gives v) and the largest
// sum is 4,186,112 < 2^24, so 24-bit multiplies are exact. Alpha is ignored.
//
// One streaming launch, no LDS, no barriers. A lane owns 16 consecutive pixels
// of a row: 48 or 64 source bytes in, 16 gray bytes out. When the source base
// and both of its strides are multiples of 16, a full group is three or four
// 16-byte loads, all issued before the first is consumed; when the destination
// base and strides are, it is one 16-byte store. A row's last, partial group
// and every group of an unaligned source go byte by byte, and an unaligned
// destination is written byte by byte: the same bytes, and in every form no
// byte after a row's last sample is read and none after a row's last pixel
// written. DIS_FRAME_GRAY8 is the same kernel with one byte per pixel (a
// strided copy). A launch takes up to two stacks of n images (the two frames
// of a batch of pairs), so the front stage is one launch.
#include <cstdint>

#include "dis_kernels.h"

namespace dis {
namespace {

constexpr int kLumaThreads = 256;
constexpr int kLumaGroup = 16;  // pixels per lane

struct LumaArgs {
    const uint8_t* src[2];  // stacks of n images each; src[1] is null for one stack
    uint8_t* dst[2];
    long long items;        // stacks * n * H * cw lanes of work
    long long src_stride, src_image_stride, dst_stride, dst_image_stride;  // bytes
    int n, W, H, cw;        // cw = ceil(W / 16) lanes per row
    int vec_src;            // every source base and both source strides are multiples of 16
    int vec_dst;            // ... and the destination's
};

__device__ __forceinline__ unsigned luma(unsigned r, unsigned g, unsigned b)
{
    return (__umul24(r, 4899u) + __umul24(g, 9617u) + __umul24(b, 1868u) + 8192u) >> 14;
}

// the gray byte of a pixel whose samples are s[0..C): C = 1 is gray itself,
// RFIRST says which end the red sample is at
template <int C, bool RFIRST>
__device__ __forceinline__ unsigned gray_of(unsigned s0, unsigned s1, unsigned s2)
{
    if constexpr (C == 1) return s0;
    return RFIRST ? luma(s0, s1, s2) : luma(s2, s1, s0);
}

// byte j of a lane's source words (j is a constant after unrolling)
__device__ __forceinline__ unsigned byte_of(const unsigned* w, int j) { return (w[j >> 2] >> ((j & 3) * 8)) & 0xffu; }

template <int C, bool RFIRST>
__global__ void __launch_bounds__(kLumaThreads) k_frames_to_gray(LumaArgs a)
{
    const long long t = (long long)blockIdx.x * kLumaThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // (stack * n + image) * H + y
    const int x0 = (int)(t - row * a.cw) * kLumaGroup;
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const int stack = f >= a.n ? 1 : 0;
    const long long img = f - (stack ? a.n : 0);
    const uint8_t* const S = (stack ? a.src[1] : a.src[0]) + img * a.src_image_stride + y * a.src_stride + (long long)x0 * C;
    uint8_t* const D = (stack ? a.dst[1] : a.dst[0]) + img * a.dst_image_stride + y * a.dst_stride + x0;
    const int m = min(kLumaGroup, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    if (m == kLumaGroup && a.vec_src) {
        // (x0 * C is a multiple of 16: so is S, and the group ends inside the row)
        unsigned w[4 * C];
        const uint4* const v = reinterpret_cast<const uint4*>(S);
        uint4 q[C];
#pragma unroll
        for (int k = 0; k < C; ++k) q[k] = v[k];  // every load first
#pragma unroll
        for (int k = 0; k < C; ++k) {
            w[4 * k] = q[k].x;
            w[4 * k + 1] = q[k].y;
            w[4 * k + 2] = q[k].z;
            w[4 * k + 3] = q[k].w;
        }
        unsigned o[4] = {0u, 0u, 0u, 0u};  // the 16 gray bytes, in store order
#pragma unroll
        for (int i = 0; i < kLumaGroup; ++i) {
            const unsigned g = gray_of<C, RFIRST>(byte_of(w, C * i), byte_of(w, C * i + (C > 1 ? 1 : 0)),
                                                  byte_of(w, C * i + (C > 1 ? 2 : 0)));
            o[i >> 2] |= g << ((i & 3) * 8);
        }
        if (a.vec_dst) {
            *reinterpret_cast<uint4*>(D) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int i = 0; i < kLumaGroup; ++i) D[i] = (uint8_t)(o[i >> 2] >> ((i & 3) * 8));
        }
        return;
    }
    // the general form: a partial group, or a source that is not 16-byte aligned
    for (int i = 0; i < m; ++i) {
        const uint8_t* const p = S + i * C;
        D[i] = (uint8_t)gray_of<C, RFIRST>(p[0], p[C > 1 ? 1 : 0], p[C > 1 ? 2 : 0]);
    }
}

template <int C, bool RFIRST>
void launch_luma_c(const LumaArgs& a, unsigned grid, hipStream_t s, Timing t)
{
    DIS_LAUNCH(t, (k_frames_to_gray<C, RFIRST>), dim3(grid), dim3(kLumaThreads), 0, s, a);
}

}  // namespace

int frame_format_channels(int format)
{
    switch (format) {
        case DIS_FRAME_GRAY8: return 1;
        case DIS_FRAME_BGR8:
        case DIS_FRAME_RGB8: return 3;
        case DIS_FRAME_BGRA8:
        case DIS_FRAME_RGBA8: return 4;
        default: return 0;
    }
}

static_assert(kLumaThreads == kFlatThreads && kLumaGroup == kLumaGroupPixels,
              "frames_to_gray_blocks (dis_args.h) counts blocks of 256 lanes of 16 pixels");

hipError_t launch_frames_to_gray(const uint8_t* src0, const uint8_t* src1, size_t src_stride, size_t src_image_stride,
                                 int format, int n, int W, int H, uint8_t* dst0, uint8_t* dst1, size_t dst_stride,
                                 size_t dst_image_stride, hipStream_t s, Timing t)
{
    const int stacks = src1 ? 2 : 1;
    const long long blocks = frames_to_gray_blocks((long long)stacks * n, W, H);
    if (blocks < 1 || !frame_format_channels(format) || !src0 || !dst0 || (src1 && !dst1)) return hipErrorInvalidValue;
    LumaArgs a{};
    a.src[0] = src0;
    a.src[1] = src1;
    a.dst[0] = dst0;
    a.dst[1] = dst1;
    a.n = n;
    a.W = W;
    a.H = H;
    a.cw = (int)(((long long)W + kLumaGroup - 1) / kLumaGroup);
    a.items = (long long)stacks * n * H * a.cw;
    a.src_stride = (long long)src_stride;
    a.src_image_stride = (long long)src_image_stride;
    a.dst_stride = (long long)dst_stride;
    a.dst_image_stride = (long long)dst_image_stride;
    // (a stack of one image never applies its image stride, as PyramidArgs.qword_ok has it)
    const size_t s_img = n > 1 ? src_image_stride : 0, d_img = n > 1 ? dst_image_stride : 0;
    a.vec_src = ((reinterpret_cast<uintptr_t>(src0) | reinterpret_cast<uintptr_t>(src1) | src_stride | s_img) & 15) == 0;
    a.vec_dst = ((reinterpret_cast<uintptr_t>(dst0) | reinterpret_cast<uintptr_t>(dst1) | dst_stride | d_img) & 15) == 0;
    const unsigned grid = (unsigned)blocks;
    switch (format) {
        case DIS_FRAME_GRAY8: launch_luma_c<1, true>(a, grid, s, t); break;
        case DIS_FRAME_BGR8: launch_luma_c<3, false>(a, grid, s, t); break;
        case DIS_FRAME_RGB8: launch_luma_c<3, true>(a, grid, s, t); break;
        case DIS_FRAME_BGRA8: launch_luma_c<4, false>(a, grid, s, t); break;
        default: launch_luma_c<4, true>(a, grid, s, t); break;
    }
    return hipGetLastError();
}

}  // namespace dis
