// dis_denoise.hip -- motion-compensated temporal denoising of u8 images
// (dis_temporal_denoise_u8, include/dis_abi.h). No reference counterpart.
//
// For every neighbour k the frame is warped to the current one by its flow
// (Wk, Vk: exactly dis_flow_warp_u8's bytes at scale 1, DIS_BORDER_REPLICATE)
// and blended in with a weight looked up by the mean absolute difference over
// the pixel's 3 x 3 window and all channels. Integers are exact, every float
// operation is separately rounded (-ffp-contract=off), so tests/denoiseref.py
// restates it bit for bit.
//
// One launch, a block of 256 lanes per 64 x 16 output tile. The block keeps the
// tile of `cur` plus a 1-pixel halo in LDS for the whole call; for each
// neighbour in turn it samples Wk on the same 66 x 18 cells (dis_sample.h's
// warp_pixel, f16 vectors widened once, the invalid vector and the mask folded
// into one byte per cell) into one of two LDS buffers, so that one barrier per
// neighbour is enough: lanes that fill buffer k + 1 never meet lanes that still
// read buffer k, and buffer k is filled again only after the barrier of k + 1.
// A halo cell outside the frame repeats the cell at the clamped position, which
// is what the window's clamp reads. Then each lane forms D_k for its 4
// consecutive pixels of a row from 3 x 6 cells read as dwords (its `cur` cells
// stay in registers over the loop) and accumulates num, the weight sum and the
// support count in registers. Nothing but dst and support is written.
//
// The weight table and the 3 x 8 pointers come by value in the kernel's
// arguments; the table is copied to LDS once per block. 4-channel taps and
// `cur` cells are dwords when every image pointer and stride is 4-byte aligned,
// dst goes out as one dword per lane (16 bytes with 4 channels) and support as
// one dword when aligned and W % 4 == 0; the scalar forms write the same bytes.
#include <cmath>
#include <cstdint>

#include "dis_args.h"
#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kDnThreads = 256;
constexpr int kDnTW = kDenoiseTileW, kDnTH = kDenoiseTileH;  // 64 x 16 outputs: 16 lanes a row, 4 pixels a lane
constexpr int kDnCW = kDnTW + 2, kDnCH = kDnTH + 2;          // cells with the halo
constexpr int kDnCells = kDnCW * kDnCH;
constexpr int kDnOkPitch = kDnCW + 2;  // (a multiple of 4)
static_assert(kDnTW == 64 && kDnTH * 16 == kDnThreads, "a lane per 4 pixels of a tile row");

struct DenoiseArgs {
    const uint8_t* cur;
    const uint8_t* nb[kDenoiseMaxNeighbours];
    const void* flow[kDenoiseMaxNeighbours];   // float2 or __half2 vectors
    const uint8_t* mask[kDenoiseMaxNeighbours];  // null: every vector trusted
    uint8_t* dst;
    uint8_t* support;  // may be null
    long long stride, image_stride;  // bytes, of cur and every neighbour
    int W, H, K;
    int tiles_x, tiles_y;
    int vec_img;      // 4 channels: cur, every neighbour and both strides 4-byte aligned, one dword per pixel
    int vec_dst;      // dst 4-byte (4 channels: 16-byte) aligned and W % 4 == 0: dword / 16-byte stores
    int vec_support;  // support 4-byte aligned and W % 4 == 0: one dword per lane
    float weights[256];
};

// bytes of an LDS row of cells, a multiple of 4 (every lane's first cell of a row is then dword-aligned)
template <int C>
constexpr int dn_pitch() { return (kDnCW * C + 3) / 4 * 4; }

__device__ __forceinline__ unsigned dn_byte(const unsigned* d, int i) { return (d[i >> 2] >> (8 * (i & 3))) & 255u; }

template <int C, bool F16>
__global__ void __launch_bounds__(kDnThreads) k_temporal_denoise(DenoiseArgs a)
{
    constexpr int P = dn_pitch<C>();
    constexpr int ND = (6 * C + 3) / 4;  // dwords that hold a lane's 6 cells of a row
    constexpr unsigned CNT = 9u * C;
    __shared__ float s_w[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_cur[kDnCH * P];
    __shared__ __attribute__((aligned(16))) uint8_t s_wk[2][kDnCH * P];
    __shared__ __attribute__((aligned(16))) uint8_t s_ok[2][kDnCH * kDnOkPitch];

    const int tid = threadIdx.x;
    const int per = a.tiles_x * a.tiles_y;
    const long long f = blockIdx.x / per;
    const int tile = (int)(blockIdx.x - f * per);
    const int tyi = tile / a.tiles_x;
    const int x0 = (tile - tyi * a.tiles_x) * kDnTW, y0 = tyi * kDnTH;
    const int W = a.W, H = a.H;

    s_w[tid] = a.weights[tid];
    {
        const uint8_t* const S = a.cur + f * a.image_stride;
        for (int i = tid; i < kDnCells; i += kDnThreads) {
            const int cy = i / kDnCW, cx = i - cy * kDnCW;
            const int gx = min(max(x0 + cx - 1, 0), W - 1), gy = min(max(y0 + cy - 1, 0), H - 1);
            const uint8_t* const g = S + gy * a.stride + (long long)gx * C;
            uint8_t* const l = s_cur + cy * P + cx * C;
            if (C == 4 && a.vec_img) {
                *reinterpret_cast<unsigned*>(l) = *reinterpret_cast<const unsigned*>(g);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) l[c] = g[c];
            }
        }
    }
    __syncthreads();

    const int row = tid >> 4, col4 = (tid & 15) * 4;  // this lane's pixels: (x0 + col4 .. + 3, y0 + row)
    unsigned cw[3][ND];  // its 3 x 6 cells of cur
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int d = 0; d < ND; ++d)
            cw[r][d] = *reinterpret_cast<const unsigned*>(s_cur + (row + r) * P + col4 * C + 4 * d);

    float num[4][C], sw[4];
    unsigned sup[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sw[i] = 0.0f;
        sup[i] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) num[i][c] = 0.0f;
    }

    for (int k = 0; k < a.K; ++k) {
        const int b = k & 1;
        const uint8_t* const S = a.nb[k] + f * a.image_stride;
        const uint8_t* const M = a.mask[k];
        for (int i = tid; i < kDnCells; i += kDnThreads) {
            const int cy = i / kDnCW, cx = i - cy * kDnCW;
            const int gx = min(max(x0 + cx - 1, 0), W - 1), gy = min(max(y0 + cy - 1, 0), H - 1);
            const long long p = (f * H + gy) * W + gx;
            float2 q;
            if constexpr (F16)
                q = widen2(static_cast<const __half2*>(a.flow[k])[p]);
            else
                q = static_cast<const float2*>(a.flow[k])[p];
            unsigned o[C];
            unsigned v = warp_pixel<C>(S, a.stride, gx, gy, W, H, q.x, q.y, 1.0f, 0, a.vec_img, o);
            if (M && M[p] == 0) v = 0u;
            uint8_t* const l = s_wk[b] + cy * P + cx * C;
            if constexpr (C == 4) {
                *reinterpret_cast<unsigned*>(l) = pack4(o);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) l[c] = (uint8_t)o[c];
            }
            s_ok[b][cy * kDnOkPitch + cx] = v ? 1 : 0;
        }
        __syncthreads();

        unsigned col[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // |Wk - cur| summed over a column of 3 cells and the channels
        unsigned wc[ND];                            // the middle row of Wk
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            unsigned ww[ND];
#pragma unroll
            for (int d = 0; d < ND; ++d)
                ww[d] = *reinterpret_cast<const unsigned*>(s_wk[b] + (row + r) * P + col4 * C + 4 * d);
#pragma unroll
            for (int j = 0; j < 6 * C; ++j) {
                const int x = (int)dn_byte(ww, j), y = (int)dn_byte(cw[r], j);
                col[j / C] += (unsigned)abs(x - y);
            }
            if (r == 1) {
#pragma unroll
                for (int d = 0; d < ND; ++d) wc[d] = ww[d];
            }
        }
        const uint8_t* const okr = s_ok[b] + (row + 1) * kDnOkPitch + col4 + 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned D = col[i] + col[i + 1] + col[i + 2];
            const unsigned idx = (D + CNT / 2) / CNT;  // 0..255
            const bool ok = okr[i] != 0;
            const float w = ok ? s_w[idx] : 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int diff = (int)dn_byte(wc, (i + 1) * C + c) - (int)dn_byte(cw[1], (i + 1) * C + c);
                const float t = w * (float)diff;
                num[i][c] = num[i][c] + t;
            }
            sw[i] = sw[i] + w;
            sup[i] += (ok && w > 0.0f) ? 1u : 0u;
        }
    }

    const int y = y0 + row, xb = x0 + col4;
    if (y >= H || xb >= W) return;
    const int m = min(4, W - xb);
    unsigned o[4 * C];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float den = 1.0f + sw[i];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float q = num[i][c] / den;
            const float r = (float)dn_byte(cw[1], (i + 1) * C + c) + q;
            o[C * i + c] = (unsigned)fminf(fmaxf(rintf(r), 0.0f), 255.0f);
        }
    }
    const long long p0 = (f * H + y) * W + xb;
    uint8_t* const d = a.dst + p0 * C;
    if (a.vec_dst) {  // (W % 4 == 0: m == 4, p0 * C a multiple of 4, of 16 with 4 channels)
        if constexpr (C == 4) {
            *reinterpret_cast<uint4*>(d) = make_uint4(pack4(o), pack4(o + 4), pack4(o + 8), pack4(o + 12));
        } else {
#pragma unroll
            for (int j = 0; j < C; ++j) reinterpret_cast<unsigned*>(d)[j] = pack4(o + 4 * j);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) {
#pragma unroll
                for (int c = 0; c < C; ++c) d[C * i + c] = (uint8_t)o[C * i + c];
            }
    }
    if (!a.support) return;
    if (a.vec_support) {
        *reinterpret_cast<unsigned*>(a.support + p0) = pack4(sup);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.support[p0 + i] = (uint8_t)sup[i];
    }
}

template <int C>
void launch_denoise_c(const DenoiseArgs& a, bool f16, unsigned grid, hipStream_t s, Timing t)
{
    if (f16)
        DIS_LAUNCH(t, (k_temporal_denoise<C, true>), dim3(grid), dim3(kDnThreads), 0, s, a);
    else
        DIS_LAUNCH(t, (k_temporal_denoise<C, false>), dim3(grid), dim3(kDnThreads), 0, s, a);
}

}  // namespace

hipError_t launch_temporal_denoise(const uint8_t* cur, const uint8_t* const* neighbours, size_t stride,
                                   size_t image_stride, int channels, const void* const* flows, int f16,
                                   const uint8_t* const* masks, int k_neighbours, int n, int W, int H,
                                   const float* weights, uint8_t* dst, uint8_t* support, hipStream_t s, Timing t)
{
    const long long blocks = denoise_blocks(n, W, H);
    if (blocks < 1 || k_neighbours < 1 || k_neighbours > kDenoiseMaxNeighbours ||
        (channels != 1 && channels != 3 && channels != 4))
        return hipErrorInvalidValue;
    DenoiseArgs a{};
    uintptr_t img = reinterpret_cast<uintptr_t>(cur) | stride | image_stride;
    a.cur = cur;
    for (int k = 0; k < k_neighbours; ++k) {
        a.nb[k] = neighbours[k];
        a.flow[k] = flows[k];
        a.mask[k] = masks ? masks[k] : nullptr;
        img |= reinterpret_cast<uintptr_t>(neighbours[k]);
    }
    a.dst = dst;
    a.support = support;
    a.stride = (long long)stride;
    a.image_stride = (long long)image_stride;
    a.W = W;
    a.H = H;
    a.K = k_neighbours;
    a.tiles_x = (W + kDnTW - 1) / kDnTW;
    a.tiles_y = (H + kDnTH - 1) / kDnTH;
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(support);
    a.vec_img = (channels == 4 && (img & 3) == 0) ? 1 : 0;
    a.vec_dst = ((da & (channels == 4 ? 15 : 3)) == 0 && (W & 3) == 0) ? 1 : 0;
    a.vec_support = (support && (sa & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    for (int i = 0; i < 256; ++i) a.weights[i] = weights[i];
    const unsigned grid = (unsigned)blocks;
    if (channels == 1)
        launch_denoise_c<1>(a, f16 != 0, grid, s, t);
    else if (channels == 3)
        launch_denoise_c<3>(a, f16 != 0, grid, s, t);
    else
        launch_denoise_c<4>(a, f16 != 0, grid, s, t);
    return hipGetLastError();
}

}  // namespace dis
