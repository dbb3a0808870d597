// dis_args.h -- the argument rules of the C-ABI that need nothing but integers:
// sizes, strides, byte extents and which buffers may share memory. Host-only
// and pure (no HIP, no allocation, nothing dereferenced; addresses are
// uintptr_t): tests/cpp/args_host.cpp runs them under the host sanitizers.
// Each rule returns nullptr if the call may go ahead, else what is wrong.
#pragma once

#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

namespace dis {

constexpr int kMaxExactSide = 1 << 24;        // pixel coordinates up to here are exact floats
constexpr long long kMaxKeyPixels = 1ll << 31;  // interpolation: a source index fills the low half of a key

inline const char* check_dims(int n, int width, int height, int max_side = INT_MAX, long long max_pixels = LLONG_MAX)
{
    if (n < 1 || width < 1 || height < 1) return "n, width, height must be >= 1";
    if (width > max_side || height > max_side) return "width or height too large";
    if ((long long)width * height > max_pixels) return "width * height too large";
    return nullptr;
}

// A stack of n strided images (warp, interpolation); a stride of 0 means tight.
// `bytes` ends with the last sample: the padding after the last row or image is
// not part of the source. The limits keep every product below 2^63.
struct ImageStack {
    size_t stride, image_stride, bytes;
};
inline const char* check_image_stack(int width, int height, int channels, int n, size_t stride, size_t image_stride,
                                     ImageStack* out)
{
    if (n < 1 || width < 1 || height < 1 || channels < 1) return "n, width, height, channels must be >= 1";
    const size_t row = (size_t)width * channels;
    if (!stride) stride = row;
    if (stride < row) return "stride smaller than a row";
    if (stride > (size_t(1) << 48) / (size_t)height) return "stride too large";
    if (!image_stride) image_stride = stride * height;
    if (image_stride < stride * height) return "image_stride smaller than an image";
    if (image_stride > (size_t(1) << 62) / (size_t)n) return "image_stride too large";
    *out = {stride, image_stride, (n - 1) * image_stride + (height - 1) * stride + row};
    return nullptr;
}

// The frame batch of the calc entry points: n pairs of W x H pixels of
// pixel_bytes interleaved u8 samples (1: gray; 3 or 4 under a colour
// dis_frame_format), frame k of either role at k * pair_stride (which a single
// pair does not need). Strides are bytes; `bytes` ends with the last sample.
struct FrameBatch {
    size_t stride, pair_stride, bytes;
};
inline const char* check_frame_batch(int W, int H, int n, int max_batch, size_t stride, size_t pair_stride,
                                     FrameBatch* out, int pixel_bytes = 1)
{
    if (n < 1 || n > max_batch) return "n must be in [1, max_batch]";
    if (pixel_bytes < 1) return "pixel_bytes must be >= 1";
    const size_t row = (size_t)W * pixel_bytes;
    if (!stride) stride = row;
    if (stride < row) return pixel_bytes == 1 ? "stride < width" : "stride smaller than a row of the frame format";
    if (!pair_stride) pair_stride = stride * H;
    if (n > 1 && pair_stride < stride * H) return "pair_stride too small";
    *out = {stride, pair_stride, (size_t)(n - 1) * pair_stride + (size_t)(H - 1) * stride + row};
    return nullptr;
}

// [a, a + na) and [b, b + nb) share a byte (empty ranges share none; the sums
// are formed so that a range ending at the top of the address space does not
// wrap)
inline bool ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb)
{
    if (na == 0 || nb == 0) return false;
    return a <= b ? b - a < na : a - b < nb;
}

// Of n named ranges, the first nin are inputs and the others outputs: every
// output must be disjoint from every input and from every other output (an
// absent buffer is an empty range). The first offending pair, by name.
struct NamedRange {
    uintptr_t p;
    size_t bytes;
    const char* name;
};
struct PairMessage {
    char text[64];
};
inline bool first_overlap(const NamedRange* r, int nin, int n, int* a, int* b)
{
    for (int o = nin; o < n; ++o)
        for (int k = 0; k < n; ++k)  // every input, then the outputs after this one
            if ((k < nin || k > o) && ranges_overlap(r[o].p, r[o].bytes, r[k].p, r[k].bytes)) {
                *a = o, *b = k;
                return true;
            }
    return false;
}
inline const char* check_disjoint(const NamedRange* r, int nin, int n, PairMessage* why)
{
    int a, b;
    if (!first_overlap(r, nin, n, &a, &b)) return nullptr;
    size_t k = 0;  // "<a> and <b> overlap", cut to fit
    for (const char* part : {r[a].name, " and ", r[b].name, " overlap"})
        for (; *part && k + 1 < sizeof why->text; ++part) why->text[k++] = *part;
    why->text[k] = 0;
    return why->text;
}

// A warm-started call (dis_calc_batch_init_u8): `init` may start exactly where
// `flow` starts (flow in, flow out: the init plane is complete before any
// output is written), otherwise the two must be disjoint; `init` must not
// touch either frame batch.
inline const char* check_init_aliasing(uintptr_t init, size_t init_bytes, uintptr_t flow, size_t flow_bytes,
                                       uintptr_t i0, uintptr_t i1, size_t frame_bytes)
{
    if (init != flow && ranges_overlap(init, init_bytes, flow, flow_bytes))
        return "init partially overlaps flow (it may be the flow buffer itself, or disjoint from it)";
    if (ranges_overlap(init, init_bytes, i0, frame_bytes) || ranges_overlap(init, init_bytes, i1, frame_bytes))
        return "init overlaps the frames";
    return nullptr;
}

// As check_disjoint, but each listed output may be one listed input itself
// (dis_flow_compose's out / a and valid_out / valid_a, dis_flow_advect_points'
// points_out / points: in place, every lane reads its own elements before it
// writes them): the output may start exactly at that input, otherwise the two
// must be disjoint. The caller lists a pair only when both hold elements of one
// size (equal formats), so that equal starts mean equal extents. Every other
// pair stays as in check_disjoint. The first offending pair, by name.
struct MayAlias {
    int out, in;  // indices into the ranges
};
inline const char* check_disjoint_or_same(const NamedRange* r, int nin, int n, const MayAlias* may, int nmay,
                                          PairMessage* why)
{
    for (int o = nin; o < n; ++o)
        for (int k = 0; k < n; ++k) {
            if (!(k < nin || k > o) || !ranges_overlap(r[o].p, r[o].bytes, r[k].p, r[k].bytes)) continue;
            bool same = false;
            for (int j = 0; j < nmay; ++j) same = same || (may[j].out == o && may[j].in == k && r[o].p == r[k].p);
            if (same) continue;
            const NamedRange pair[2] = {r[k], r[o]};
            return check_disjoint(pair, 1, 2, why);
        }
    return nullptr;
}

// The points of dis_flow_advect_points: n fields of `count` (x, y) float pairs
// each. *points = n * count; the limit keeps every byte count far below 2^63.
inline const char* check_points(int n, int count, size_t* points)
{
    if (n < 1 || count < 1) return "n and count must be >= 1";
    if ((long long)n * count > (1ll << 40)) return "n * count too large";
    *points = (size_t)n * (size_t)count;
    return nullptr;
}

// Blocks of the launches whose grid is one-dimensional over all images (256
// lanes a block); -1 when they exceed a grid, and the entry point refuses the
// call. Pure, so that tests/cpp can run them: the kernels' files assert the
// lane counts they assume.
constexpr int kFlatThreads = 256;

// dis_flow_warp_u8, dis_flow_consistency, dis_flow_compose and the blend of
// dis_flow_interp_u8: a lane per 4 pixels of a row, n * H rows.
inline long long row_quad_blocks(int n, int W, int H)
{
    const long long rows = (long long)n * H, cw = (W + 3) / 4;
    if (rows > 0x7fffffffLL * kFlatThreads / cw) return -1;
    return (rows * cw + kFlatThreads - 1) / kFlatThreads;
}
inline long long flow_warp_blocks(int n, int W, int H) { return row_quad_blocks(n, W, H); }
inline long long flow_consistency_blocks(int n, int W, int H) { return row_quad_blocks(n, W, H); }
inline long long flow_compose_blocks(int n, int W, int H) { return row_quad_blocks(n, W, H); }

// dis_flow_advect_points: a lane per point.
inline long long flow_advect_blocks(int n, int count)
{
    const long long items = (long long)n * count;
    if (items > 0x7fffffffLL * kFlatThreads) return -1;
    return (items + kFlatThreads - 1) / kFlatThreads;
}

// The splat of dis_flow_interp_u8: a lane per pixel (the blend's grid is
// smaller); -1 also when W * H exceeds 2^31.
inline long long flow_interp_blocks(int n, int W, int H)
{
    const long long wh = (long long)W * H;
    if (wh > (1ll << 31) || n > 0x7fffffffLL * kFlatThreads / wh) return -1;
    return (wh * n + kFlatThreads - 1) / kFlatThreads;
}

// dis_frames_to_gray_u8 (and the front stage of a colour context, which takes
// two stacks): a lane per 16 pixels of a row.
constexpr int kLumaGroupPixels = 16;
inline long long frames_to_gray_blocks(long long images, int W, int H)
{
    if (images < 1 || W < 1 || H < 1) return -1;
    const long long cw = ((long long)W + kLumaGroupPixels - 1) / kLumaGroupPixels;
    if (images > 0x7fffffffLL * kFlatThreads / cw / H) return -1;
    return (images * H * cw + kFlatThreads - 1) / kFlatThreads;
}

// The levels of dis_flow_fill's push-pull: level 0 is the W x H field, each
// further level halves both sides (rounding up) until 1 x 1 at level L. The
// workspace holds levels 1..L of every field, 8 bytes a cell: off[l] cells lie
// before level l in a field's part (off[0] is unused), `cells` in all.
constexpr int kMaxFillLevels = 25;  // sides up to 2^24: L <= 24
struct FillLevels {
    int L;
    int w[kMaxFillLevels], h[kMaxFillLevels];
    size_t off[kMaxFillLevels];
    size_t cells;
};
inline void fill_levels(int width, int height, FillLevels* g)
{
    int l = 0;
    g->w[0] = width, g->h[0] = height, g->off[0] = 0, g->cells = 0;
    while (g->w[l] > 1 || g->h[l] > 1) {
        g->w[l + 1] = (g->w[l] + 1) / 2, g->h[l + 1] = (g->h[l] + 1) / 2;
        g->off[l + 1] = g->cells;
        g->cells += (size_t)g->w[l + 1] * g->h[l + 1];
        ++l;
    }
    g->L = l;
}

// Blocks of one tile pass of the fill over n fields (a block per 64 x 32 cells
// of the pass's first level; level 0 has the most); -1 when they exceed a grid.
constexpr int kFillTileW = 64, kFillTileH = 32;
inline long long fill_tile_blocks(int n, int width, int height)
{
    const long long tx = ((long long)width + kFillTileW - 1) / kFillTileW;
    const long long ty = ((long long)height + kFillTileH - 1) / kFillTileH;
    if (n < 1 || tx * ty > 0x7fffffffLL / n) return -1;
    return tx * ty * n;
}

// dis_flow_fill_workspace: the sizes of dis_flow_fill, then 8 * n * cells (the
// grid limit keeps n * W * H below 2^42, so the product far below 2^63).
inline const char* check_fill_workspace(int n, int width, int height, size_t* bytes)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide)) return why;
    if (fill_tile_blocks(n, width, height) < 0) return "n * width * height too large for one launch";
    FillLevels g;
    fill_levels(width, height, &g);
    *bytes = 8 * (size_t)n * g.cells;
    return nullptr;
}

// dis_flow_fit_motion sums a field in chunks of 16384 pixels (row-major), a
// block per chunk and field; the last chunk of a field may be partial.
constexpr int kMotionChunk = 16384;
constexpr long long kMaxMotionPixels = 1ll << 31;  // a field's pixel index stays below 2^31 + one chunk
constexpr int kMotionTerms = 12;                   // sums of one chunk
constexpr int kMotionHead = 16;                    // doubles a field's part of the workspace begins with (the model)
inline long long motion_chunks(int width, int height)
{
    return ((long long)width * height + kMotionChunk - 1) / kMotionChunk;
}

// Blocks of one accumulation pass over n fields; -1 when they exceed a grid.
inline long long motion_blocks(int n, int width, int height)
{
    const long long c = motion_chunks(width, height);
    if (n < 1 || c < 1 || c > 0x7fffffffLL / n) return -1;
    return c * n;
}

// Blocks of dis_motion_to_flow's launch over n fields (256 lanes a block, a
// lane per 4 pixels of a row); -1 when they exceed a grid.
inline long long motion_flow_blocks(int n, int width, int height)
{
    const long long rows = (long long)n * height, cw = ((long long)width + 3) / 4;
    if (n < 1 || cw < 1 || rows > 0x7fffffffLL * 256 / cw) return -1;
    return (rows * cw + 255) / 256;
}

// The sizes of dis_motion_to_flow: the sides, the pixels and its grid.
inline const char* check_motion_flow(int n, int width, int height)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide, kMaxMotionPixels)) return why;
    if (motion_flow_blocks(n, width, height) < 0) return "n * width * height too large for one launch";
    return nullptr;
}

// dis_flow_fit_motion_workspace: the sizes of dis_flow_fit_motion (the sides,
// the pixels, the grid of a pass), then per field the head and twelve doubles
// per chunk (n * chunks fits a grid, so the product stays below 2^39).
inline const char* check_motion_workspace(int n, int width, int height, size_t* bytes)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide, kMaxMotionPixels)) return why;
    if (motion_blocks(n, width, height) < 0) return "n * width * height too large for one launch";
    *bytes = (size_t)n * ((size_t)motion_chunks(width, height) * kMotionTerms + kMotionHead) * 8;
    return nullptr;
}

// dis_flow_fit_homography: dis_flow_fit_motion's chunks, blocks and size rules
// with 27 sums a chunk; its coordinates are scaled by s, the smallest power of
// two >= max(W, H, 2) / 2 (so |a|, |b| < 1 and every division by s is exact).
constexpr int kHomographyTerms = 27;
inline int homography_scale(int width, int height)
{
    const int m = width > height ? (width > 2 ? width : 2) : (height > 2 ? height : 2);
    int s = 1;
    while (2 * (long long)s < m) s *= 2;
    return s;
}
inline const char* check_homography_workspace(int n, int width, int height, size_t* bytes)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide, kMaxMotionPixels)) return why;
    if (motion_blocks(n, width, height) < 0) return "n * width * height too large for one launch";
    *bytes = (size_t)n * ((size_t)motion_chunks(width, height) * kHomographyTerms + kMotionHead) * 8;
    return nullptr;
}

// dis_temporal_denoise_u8: a block per 64 x 16 output pixels and image, up to 8
// neighbours a call (their pointers travel in the kernel's arguments).
constexpr int kDenoiseMaxNeighbours = 8;
constexpr int kDenoiseTileW = 64, kDenoiseTileH = 16;

// Blocks of the launch over n images; -1 when they exceed a grid (which also
// keeps every byte count of the call far below 2^63).
inline long long denoise_blocks(int n, int width, int height)
{
    const long long tx = ((long long)width + kDenoiseTileW - 1) / kDenoiseTileW;
    const long long ty = ((long long)height + kDenoiseTileH - 1) / kDenoiseTileH;
    if (n < 1 || tx < 1 || ty < 1 || tx * ty > 0x7fffffffLL / n) return -1;
    return tx * ty * n;
}

// The sizes of dis_temporal_denoise_u8: the sides, the channels, the neighbour
// count and the grid.
inline const char* check_denoise_sizes(int k_neighbours, int n, int width, int height, int channels)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide)) return why;
    if (channels != 1 && channels != 3 && channels != 4) return "channels must be 1, 3 or 4";
    if (k_neighbours < 1 || k_neighbours > kDenoiseMaxNeighbours) return "k_neighbours must be in [1, 8]";
    if (denoise_blocks(n, width, height) < 0) return "n * width * height too large for one launch";
    return nullptr;
}

// One entry of the weight table: in [0, 1] (false for NaN and the infinities).
inline bool denoise_weight_ok(float w) { return w >= 0.0f && w <= 1.0f; }

// The buffers of dis_temporal_denoise_u8 by address: cur and the K neighbours
// (image_bytes each), the K flows (flow_bytes each), the K masks (pixels bytes
// each; `masks` may be null, and so may any of its entries), dst (dst_bytes) and
// support (pixels bytes, may be 0 = absent). No neighbour or flow may be null;
// dst and support must be disjoint from every input and from each other. For
// device pointers (flow_align = bytes of one (u,v) pair, else 0) every flow
// must be aligned to a pair.
inline const char* check_denoise_buffers(uintptr_t cur, const uintptr_t* neighbours, const uintptr_t* flows,
                                         const uintptr_t* masks, int k_neighbours, size_t image_bytes,
                                         size_t flow_bytes, size_t pixels, uintptr_t dst, size_t dst_bytes,
                                         uintptr_t support, size_t flow_align, PairMessage* why)
{
    static const char* const nb[kDenoiseMaxNeighbours] = {"neighbours[0]", "neighbours[1]", "neighbours[2]", "neighbours[3]",
                                                          "neighbours[4]", "neighbours[5]", "neighbours[6]", "neighbours[7]"};
    static const char* const fl[kDenoiseMaxNeighbours] = {"flows[0]", "flows[1]", "flows[2]", "flows[3]",
                                                          "flows[4]", "flows[5]", "flows[6]", "flows[7]"};
    static const char* const mk[kDenoiseMaxNeighbours] = {"masks[0]", "masks[1]", "masks[2]", "masks[3]",
                                                          "masks[4]", "masks[5]", "masks[6]", "masks[7]"};
    if (k_neighbours < 1 || k_neighbours > kDenoiseMaxNeighbours) return "k_neighbours must be in [1, 8]";
    NamedRange r[3 * kDenoiseMaxNeighbours + 3];
    int m = 0;
    r[m++] = {cur, image_bytes, "cur"};
    for (int k = 0; k < k_neighbours; ++k) {
        if (!neighbours[k] || !flows[k]) return "null entry in neighbours or flows";
        if (flow_align && (flows[k] & (flow_align - 1)))
            return "every flow must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16)";
        r[m++] = {neighbours[k], image_bytes, nb[k]};
        r[m++] = {flows[k], flow_bytes, fl[k]};
        const uintptr_t mp = masks ? masks[k] : 0;
        r[m++] = {mp, mp ? pixels : 0, mk[k]};
    }
    const int nin = m;
    r[m++] = {dst, dst_bytes, "dst"};
    r[m++] = {support, support ? pixels : 0, "support"};
    return check_disjoint(r, nin, m, why);
}

// dis_warp_motion_u8: a block per 64 x 16 output pixels and image (a lane per 4
// pixels of a row). Blocks of the launch over n images; -1 when they exceed a
// grid (which also keeps every byte count of the call far below 2^63).
constexpr int kWarpMotionTileW = 64, kWarpMotionTileH = 16;
inline long long warp_motion_blocks(int n, int width, int height)
{
    const long long tx = ((long long)width + kWarpMotionTileW - 1) / kWarpMotionTileW;
    const long long ty = ((long long)height + kWarpMotionTileH - 1) / kWarpMotionTileH;
    if (n < 1 || tx < 1 || ty < 1 || tx * ty > 0x7fffffffLL / n) return -1;
    return tx * ty * n;
}

// The sizes of dis_warp_motion_u8: the sides, the channels and the grid.
inline const char* check_warp_motion_sizes(int n, int width, int height, int channels)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide)) return why;
    if (channels != 1 && channels != 3 && channels != 4) return "channels must be 1, 3 or 4";
    if (warp_motion_blocks(n, width, height) < 0) return "n * width * height too large for one launch";
    return nullptr;
}

// The buffers of dis_warp_motion_u8 by address: src (image_bytes) and params
// (24 bytes an image) are read, dst and valid (pixels bytes, 0 = absent)
// written. params_align: 4 for device pointers, else 0.
inline const char* check_warp_motion_buffers(uintptr_t src, size_t image_bytes, uintptr_t params, int n, uintptr_t dst,
                                             size_t dst_bytes, uintptr_t valid, size_t pixels, size_t params_align,
                                             PairMessage* why)
{
    if (params_align && (params & (params_align - 1))) return "params must be 4-byte aligned";
    const NamedRange r[4] = {{src, image_bytes, "src"}, {params, (size_t)24 * (size_t)n, "params"},
                             {dst, dst_bytes, "dst"}, {valid, valid ? pixels : 0, "valid"}};
    return check_disjoint(r, 2, 4, why);
}

// dis_motion_stabilize: the values (a float compares false with everything
// when it is NaN, so each test is written to fail for one) ...
constexpr int kMaxStabilizeRadius = 1024;
inline const char* check_stabilize(int n_frames, int width, int height, int radius, float sigma, float zoom)
{
    if (n_frames < 1) return "n_frames must be >= 1";
    if (width < 1 || height < 1) return "width and height must be >= 1";
    if (width > kMaxExactSide || height > kMaxExactSide) return "width or height too large";
    if (radius < 0 || radius > kMaxStabilizeRadius) return "radius must be in [0, 1024]";
    if (!(sigma > 0.0f && sigma <= 3.40282347e38f)) return "sigma must be finite and > 0";
    if (!(zoom >= 1.0f && zoom <= 16.0f)) return "zoom must be finite and in [1, 16]";
    return nullptr;
}

// ... and the buffers by address: pair_params ((n_frames - 1) * 24 bytes) is
// read; corrections (n_frames * 24), status (n_frames, 0 = absent) and
// replaced (one int, 0 = absent) are written.
inline const char* check_stabilize_buffers(uintptr_t pair_params, uintptr_t corrections, uintptr_t status,
                                           uintptr_t replaced, int n_frames, PairMessage* why)
{
    const size_t n = (size_t)n_frames;
    const NamedRange r[4] = {{pair_params, pair_params ? (n - 1) * 24 : 0, "pair_params"},
                             {corrections, n * 24, "corrections"},
                             {status, status ? n : 0, "status"},
                             {replaced, replaced ? sizeof(int) : 0, "replaced"}};
    return check_disjoint(r, 1, 4, why);
}

// dis_warp_homography_u8 and dis_homography_stabilize: their affine siblings'
// sizes and values (check_warp_motion_sizes, check_stabilize) and the same
// buffer rules with 32 bytes a model.
inline const char* check_warp_homography_buffers(uintptr_t src, size_t image_bytes, uintptr_t params, int n,
                                                 uintptr_t dst, size_t dst_bytes, uintptr_t valid, size_t pixels,
                                                 size_t params_align, PairMessage* why)
{
    if (params_align && (params & (params_align - 1))) return "params must be 4-byte aligned";
    const NamedRange r[4] = {{src, image_bytes, "src"}, {params, (size_t)32 * (size_t)n, "params"},
                             {dst, dst_bytes, "dst"}, {valid, valid ? pixels : 0, "valid"}};
    return check_disjoint(r, 2, 4, why);
}
inline const char* check_homography_stabilize_buffers(uintptr_t pair_params, uintptr_t corrections, uintptr_t status,
                                                      uintptr_t replaced, int n_frames, PairMessage* why)
{
    const size_t n = (size_t)n_frames;
    const NamedRange r[4] = {{pair_params, pair_params ? (n - 1) * 32 : 0, "pair_params"},
                             {corrections, n * 32, "corrections"},
                             {status, status ? n : 0, "status"},
                             {replaced, replaced ? sizeof(int) : 0, "replaced"}};
    return check_disjoint(r, 1, 4, why);
}

// dis_yuv420_to_frames_u8 / dis_frames_to_yuv420_u8: n 4:2:0 surfaces of W x H
// pixels (both even): a Y plane of W x H bytes and W/2 x H/2 Cb and Cr samples,
// the sample of block (X, Y) at Y * c_stride + X * c_step (c_step 1: planar,
// 2: interleaved). Strides in bytes; 0 means W and stride * H for the Y plane,
// (W/2) * c_step and c_stride * (H/2) for the chroma planes. y_bytes / c_bytes
// end with ONE image's last sample (of the plane a chroma pointer addresses).
constexpr int kYuvStripW = 16;  // a lane converts 16 x 2 pixels
constexpr int kYuvThreads = 256;
struct Yuv420Layout {
    size_t y_stride, y_image_stride, c_stride, c_image_stride;
    size_t y_bytes, c_bytes;
};
inline const char* check_yuv420_layout(int n, int width, int height, int c_step, size_t y_stride, size_t y_image_stride,
                                       size_t c_stride, size_t c_image_stride, Yuv420Layout* out)
{
    if (const char* why = check_dims(n, width, height, kMaxExactSide)) return why;
    if ((width | height) & 1) return "width and height must be even (4:2:0)";
    if (c_step != 1 && c_step != 2) return "c_step must be 1 (planar) or 2 (interleaved)";
    ImageStack ys, cs;
    if (check_image_stack(width, height, 1, n, y_stride, y_image_stride, &ys))
        return "y_stride or y_image_stride smaller than a row / an image (or too large)";
    if (check_image_stack(width / 2, height / 2, c_step, n, c_stride, c_image_stride, &cs))
        return "c_stride or c_image_stride smaller than a row / an image (or too large)";
    *out = {ys.stride, ys.image_stride, cs.stride, cs.image_stride,
            (size_t)(height - 1) * ys.stride + (size_t)width,
            (size_t)(height / 2 - 1) * cs.stride + (size_t)(width / 2 - 1) * c_step + 1};
    return nullptr;
}

// Blocks of either launch (a lane per 16 x 2 pixels); -1 when they exceed a grid.
inline long long yuv420_blocks(int n, int width, int height)
{
    if (n < 1 || width < 2 || height < 2) return -1;
    const long long cw = ((long long)width + kYuvStripW - 1) / kYuvStripW, rows = height / 2;
    if (n > 0x7fffffffLL * kYuvThreads / cw / rows) return -1;
    return ((long long)n * rows * cw + kYuvThreads - 1) / kYuvThreads;
}

// A plane of n images: image i occupies [p + i * image_stride, ... + image_bytes),
// image_bytes <= image_stride (an absent plane has p = 0 and no bytes).
struct PlaneStack {
    uintptr_t p;
    size_t image_stride, image_bytes;
    const char* name;
};

// Two such planes share a byte. With one image stride S (the planes of an NV12
// or I420 surface lie image by image in one buffer, each in the gaps of the
// others) it is exact: with a.p <= b.p and d = b.p - a.p, image i of a meets
// image j = i - k of b iff k * S + a.bytes > d and k * S < d + b.bytes, which only
// k = d / S and k + 1 can satisfy (bytes <= S). With two image strides the
// whole extents are compared (planes so laid out are refused even where their
// images happen to miss each other).
inline bool plane_stacks_overlap(const PlaneStack& a, const PlaneStack& b, int n)
{
    if (!a.p || !b.p || !a.image_bytes || !b.image_bytes || n < 1) return false;
    if (a.p > b.p) return plane_stacks_overlap(b, a, n);
    const size_t m = (size_t)(n - 1);
    if (n == 1 || a.image_stride != b.image_stride)
        return ranges_overlap(a.p, m * a.image_stride + a.image_bytes, b.p, m * b.image_stride + b.image_bytes);
    const size_t S = a.image_stride, d = b.p - a.p, k = d / S, rem = d % S;
    if (k <= m && rem < a.image_bytes) return true;              // k: image k of a reaches into image 0 of b
    return k + 1 <= m && S - rem < b.image_bytes;                // k + 1: image 0 of b reaches into image k + 1 of a
}

// The planes of a conversion call: r[0 .. nin) are read, r[nin .. n_planes)
// written; every written plane must be disjoint from every read one and from
// every other written one. The caller passes the Cb and Cr of one interleaved
// plane (c_step 2, one byte apart) as ONE plane: yuv420_chroma_planes. The
// first offending pair, by name.
inline const char* check_plane_stacks(const PlaneStack* r, int nin, int n_planes, int n, PairMessage* why)
{
    for (int o = nin; o < n_planes; ++o)
        for (int k = 0; k < n_planes; ++k)
            if ((k < nin || k > o) && plane_stacks_overlap(r[o], r[k], n)) {
                const NamedRange pair[2] = {{1, 1, r[k].name}, {1, 1, r[o].name}};
                return check_disjoint(pair, 1, 2, why);
            }
    return nullptr;
}

// The chroma planes of a surface as 1 or 2 entries of such a list (returns how
// many): Cb and Cr one byte apart with c_step 2 are the two halves of one
// interleaved plane, which begins at the lower of the two and is one byte
// longer; otherwise each is a plane of its own (with c_step 2 it then spans
// the bytes between its samples too). Null pointers give absent planes.
inline int yuv420_chroma_planes(uintptr_t cb, uintptr_t cr, int c_step, const Yuv420Layout& l, PlaneStack* out)
{
    if (cb && cr && c_step == 2 && (cb + 1 == cr || cr + 1 == cb)) {
        out[0] = {cb < cr ? cb : cr, l.c_image_stride, l.c_bytes + 1, "cb/cr"};
        return 1;
    }
    out[0] = {cb, l.c_image_stride, cb ? l.c_bytes : 0, "cb"};
    out[1] = {cr, l.c_image_stride, cr ? l.c_bytes : 0, "cr"};
    return 2;
}

}  // namespace dis
