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

}  // namespace dis
