// dis_kernels.h -- kernel argument blocks and host launchers.
#pragma once

#include <hip/hip_ext.h>

#include "dis_args.h"  // the launches' block counts (flow_warp_blocks, ...)
#include "dis_common.h"

namespace dis {

// Optional per-launch timing: events attached to the dispatch packet itself
// (hipExtLaunchKernelGGL), so timing adds no extra queue packets.
struct Timing {
    hipEvent_t start = nullptr;
    hipEvent_t stop = nullptr;
};

#define DIS_LAUNCH(T, kernel, grid, block, shmem, stream, ...)                                               \
    do {                                                                                                    \
        if ((T).start)                                                                                      \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, (T).start, (T).stop, 0, __VA_ARGS__); \
        else                                                                                                \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                            \
    } while (0)

// One patch-search launch: one level, a batch of pairs.
struct SearchArgs {
    const float* img0;         // frame-0 level planes (stack), for fused gradients
    const float* img1;         // frame-1 level planes (stack)
    const float* dx;           // frame-0 Sobel dx planes (stack)
    const float* dy;           // frame-0 Sobel dy planes (stack)
    const float2* dense_coarse;  // dense flow of level l+1 (nullptr at the coarsest level)
    float2* u_out;             // patch displacements of level l
    long long plane_stride;    // floats per pair
    long long plane_off;       // this level's offset in the plane stack
    long long dense_stride;    // float2 per pair (dense stack), dense_coarse pre-offset
    int coarse_ld;             // row stride of dense_coarse in float2: W / 2 (level l+1's width), or the
                               //   init plane's iw at a warm-started coarsest level (W_C may be odd)
    long long u_stride;        // float2 per pair (patch stack), u_out pre-offset
    int phys_pad;              // 0: virtual padding (clamp image / zero gradients);
                               // >0: planes are physically padded by this many pixels
                               //     (compat path), plane_off points at the padded origin
    int W, H, steps, npw, nph, offw, offh, n;
    float tmp_lb, tmp_ub_w, tmp_ub_h, outlier;
    int iters, norm;
    int paper;                 // template-subtracted residual (dis_params.paper_mode)
};

// Fast patch-size-8 search (dis_search8.hip): gradients fused from the level
// image, init fused from the coarser level's patch displacements.
struct Search8Args {
    const float* img0;        // frame-0 level planes (stack)
    const float* img1;        // frame-1 level planes (stack)
    const float2* u_coarse;   // level l+1 patch u (pre-offset), nullptr at the coarsest level
    float2* u_out;            // level l patch u (pre-offset)
    long long plane_stride, plane_off, u_stride;
    int W, H, steps, npw, nph, offw, offh;
    int c_npw, c_nph, c_offw, c_offh;  // coarser level grid
    float tmp_lb, tmp_ub_w, tmp_ub_h;
    float thr_sq;             // largest float s with sqrtf(s) <= outlierthresh
    int iters, norm;
    int tile_stride;          // LDS tile row stride (search8_tile_stride(steps))
    int quad;                 // LPP 2 patch layout: 0 = 2 x 8, 1 = 4 x 4 patches per half-wave (search8_tile_quad)
    int lanes_per_patch;      // 1, 2, 4 or 8 (k_search8<LPP>)
    const float2* dense_coarse;  // non-null: init from the coarser level's DENSE flow (variational
    long long dense_stride;      //   refinement on) instead of u_coarse; float2 per pair
    int coarse_ld;               // row stride of dense_coarse in float2: W / 2, or the init plane's iw at a
                                 //   warm-started coarsest level (wave-uniform, read once per patch)
    int tile_cap;             // > 0: usable tile rows / columns capped at this (variant 9, a parity-test
                              //   switch that sends most blocks through the fallback list); 0 = the full tile
    int* fb_count;            // LPP 1/2: blocks too spread for the LDS tile are listed here
    int* fb_list;             //   (count zeroed before the launch) and redone by k_search8_fb;
                              //   nullptr: one kernel with the global-read path inline
    int paper;                // template-subtracted residual (k_search8<.., kPaper>) and
                              //   the residual-weighted coarse-to-fine initialisation, which reads the
    long long c_plane_off;    //   coarser level's planes (offset in the stack) of size c_W x c_H
    int c_W, c_H;
    int fma;                  // DIS_PRECISION_FMA: contracted warp / dot products, reciprocal solve
    // compat path (dis_flow_from_pyramids): non-null = the caller's physically
    // padded planes (pad pixels on every side, row stride W + 2 pad; plane_off
    // = the padded plane's start): template gradients from gdx/gdy_plane, I1
    // taps from the padded img1 plane
    const float* gdx_plane;
    const float* gdy_plane;
    int pad;
};

struct DensifyArgs {
    const float2* u;       // patch u of the level (pre-offset)
    float2* dense;         // dense flow of the level (pre-offset)
    long long u_stride, dense_stride;
    int W, H, ps, steps, npw, nph, offw, offh;
    // paper mode: votes weighted by 1/max(1, |I1(x+u) - I0(x)|)
    const float* img0;     // level planes of pair 0 (pre-offset), pair stride plane_stride
    const float* img1;
    long long plane_stride;
    int paper;
};

struct UpsampleArgs {
    const float2* dense;   // finest-level dense flow (pre-offset)
    float2* flow;          // W x H output, pair stride W*H
    long long dense_stride;
    int W, H, wF, hF, F, pad_left, pad_top, xmax;
    float sc;
    double inv_sc;
};

// The pyramid (dis_pyramid.hip): u8 -> levels 1..`levels` (and 0 if write_l0).
struct PyramidArgs {
    const uint8_t* I0;
    const uint8_t* I1;
    size_t stride, pair_stride;
    int W, H, Wp, Hp, pl, pt;
    float* img0;
    float* img1;
    long long plane_stride;
    int levels;    // levels produced by the pyramid kernels, 1..6 (min(C, 6))
    int write_l0;  // also store the level-0 magnitude plane
    long long off[kMaxLevels];  // plane offset per level
    int w[kMaxLevels];          // plane width per level
    int* zero;                  // nzero ints set to 0 by workgroup 0 (the searches' fallback counts)
    int nzero;
    // the next two 8-byte aligned: k_pyr12 reads them with one scalar load, and
    // its register allocation, hence its whole instruction stream, follows
    // from how the loads of nzero and of these two group
    alignas(8) int qword_ok;    // I0/I1, stride, pair_stride and pad_left multiples of 16: 16-byte row loads
    int vec_st;                 // k_pyr12: level-1 / level-2 rows 16-byte aligned (W_2 % 4 == 0; set by launch_pyramid2)
};

// Fused densify + upsample + crop (dis_output.hip).
struct OutputArgs {
    const float2* u;   // finest-level patch u (pre-offset)
    float2* flow;      // W x H x 2 output, pair stride W*H
    long long u_stride;
    int W, H, wF, hF, F, pad_left, pad_top, xmax;
    int npw, nph, offw, offh, steps, hp;
    int vec_store;     // W even and the output base 16-byte aligned (f16 output: 8-byte aligned)
    float sc;
    // paper mode: votes weighted by 1/max(1, |I1(x+u) - I0(x)|) on level F
    int paper;
    const float* img0;  // level-F planes of pair 0 (pre-offset), pair stride plane_stride
    const float* img1;
    long long plane_stride;
};

// a.levels >= 2 (C >= 2): k_pyr12, levels 1-2 from global memory, then
// k_pyr_tail_reg, levels 3..a.levels; a.levels == 1 (C == 1): k_pyr1. Either
// returns hipErrorInvalidValue for the other's arguments.
hipError_t launch_pyramid2(const PyramidArgs& a, int batch, hipStream_t s, Timing t = {});
hipError_t launch_pyramid1(const PyramidArgs& a, int batch, hipStream_t s, Timing t = {});
bool output_fits(const OutputArgs& a);
// f16 != 0 (here and in launch_upsample): a.flow points at __half2 vectors
// (DIS_FLOW_F16), written by the kernels' __half2 instantiations
hipError_t launch_output(const OutputArgs& a, int batch, hipStream_t s, Timing t = {}, int f16 = 0);
hipError_t launch_level0(const uint8_t* I0, const uint8_t* I1, size_t stride, size_t pair_stride,
                         const Geometry& g, float* img0, float* img1, int batch, hipStream_t s);
hipError_t launch_down2(const Geometry& g, int l, float* img0, float* img1, int batch, hipStream_t s);
hipError_t launch_sobel(const Geometry& g, int l, const float* img0, float* dx, float* dy, int batch,
                        hipStream_t s);
hipError_t launch_search_generic(const SearchArgs& a, int ps, int batch, hipStream_t s, Timing t = {});
int search8_tile_stride(int steps, int lanes_per_patch);
int search8_tile_quad(int steps, int lanes_per_patch);  // LPP 2: 4 x 4-patch half-waves (Search8Args.quad)
bool search8_lpp1_fits(int steps);
hipError_t launch_search8(const Search8Args& a, int batch, hipStream_t s, Timing t = {});
// one wave64 per patch (dis_search_wave.hip; lanes_per_patch 64, variant 6)
hipError_t launch_search_wave(const Search8Args& a, int batch, hipStream_t s, Timing t = {});
hipError_t launch_densify(const DensifyArgs& a, int batch, hipStream_t s);
hipError_t launch_upsample(const UpsampleArgs& a, int batch, hipStream_t s, int f16 = 0);

// Middlebury colour coding of n W x H (u,v) fields into BGR u8 (dis_color.hip);
// maxbits: 32 * n device uints of scratch.
hipError_t launch_flow_color(const float* flow, int n, int W, int H, float maxmotion, uint8_t* bgr,
                             unsigned int* maxbits, hipStream_t s);
// device workspace words launch_flow_color needs for n fields (zeroed by it)
size_t flow_color_ws_words(int n);

// Forward-backward consistency of n W x H (u,v) fields (dis_consistency.hip):
// mask (u8, 255 = consistent) and, if err is non-null, the squared round-trip
// distance per pixel. fw and bw 8-byte aligned.
hipError_t launch_flow_consistency(const float* fw, const float* bw, int n, int W, int H, float alpha1,
                                   float alpha2, uint8_t* mask, float* err, hipStream_t s, Timing t = {});

// Backward warp of n W x H u8 images of `channels` (1, 3, 4) interleaved
// samples by n (u,v) fields (dis_warp.hip): dst(x, y) = src sampled bilinearly
// at (x + scale * u, y + scale * v); valid (u8, 255 = target inside the frame)
// may be null. f16 != 0: `flow` holds __half2 vectors (4-byte aligned), else
// float2 (8-byte aligned). Strides in bytes, already resolved (never 0).
hipError_t launch_flow_warp(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                            const void* flow, int f16, int n, int W, int H, float scale, int zero_border,
                            uint8_t* dst, uint8_t* valid, hipStream_t s, Timing t = {});

// The frame at time t in [0, 1] between n pairs of W x H u8 images (dis_interp.hip,
// dis_flow_interp_u8): one memset of `workspace` (n * W * H 64-bit keys, 8-byte
// aligned) to 0xFF, k_interp_splat (the forward flow projected to time t by
// atomicMin on the keys) and k_interp_blend (both frames sampled with the
// winning vectors; holes from bw, which may be null, or fw). I0 and I1 share
// the strides (bytes, already resolved); fw and bw as launch_flow_warp's flow;
// fill (u8, 0 / 1 / 2) may be null. flow_interp_blocks(n, W, H) >= 1: the
// splat's grid (a lane per pixel), -1 when W * H > 2^31 or the grid limit is
// exceeded.
hipError_t launch_flow_interp(const uint8_t* I0, const uint8_t* I1, size_t stride, size_t image_stride, int channels,
                              const void* fw, const void* bw, int f16, int n, int W, int H, float t, uint8_t* dst,
                              uint8_t* fill, void* workspace, hipStream_t s, Timing t_splat = {}, Timing t_blend = {});

// Composition of n W x H (u,v) fields (dis_compose.hip, dis_flow_compose):
// out(x) = a(x) + b sampled bilinearly at x + a(x), the canonical NaN and
// valid_out 0 where a's vector, its valid_a byte, the target or one of the four
// taps of b / mask_b is not to be trusted. *_f16 != 0: that field holds __half2
// vectors (4-byte aligned), else float2 (8-byte aligned). valid_a, mask_b and
// valid_out may be null; out may be a (equal formats) and valid_out valid_a.
hipError_t launch_flow_compose(const void* a, int a_f16, const void* b, int b_f16, int n, int W, int H,
                               const uint8_t* valid_a, const uint8_t* mask_b, void* out, int out_f16,
                               uint8_t* valid_out, hipStream_t s, Timing t = {});
// n fields, `count` (x, y) float pairs each, moved by the field sampled at them
// (dis_flow_advect_points); points 8-byte aligned, status (u8) may be null,
// points_out may be points.
hipError_t launch_flow_advect(const void* flow, int f16, int n, int W, int H, const float* points, int count,
                              float* points_out, uint8_t* status, hipStream_t s, Timing t = {});

// Push-pull fill of the untrusted vectors of n W x H (u,v) fields (dis_fill.hip,
// dis_flow_fill): k_fill_pull over levels 0..5, k_fill_top from there to 1 x 1
// and back, k_fill_push down to `out` and `level` -- three launches, unless
// level 5 and above exceed the top block's LDS (6,208 cells):
// then a further pull and push pass over five more levels each. f16 / out_f16
// != 0: that field holds __half2 vectors (4-byte aligned), else float2 (8-byte
// aligned). mask and level may be null; out may be flow (equal formats).
// workspace: 8 bytes per cell of levels 1..L of every field (dis_args.h,
// fill_levels), 8-byte aligned; null for 1 x 1 fields. fill_tile_blocks(n, W, H)
// (dis_args.h) >= 1.
hipError_t launch_flow_fill(const void* flow, int f16, const uint8_t* mask, int n, int W, int H, void* out, int out_f16,
                            uint8_t* level, void* workspace, hipStream_t s);

// Global motion of n W x H (u,v) fields (dis_motion.hip, dis_flow_fit_motion):
// per pass k_motion_accum (a block per chunk of 16384 pixels and field) and
// k_motion_solve (a block per field), iterations + 1 passes, then
// k_motion_inliers when `inliers` is given. f16 != 0: the fields hold __half2
// vectors (4-byte aligned), else float2 (8-byte aligned). mask, info and
// inliers may be null. workspace: check_motion_workspace's bytes (dis_args.h),
// 8-byte aligned. model: a dis_motion_model; motion_blocks(n, W, H) >= 1.
hipError_t launch_fit_motion(const void* flow, int f16, const uint8_t* mask, int n, int W, int H, int model, int iterations,
                             float threshold, float* params, unsigned* info, uint8_t* inliers, void* workspace,
                             hipStream_t s);
// The fields of n models of six parameters (dis_motion_to_flow): float2 or
// (out_f16 != 0) __half2 vectors; motion_flow_blocks(n, W, H) >= 1.
hipError_t launch_motion_flow(const float* params, int n, int W, int H, void* out, int out_f16, hipStream_t s);

// Backward warp of n W x H u8 images of `channels` (1, 3, 4) interleaved samples
// by n motion models of six device floats each (dis_warpmotion.hip,
// dis_warp_motion_u8): launch_motion_flow's vectors computed in registers, then
// launch_flow_warp's pixel at scale 1; one launch, a block per 64 x 16 pixels;
// with 3 channels the taps come from an LDS image of the tile's source box
// where it fits. valid may be null. Strides in bytes, already resolved (never
// 0). warp_motion_blocks(n, W, H) (dis_args.h) >= 1. direct_only != 0: the
// kernel without the LDS route (the same bytes; for A/B timing). routes
// (null in the library's own calls): three device counters the launch adds to --
// blocks that staged their box, blocks that ran the direct form, pixels of
// staged blocks that read global memory -- for tools/stabilize_ab's route mode.
hipError_t launch_warp_motion(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                              const float* params, int n, int W, int H, int zero_border, uint8_t* dst, uint8_t* valid,
                              hipStream_t s, Timing t = {}, int direct_only = 0, unsigned* routes = nullptr);

// The eight-parameter family (dis_homography.hip): launch_fit_motion's passes
// with 27 sums and an 8 x 8 solve (dis_flow_fit_homography; workspace:
// check_homography_workspace's bytes), the fields of n models of eight
// parameters (dis_homography_to_flow), and launch_warp_motion's direct form with
// the projective vector (dis_warp_homography_u8). Pointers, strides and limits
// as for their affine siblings above.
hipError_t launch_fit_homography(const void* flow, int f16, const uint8_t* mask, int n, int W, int H, int iterations,
                                 float threshold, float* params, unsigned* info, uint8_t* inliers, void* workspace,
                                 hipStream_t s);
hipError_t launch_homography_flow(const float* params, int n, int W, int H, void* out, int out_f16, hipStream_t s);
hipError_t launch_warp_homography(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                                  const float* params, int n, int W, int H, int zero_border, uint8_t* dst,
                                  uint8_t* valid, hipStream_t s);

// Motion-compensated temporal denoising of n W x H u8 images of `channels`
// (1, 3, 4) interleaved samples (dis_denoise.hip, dis_temporal_denoise_u8): one
// launch, a block per 64 x 16 pixels. `neighbours`, `flows` and `masks` are host
// arrays of k_neighbours (1..8) device pointers, copied into the kernel's
// arguments with the 256 host `weights`; masks or any of its entries and
// support may be null. f16 != 0: the flows hold __half2 vectors (4-byte
// aligned), else float2 (8-byte aligned). Strides in bytes, already resolved
// (never 0). denoise_blocks(n, W, H) (dis_args.h) >= 1.
hipError_t launch_temporal_denoise(const uint8_t* cur, const uint8_t* const* neighbours, size_t stride,
                                   size_t image_stride, int channels, const void* const* flows, int f16,
                                   const uint8_t* const* masks, int k_neighbours, int n, int W, int H,
                                   const float* weights, uint8_t* dst, uint8_t* support, hipStream_t s, Timing t = {});

// The init plane of a warm-started call (dis_init.hip): iw x ih = ceil(W_C / 2) x
// ceil(H_C / 2) float2 per pair. launch_flow_to_init reduces n full-resolution
// W x H flows to n planes (pad / clamp extension, C + 1 halvings, sanitising) in
// one launch; launch_init_copy is the sanitising copy of `count` floats of
// caller-made planes.
// f16 != 0: `flow` holds __half2 vectors (DIS_FLOW_F16), widened on load.
void init_plane_size(const Geometry& g, int* iw, int* ih);
hipError_t launch_flow_to_init(const float* flow, float* planes, int n, const Geometry& g, hipStream_t s,
                               Timing t = {}, int f16 = 0);
hipError_t launch_init_copy(const float* src, float* dst, long long count, hipStream_t s, Timing t = {});

// dis_flow_convert's kernel (dis_convert.hip): `count` values from src_format
// to the other format (DIS_FLOW_F32 / DIS_FLOW_F16; the formats differ).
hipError_t launch_flow_convert(const void* src, int src_format, void* dst, size_t count, hipStream_t s);

// Interleaved u8 colour frames to u8 gray (dis_luma.hip): up to two stacks of
// n W x H images of `format` (dis_frame_format; DIS_FRAME_GRAY8 copies) from
// src0 / src1 (null: one stack) into dst0 / dst1, one launch. Both sources share
// the strides, both destinations theirs (bytes, already resolved, never 0). No
// pointer needs any alignment. frame_format_channels: bytes per pixel, 0 for an
// unknown format. frames_to_gray_blocks: the launch's grid for `images` images,
// -1 when it exceeds the grid limit.
int frame_format_channels(int format);
hipError_t launch_frames_to_gray(const uint8_t* src0, const uint8_t* src1, size_t src_stride, size_t src_image_stride,
                                 int format, int n, int W, int H, uint8_t* dst0, uint8_t* dst1, size_t dst_stride,
                                 size_t dst_image_stride, hipStream_t s, Timing t = {});

// Variational refinement of one level's dense flow (dis_varref.hip).
constexpr int kVarRefPlanes = 8;   // per-pair workspace planes
constexpr int kVarRefSor = 5;      // red-black SOR sweeps per fixed-point iteration
struct VarRefArgs {
    const float* img0;      // level planes of pair 0 (pre-offset), pair stride plane_stride
    const float* img1;
    long long plane_stride;
    float2* flow;           // dense flow of pair 0 (pre-offset), refined in place
    long long flow_stride;  // float2 per pair
    float* ws;              // workspace of pair 0, pair stride ws_stride floats
    long long ws_plane, ws_stride;
    int W, H, iters;
};
// tfn (optional, kernel timing): events for each k_vr_lin (kind 0) and
// k_vr_sor (kind 1) launch
typedef Timing (*VarRefTiming)(void* ctx, int kind);
hipError_t launch_var_refine(const VarRefArgs& a, int n, hipStream_t s, VarRefTiming tfn = nullptr,
                             void* tctx = nullptr);

}  // namespace dis
