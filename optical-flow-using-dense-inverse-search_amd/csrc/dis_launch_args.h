// dis_launch_args.h -- the host arithmetic in front of the launches: geometry
// (make_geometry, dis_common.h), the constants every launch of a geometry
// shares, and one builder per kernel argument block (dis_kernels.h). Each
// builder is the only place that assigns its block's fields from the geometry
// and the planes; what depends on the call (warm start, refinement, precision,
// debug, the fallback lists) the caller sets on the returned block. No HIP
// runtime call: tests/cpp/launch_args_host.cpp runs all of it on the CPU.
#pragma once

#include "dis_kernels.h"

namespace dis {

// Largest float s with sqrtf(s) <= thr (sqrtf is correctly rounded and
// monotone, so `sqrtf(s) > thr` <=> `s > thr_sq`; src/patch.cpp:185).
float sqrt_threshold(float thr);

// cv::resize HResizeLinear: first destination column whose source index
// reaches wF-1; columns from there on take S[wF-1] alone (src/main.cpp:195).
int upsample_xmax(const Geometry& g);

// What every launch of one geometry shares; made once (dis_create, or once per
// compat call).
struct LaunchConsts {
    float outlier;  // src/patch.cpp:185: ps / 2
    float thr_sq;   // sqrt_threshold(outlier)
    int paper;      // dis_params.paper_mode
    int xmax;       // upsample_xmax
    float sc;       // 2^F, the finest level's flow scale
};
LaunchConsts launch_consts(const Geometry& g, int paper_mode);
// the searches' and densify's part alone (the compat path ends at the finest
// level's dense flow: no upsampling, and upsample_xmax walks a whole row)
LaunchConsts search_consts(const Geometry& g, int paper_mode);

// level patches x pairs up to which 8 lanes per patch is used (A/B: 65536
// -2.6 %); above it 2 lanes per patch (LPP 1 / 4 measured slower)
constexpr long long kLpp8MaxPatches = 16384;

// Lanes per patch for the patch_size-8 search at one level. Few patches leave
// the chip idle and the level is bound by one wave's serial iteration chain:
// spend more lanes per patch (shorter chain). Many patches make it VALU-bound:
// 2 lanes per patch does the least total work. (Variant 5 asks for 1 lane;
// set_search8_lanes falls back to 2 where one lane's tile does not fit.)
int search8_lanes(int variant, long long patches);

// Search8Args.lanes_per_patch, tile_stride and quad together, from the tile
// layout rules of dis_search8.hip (defined in dis_enqueue.hip).
void set_search8_lanes(Search8Args* b, int lanes);

// entries of one pair's fallback list of a level (k_search8_fb): its 8x8-patch
// blocks, the most a search can list
size_t fb_list_blocks(const LevelGeom& L);

// u8 frame rows loadable `bytes` (16: PyramidArgs.qword_ok) at a
// time: both bases, the strides and pad_left are multiples of it (one pair:
// pair_stride is never applied)
bool frame_rows_aligned(const void* I0, const void* I1, size_t stride, size_t pair_stride, int n, int pad_left,
                        int bytes);
// OutputArgs.vec_store, two pixels per store: 16 bytes of floats, 8 bytes of halves
bool flow_vec_store(const void* flow, int W, bool f16);

// Where one sub-batch's planes live: pointers at its first pair, per-pair
// strides, and each level's offset in the plane stacks. (The patch arrays'
// and dense flows' level offsets are the geometry's in both forms.)
struct Planes {
    float* img0;  // null in the compat form: the caller supplies gradients, not frame 0
    float* img1;
    float* dx;
    float* dy;
    float2* pu;
    float2* dense;
    long long plane_stride, u_stride, dense_stride;
    long long plane_off[kMaxLevels];
    int pad;  // 0: virtual padding; > 0: planes physically padded by this many pixels on every side
};
// pairs p0.. of a context's workspace (virtual padding: offsets and strides of g)
Planes context_planes(const Geometry& g, int p0, float* img0, float* img1, float* dx, float* dy, float2* pu,
                      float2* dense);
// one pair of caller-padded planes stacked level after level (compat path)
Planes compat_planes(const Geometry& g, int pad, float* img1, float* dx, float* dy, float2* pu, float2* dense);

// Left to the caller: zero / nzero, and write_l0 under debug dumps.
PyramidArgs pyramid_args(const Geometry& g, const Planes& P, const uint8_t* I0, const uint8_t* I1, size_t stride,
                         size_t pair_stride, int n);
// Left to the caller: the warm-started coarsest level's dense_coarse.
SearchArgs search_args(const Geometry& g, int l, const Planes& P, const LaunchConsts& k);
// Left to the caller: the lane layout (set_search8_lanes), the fallback list,
// tile_cap, fma, and the coarse planes / dense init of paper mode, refinement
// and warm start.
Search8Args search8_args(const Geometry& g, int l, const Planes& P, const LaunchConsts& k);
DensifyArgs densify_args(const Geometry& g, int l, const Planes& P, const LaunchConsts& k);
// Left to the caller: the workspace (ws, ws_plane, ws_stride) and iters.
VarRefArgs varref_args(const Geometry& g, int l, const Planes& P);
OutputArgs output_args(const Geometry& g, const Planes& P, const LaunchConsts& k, float2* flow, bool f16);
UpsampleArgs upsample_args(const Geometry& g, const Planes& P, const LaunchConsts& k, float2* flow);

}  // namespace dis
