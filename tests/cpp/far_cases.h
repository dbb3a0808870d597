// far_cases.h -- the far cases of tests/farcases.py (just over 2^31 pixels in one
// call) against the pure argument rules and block counts of csrc/dis_args.h:
// every family's check function and block-count function accept both cases,
// with the sizes and the grid the kernels then index by. The args_*_host
// programs each run their family's part (under the host sanitizers, as the
// rest of them). Integers only: no device call, no C-ABI call, no pointer.
#pragma once

#include <cstdio>

#include "dis_args.h"

namespace far {

struct Case {
    const char* name;
    int W, H, n;
};
constexpr Case kAligned{"aligned", 256, 128, 65539};  // the 2^30 and 2^31 pixel marks are image starts
constexpr Case kRagged{"ragged", 253, 131, 64797};    // odd sides: no vector form, the marks inside images
constexpr Case kEven{"even", 250, 130, 66080};        // the ragged case of the 4:2:0 entry points (even sides)
constexpr Case kCases[2] = {kAligned, kRagged};
constexpr Case kYuvCases[2] = {kAligned, kEven};
constexpr Case kColor{"color", 16, 8, 65539};         // more fields than a launch's y extent

inline long long pixels(const Case& c) { return (long long)c.n * c.W * c.H; }
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline void check(bool ok, const Case& c, const char* what, int* failures)
{
    if (!ok) {
        std::printf("FAIL: far case %s (%d x %d x %d): %s\n", c.name, c.W, c.H, c.n, what);
        ++*failures;
    }
}

// what every far case is: more than 2^31 pixels, fewer than 2^32
inline void sizes(const Case& c, int* f)
{
    check(pixels(c) > (1ll << 31) && pixels(c) < (1ll << 32), c, "just over 2^31 pixels", f);
}

// dis_flow_warp_u8, dis_flow_interp_u8, dis_flow_consistency, dis_flow_convert, dis_frames_to_gray_u8:
// check_dims, check_image_stack (tight and padded, 1 / 3 / 4 channels) and the one-dimensional grids
inline void flat_families(int* f)
{
    for (const Case& c : kCases) {
        sizes(c, f);
        const long long lanes = (long long)c.n * c.H * ((c.W + 3) / 4);
        check(dis::check_dims(c.n, c.W, c.H) == nullptr, c, "check_dims", f);
        check(dis::check_dims(c.n, c.W, c.H, dis::kMaxExactSide) == nullptr, c, "check_dims, exact sides", f);
        check(dis::check_dims(c.n, c.W, c.H, dis::kMaxExactSide, dis::kMaxKeyPixels) == nullptr, c, "check_dims, key pixels", f);
        check(dis::flow_warp_blocks(c.n, c.W, c.H) == ceil_div(lanes, 256), c, "flow_warp_blocks", f);
        check(dis::flow_consistency_blocks(c.n, c.W, c.H) == ceil_div(lanes, 256), c, "flow_consistency_blocks", f);
        check(dis::flow_interp_blocks(c.n, c.W, c.H) == ceil_div(pixels(c), 256), c, "flow_interp_blocks", f);
        check(dis::flow_interp_blocks(c.n, c.W, c.H) < 0x7fffffffLL, c, "the splat's grid fits", f);
        check(dis::frames_to_gray_blocks(c.n, c.W, c.H) == ceil_div((long long)c.n * c.H * ((c.W + 15) / 16), 256), c,
              "frames_to_gray_blocks", f);
        check(dis::frames_to_gray_blocks(2ll * c.n, c.W, c.H) > 0, c, "frames_to_gray_blocks, two stacks", f);
        for (int C : {1, 3, 4}) {
            dis::ImageStack im{};
            const size_t row = (size_t)c.W * C;
            check(dis::check_image_stack(c.W, c.H, C, c.n, 0, 0, &im) == nullptr && im.stride == row &&
                      im.image_stride == row * c.H && im.bytes == (size_t)pixels(c) * C,
                  c, "check_image_stack, tight", f);
            const size_t stride = row + 5, image_stride = stride * c.H + 7;
            check(dis::check_image_stack(c.W, c.H, C, c.n, stride, image_stride, &im) == nullptr && im.stride == stride &&
                      im.image_stride == image_stride &&
                      im.bytes == (size_t)(c.n - 1) * image_stride + (size_t)(c.H - 1) * stride + row,
                  c, "check_image_stack, padded", f);
            check(C == 1 || im.bytes > (size_t(1) << 32), c, "a colour stack crosses 2^32 bytes", f);
        }
    }
}

// dis_flow_compose and dis_flow_advect_points
inline void compose(int* f)
{
    for (const Case& c : kCases) {
        sizes(c, f);
        const long long lanes = (long long)c.n * c.H * ((c.W + 3) / 4);
        size_t pts = 0;
        check(dis::check_dims(c.n, c.W, c.H, dis::kMaxExactSide) == nullptr, c, "check_dims", f);
        check(dis::flow_compose_blocks(c.n, c.W, c.H) == ceil_div(lanes, 256), c, "flow_compose_blocks", f);
        check(dis::check_points(c.n, 64, &pts) == nullptr && pts == (size_t)c.n * 64, c, "check_points", f);
        check(dis::flow_advect_blocks(c.n, 64) == ceil_div((long long)c.n * 64, 256), c, "flow_advect_blocks", f);
    }
}

inline void fill(int* f)
{
    for (const Case& c : kCases) {
        sizes(c, f);
        size_t bytes = 0;
        dis::FillLevels g;
        dis::fill_levels(c.W, c.H, &g);
        check(dis::check_fill_workspace(c.n, c.W, c.H, &bytes) == nullptr && bytes == 8 * (size_t)c.n * g.cells, c,
              "check_fill_workspace", f);
        check(bytes > (size_t(1) << 32), c, "the workspace crosses 2^32 bytes", f);
        check(dis::fill_tile_blocks(c.n, c.W, c.H) == (long long)c.n * ceil_div(c.W, 64) * ceil_div(c.H, 32), c,
              "fill_tile_blocks", f);
    }
}

// dis_flow_fit_motion / dis_motion_to_flow (terms 12) and the homography pair (terms 27)
inline void motion(int terms, int* f)
{
    for (const Case& c : kCases) {
        sizes(c, f);
        size_t bytes = 0;
        const long long chunks = ceil_div((long long)c.W * c.H, 16384);
        const char* why = terms == 12 ? dis::check_motion_workspace(c.n, c.W, c.H, &bytes)
                                      : dis::check_homography_workspace(c.n, c.W, c.H, &bytes);
        check(why == nullptr && bytes == (size_t)c.n * ((size_t)chunks * terms + 16) * 8, c, "the fit's workspace", f);
        check(dis::motion_chunks(c.W, c.H) == chunks && dis::motion_blocks(c.n, c.W, c.H) == chunks * c.n, c, "motion_blocks", f);
        check(dis::check_motion_flow(c.n, c.W, c.H) == nullptr, c, "check_motion_flow", f);
        check(dis::motion_flow_blocks(c.n, c.W, c.H) == ceil_div((long long)c.n * c.H * ((c.W + 3) / 4), 256), c,
              "motion_flow_blocks", f);
    }
}

inline void denoise(int* f)
{
    for (const Case& c : kCases) {
        sizes(c, f);
        for (int C : {1, 3, 4})
            check(dis::check_denoise_sizes(1, c.n, c.W, c.H, C) == nullptr, c, "check_denoise_sizes", f);
        check(dis::denoise_blocks(c.n, c.W, c.H) == (long long)c.n * ceil_div(c.W, 64) * ceil_div(c.H, 16), c, "denoise_blocks", f);
    }
}

// dis_warp_motion_u8 and dis_warp_homography_u8
inline void warp_model(int* f)
{
    for (const Case& c : kCases) {
        sizes(c, f);
        for (int C : {1, 3, 4})
            check(dis::check_warp_motion_sizes(c.n, c.W, c.H, C) == nullptr, c, "check_warp_motion_sizes", f);
        check(dis::warp_motion_blocks(c.n, c.W, c.H) == (long long)c.n * ceil_div(c.W, 64) * ceil_div(c.H, 16), c,
              "warp_motion_blocks", f);
    }
}

// dis_yuv420_to_frames_u8 / dis_frames_to_yuv420_u8: the ragged case itself is refused (odd sides)
inline void yuv(int* f)
{
    dis::Yuv420Layout l{};
    check(dis::check_yuv420_layout(kRagged.n, kRagged.W, kRagged.H, 1, 0, 0, 0, 0, &l) != nullptr, kRagged,
          "odd sides are refused", f);
    for (const Case& c : kYuvCases) {
        sizes(c, f);
        for (int step : {1, 2}) {
            check(dis::check_yuv420_layout(c.n, c.W, c.H, step, 0, 0, 0, 0, &l) == nullptr && l.y_stride == (size_t)c.W &&
                      l.y_image_stride == (size_t)c.W * c.H && l.c_stride == (size_t)(c.W / 2) * step &&
                      l.c_image_stride == (size_t)(c.W / 2) * step * (c.H / 2),
                  c, "check_yuv420_layout", f);
        }
        check(dis::yuv420_blocks(c.n, c.W, c.H) == ceil_div((long long)c.n * (c.H / 2) * ceil_div(c.W, 16), 256), c,
              "yuv420_blocks", f);
    }
}

// dis_flow_color: check_dims is all it checks (the launcher slices the fields, so the many-fields case and
// both far cases are accepted as they stand)
inline void color(int* f)
{
    check(dis::check_dims(kColor.n, kColor.W, kColor.H) == nullptr && kColor.n > 65536, kColor, "check_dims", f);
    for (const Case& c : kCases) {
        sizes(c, f);
        check(dis::check_dims(c.n, c.W, c.H) == nullptr, c, "check_dims of dis_flow_color", f);
    }
}

}  // namespace far
