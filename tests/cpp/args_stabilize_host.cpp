// args_stabilize_host.cpp -- dis_motion_stabilize (csrc/dis_stabilize.cpp) and
// the argument rules of it and of dis_warp_motion_u8 (csrc/dis_args.h) at their
// edges: the value rules (check_stabilize), the overlap rules over the four
// ranges of each entry point, the grid of the warp (warp_motion_blocks), and
// the path math on exact cases, the longest window, one frame, null optional
// outputs and models that are not finite or collapse the path. Built with
// -fsanitize=address,undefined by tests/cpp/stabilize.mk (target
// args_stabilize) and run by tests/test_stabilize_host.py. The buffers handed
// to the entry are exactly as large as the contract says, so a write past an
// end aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dis_abi.h"
#include "dis_args.h"
#include "far_cases.h"

namespace dis {
static std::string g_error;
dis_status set_error(dis_status s, const std::string& msg)  // (the library's lives in dis_runtime.hip)
{
    g_error = msg;
    return s;
}
}  // namespace dis

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++failures;
    }
}

static bool all_zero_bits(const float* v, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        uint32_t w;
        std::memcpy(&w, v + i, 4);
        if (w) return false;
    }
    return true;
}

static dis::PairMessage g_why;

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {  // the value rules
        expect(dis::check_stabilize(1, 1, 1, 0, 1.0f, 1.0f) == nullptr, "the smallest call");
        expect(dis::check_stabilize(INT32_MAX, dis::kMaxExactSide, dis::kMaxExactSide, 1024, 3.0e38f, 16.0f) == nullptr,
               "the largest values");
        expect(dis::check_stabilize(0, 4, 4, 1, 1.0f, 1.0f) && dis::check_stabilize(-1, 4, 4, 1, 1.0f, 1.0f), "n_frames < 1");
        expect(dis::check_stabilize(2, 0, 4, 1, 1.0f, 1.0f) && dis::check_stabilize(2, 4, 0, 1, 1.0f, 1.0f) &&
                   dis::check_stabilize(2, -4, 4, 1, 1.0f, 1.0f), "sides below 1");
        expect(dis::check_stabilize(2, dis::kMaxExactSide + 1, 4, 1, 1.0f, 1.0f) &&
                   dis::check_stabilize(2, 4, dis::kMaxExactSide + 1, 1, 1.0f, 1.0f), "sides above 2^24");
        expect(dis::check_stabilize(2, 4, 4, -1, 1.0f, 1.0f) && dis::check_stabilize(2, 4, 4, 1025, 1.0f, 1.0f) &&
                   dis::check_stabilize(2, 4, 4, INT32_MIN, 1.0f, 1.0f), "radius outside 0..1024");
        expect(dis::check_stabilize(2, 4, 4, 1, 0.0f, 1.0f) && dis::check_stabilize(2, 4, 4, 1, -0.0f, 1.0f) &&
                   dis::check_stabilize(2, 4, 4, 1, -1.0f, 1.0f) && dis::check_stabilize(2, 4, 4, 1, nan, 1.0f) &&
                   dis::check_stabilize(2, 4, 4, 1, inf, 1.0f) && dis::check_stabilize(2, 4, 4, 1, -inf, 1.0f),
               "sigma not finite or not > 0");
        expect(dis::check_stabilize(2, 4, 4, 1, 1e-45f, 1.0f) == nullptr, "the smallest sigma");
        expect(dis::check_stabilize(2, 4, 4, 1, 1.0f, 0.99999994f) && dis::check_stabilize(2, 4, 4, 1, 1.0f, 16.000002f) &&
                   dis::check_stabilize(2, 4, 4, 1, 1.0f, nan) && dis::check_stabilize(2, 4, 4, 1, 1.0f, inf) &&
                   dis::check_stabilize(2, 4, 4, 1, 1.0f, -4.0f), "zoom outside [1, 16]");
    }
    {  // the overlap rule of dis_motion_stabilize: pair | corrections, status, replaced (4 frames)
        auto rule = [](uintptr_t pair, uintptr_t out, uintptr_t st, uintptr_t rep, int n) {
            return dis::check_stabilize_buffers(pair, out, st, rep, n, &g_why);
        };
        expect(rule(0x1000, 0x2000, 0x3000, 0x4000, 4) == nullptr, "all apart");
        expect(rule(0x1000, 0x1000 + 72, 0, 0, 4) == nullptr, "corrections right after pair_params");
        expect(rule(0x1000, 0x1000 + 71, 0, 0, 4) && std::strstr(g_why.text, "corrections") && std::strstr(g_why.text, "pair_params"),
               "corrections on pair_params' last byte");
        expect(rule(0x1000, 0x1000 - 95, 0, 0, 4) != nullptr, "corrections end in pair_params");
        expect(rule(0x1000, 0x1000 - 96, 0, 0, 4) == nullptr, "corrections right before pair_params");
        expect(rule(0x1000, 0x2000, 0x2000 + 95, 0, 4) && std::strstr(g_why.text, "status"), "status on corrections' last byte");
        expect(rule(0x1000, 0x2000, 0x2000 + 96, 0, 4) == nullptr, "status right after corrections");
        expect(rule(0x1000, 0x2000, 0x1000 + 71, 0, 4) != nullptr, "status in pair_params");
        expect(rule(0x1000, 0x2000, 0x3000, 0x3000 + 3, 4) && std::strstr(g_why.text, "replaced"), "replaced on status' last byte");
        expect(rule(0x1000, 0x2000, 0x3000, 0x3000 + 4, 4) == nullptr, "replaced right after status");
        expect(rule(0x1000, 0x2000, 0x3000, 0x1000 - 3, 4) != nullptr, "replaced ends in pair_params");
        expect(rule(0x1000, 0x2000, 0x3000, 0x2000 + 92, 4) != nullptr, "replaced in corrections");
        expect(rule(0, 0x2000, 0x3000, 0x4000, 1) == nullptr, "one frame: no pair_params");
        expect(rule(0x2000, 0x2000, 0, 0, 1) == nullptr, "one frame: pair_params holds nothing");
        expect(rule(UINTPTR_MAX - 71, UINTPTR_MAX - 95, 0, 0, 4) != nullptr, "no wrap at the top of the address space");
    }
    {  // the grid and the buffers of dis_warp_motion_u8
        expect(dis::warp_motion_blocks(1, 1, 1) == 1 && dis::warp_motion_blocks(1, 64, 16) == 1, "one tile");
        expect(dis::warp_motion_blocks(2, 65, 17) == 8 && dis::warp_motion_blocks(3, 67, 33) == 18, "a tile plus one");
        expect(dis::warp_motion_blocks(64, 1920, 1080) == 64 * 30 * 68, "64 images of 1080p");
        expect(dis::warp_motion_blocks(INT32_MAX, 64, 16) == INT32_MAX && dis::warp_motion_blocks(INT32_MAX, 65, 16) == -1,
               "the grid limit");
        expect(dis::warp_motion_blocks(1, dis::kMaxExactSide, dis::kMaxExactSide) == -1 &&
                   dis::warp_motion_blocks(INT32_MAX, dis::kMaxExactSide, dis::kMaxExactSide) == -1, "no overflow on the way");
        expect(dis::warp_motion_blocks(0, 4, 4) == -1 && dis::warp_motion_blocks(-1, 4, 4) == -1, "no images");
        expect(dis::check_warp_motion_sizes(1, 4, 4, 1) == nullptr && dis::check_warp_motion_sizes(1, 4, 4, 3) == nullptr &&
                   dis::check_warp_motion_sizes(1, 4, 4, 4) == nullptr, "the channels");
        expect(dis::check_warp_motion_sizes(1, 4, 4, 2) && dis::check_warp_motion_sizes(1, 4, 4, 0) &&
                   dis::check_warp_motion_sizes(1, 4, 4, 5), "other channels");
        expect(dis::check_warp_motion_sizes(0, 4, 4, 1) && dis::check_warp_motion_sizes(1, 0, 4, 1) &&
                   dis::check_warp_motion_sizes(1, dis::kMaxExactSide + 1, 1, 1) &&
                   dis::check_warp_motion_sizes(INT32_MAX, 65, 16, 1), "sizes and the grid");
        // two images of 10 pixels of 3 channels: 60 bytes of src and dst, 48 of params, 20 of valid
        auto rule = [](uintptr_t src, uintptr_t par, uintptr_t dst, uintptr_t valid, size_t align) {
            return dis::check_warp_motion_buffers(src, 60, par, 2, dst, 60, valid, 20, align, &g_why);
        };
        expect(rule(0x1000, 0x2000, 0x3000, 0x4000, 4) == nullptr, "all apart");
        expect(rule(0x1000, 0x2000, 0x1000 + 60, 0, 0) == nullptr, "dst right after src");
        expect(rule(0x1000, 0x2000, 0x1000 + 59, 0, 0) && std::strstr(g_why.text, "dst") && std::strstr(g_why.text, "src"),
               "dst on src's last byte");
        expect(rule(0x1000, 0x2000, 0x2000 + 47, 0, 0) && std::strstr(g_why.text, "params"), "dst on params' last byte");
        expect(rule(0x1000, 0x2000, 0x2000 + 48, 0, 0) == nullptr, "dst right after params");
        expect(rule(0x1000, 0x2000, 0x3000, 0x2000 - 19, 0) != nullptr, "valid ends in params");
        expect(rule(0x1000, 0x2000, 0x3000, 0x3000 + 59, 0) != nullptr, "valid on dst's last byte");
        expect(rule(0x1000, 0x2000, 0x3000, 0x1000, 0) != nullptr, "valid is src");
        expect(rule(0x1000, 0x1000, 0x3000, 0, 0) == nullptr, "the inputs may share memory");
        expect(rule(0x1000, 0x2002, 0x3000, 0, 4) != nullptr && rule(0x1000, 0x2002, 0x3000, 0, 0) == nullptr,
               "device params must be 4-byte aligned, host params not");
    }
    {  // the path math
        const int n = 12, W = 160, H = 120;
        std::vector<float> pair((size_t)(n - 1) * 6, 0.0f), out((size_t)n * 6, 5.0f);
        std::vector<uint8_t> st((size_t)n, 9);
        int rep = -1;
        expect(dis_motion_stabilize(pair.data(), n, W, H, 3, 1.5f, 1.0f, out.data(), st.data(), &rep) == DIS_OK, "identity models");
        expect(all_zero_bits(out.data(), out.size()) && rep == 0, "identity models, zoom 1: +0.0f everywhere");
        for (uint8_t s : st) expect(s == 1, "identity models: status 1");
        // radius above the frame count, the longest window, null optional outputs
        for (int k = 0; k + 1 < n; ++k) pair[6 * k] = 1.5f, pair[6 * k + 3] = -0.25f;
        expect(dis_motion_stabilize(pair.data(), n, W, H, 1024, 1.0e30f, 1.0f, out.data(), nullptr, nullptr) == DIS_OK,
               "radius 1024 over 12 frames");
        // flat weights: every frame is moved onto the mean position, 5.5 pairs ahead of frame 0
        expect(std::fabs(out[0] + 5.5f * 1.5f) < 1e-5f && std::fabs(out[3] - 5.5f * 0.25f) < 1e-5f, "flat weights: the mean path");
        expect(dis_motion_stabilize(pair.data(), n, W, H, 0, 1e-45f, 2.0f, out.data(), st.data(), &rep) == DIS_OK, "radius 0");
        expect(out[0] == 79.5f * 0.5f && out[1] == -0.5f && out[2] == 0.0f && out[3] == 59.5f * 0.5f && out[4] == 0.0f &&
                   out[5] == -0.5f, "radius 0 over translations: M = Z");
        // one frame: pair_params is not read
        float one[6];
        uint8_t s1 = 9;
        expect(dis_motion_stabilize(nullptr, 1, 1, 1, 1024, 0.5f, 16.0f, one, &s1, &rep) == DIS_OK && s1 == 1 && rep == 0,
               "one frame of one pixel");
        expect(one[0] == 0.0f && one[1] == -0.9375f && one[5] == -0.9375f, "one pixel: the centre is the origin");
        // models that are not finite count as no motion
        pair[6 * 4 + 2] = nan, pair[6 * 7] = inf, pair[6 * 9 + 5] = -inf;
        expect(dis_motion_stabilize(pair.data(), n, W, H, 2, 1.0f, 1.0f, out.data(), st.data(), &rep) == DIS_OK && rep == 3,
               "three replaced models");
        for (float v : out) expect(std::isfinite(v), "replaced models leave finite corrections");
        // a pair whose linear part is zero: the later smoothed matrices cannot be inverted
        for (int e = 0; e < 6; ++e) pair[6 * 4 + e] = (e == 1 || e == 5) ? -1.0f : 0.0f;
        pair[6 * 7] = 1.5f, pair[6 * 9 + 5] = 0.0f;
        expect(dis_motion_stabilize(pair.data(), n, W, H, 1, 0.5f, 1.0f, out.data(), st.data(), &rep) == DIS_OK && rep == 0,
               "a collapsed path");
        expect(st[4] == 1 && st[5] == 1 && st[6] == 0 && st[11] == 0 && all_zero_bits(out.data() + 6 * 6, 6 * 6),
               "frames behind the collapse: status 0, zeros");
        // huge models overflow the path: whatever comes out is finite or zeroed
        for (float& v : pair) v = 3.0e38f;
        expect(dis_motion_stabilize(pair.data(), n, W, H, 3, 1.5f, 1.1f, out.data(), st.data(), &rep) == DIS_OK, "huge models");
        for (int k = 0; k < n; ++k)
            for (int e = 0; e < 6; ++e)
                expect(std::isfinite(out[6 * k + e]) && (st[k] == 1 || out[6 * k + e] == 0.0f), "an overflowed frame falls back");
        // refusals of the entry itself
        expect(dis_motion_stabilize(nullptr, 2, W, H, 1, 1.0f, 1.0f, out.data(), nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "null pair_params with two frames");
        expect(dis_motion_stabilize(pair.data(), 2, W, H, 1, 1.0f, 1.0f, nullptr, nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "null corrections");
        expect(dis_motion_stabilize(pair.data(), 2, W, H, 1, 1.0f, 1.0f, pair.data() + 3, nullptr, nullptr) ==
                   DIS_ERR_INVALID_ARGUMENT && dis::g_error.find("overlap") != std::string::npos, "corrections inside pair_params");
        expect(dis_motion_stabilize(pair.data(), 0, W, H, 1, 1.0f, 1.0f, out.data(), nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "no frames");
    }
    far::warp_model(&failures);  // the far cases of dis_warp_motion_u8 (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
