// args_homography_host.cpp -- dis_homography_stabilize (csrc/dis_stabilize.cpp)
// and the argument rules of the homography family (csrc/dis_args.h) at their
// edges: the scale of the fit's coordinates, the workspace size, the overlap
// rules over the ranges of dis_warp_homography_u8 and
// dis_homography_stabilize (32 bytes a model), and the path math on exact
// cases, the longest window, one frame, null optional outputs, affine inputs
// and models that are not finite or collapse the path. Built with
// -fsanitize=address,undefined by tests/cpp/homography.mk (target
// args_homography) and run by tests/test_homography_host.py. The buffers handed
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
    {  // the scale: the smallest power of two >= max(W, H, 2) / 2
        expect(dis::homography_scale(1, 1) == 1 && dis::homography_scale(2, 1) == 1 && dis::homography_scale(1, 3) == 2,
               "the smallest frames");
        expect(dis::homography_scale(4, 4) == 2 && dis::homography_scale(5, 3) == 4 && dis::homography_scale(8, 9) == 8,
               "around a power of two");
        expect(dis::homography_scale(320, 240) == 256 && dis::homography_scale(1920, 1080) == 1024 &&
                   dis::homography_scale(512, 2) == 256 && dis::homography_scale(513, 2) == 512, "common frames");
        expect(dis::homography_scale(dis::kMaxExactSide, 1) == (1 << 23) && dis::homography_scale(1, dis::kMaxExactSide) == (1 << 23),
               "the largest side");
    }
    {  // the workspace
        size_t b = 5;
        expect(dis::check_homography_workspace(1, 1, 1, &b) == nullptr && b == (27 + 16) * 8, "one pixel");
        expect(dis::check_homography_workspace(3, 257, 64, &b) == nullptr && b == 3 * (2 * 27 + 16) * 8, "two chunks");
        expect(dis::check_homography_workspace(1, 65536, 32768, &b) == nullptr && b == (131072ull * 27 + 16) * 8, "2^31 pixels");
        b = 5;
        expect(dis::check_homography_workspace(0, 4, 4, &b) && dis::check_homography_workspace(1, 0, 4, &b) &&
                   dis::check_homography_workspace(1, 4, -1, &b) && dis::check_homography_workspace(1, dis::kMaxExactSide + 1, 1, &b) &&
                   dis::check_homography_workspace(1, 65536, 32769, &b) &&
                   dis::check_homography_workspace(16384, dis::kMaxExactSide, 128, &b) && b == 5, "refused sizes leave bytes alone");
    }
    {  // the buffers of dis_warp_homography_u8: two images of 10 pixels of 3 channels, 64 bytes of params
        auto rule = [](uintptr_t src, uintptr_t par, uintptr_t dst, uintptr_t valid, size_t align) {
            return dis::check_warp_homography_buffers(src, 60, par, 2, dst, 60, valid, 20, align, &g_why);
        };
        expect(rule(0x1000, 0x2000, 0x3000, 0x4000, 4) == nullptr, "all apart");
        expect(rule(0x1000, 0x2000, 0x1000 + 60, 0, 0) == nullptr, "dst right after src");
        expect(rule(0x1000, 0x2000, 0x1000 + 59, 0, 0) && std::strstr(g_why.text, "dst") && std::strstr(g_why.text, "src"),
               "dst on src's last byte");
        expect(rule(0x1000, 0x2000, 0x2000 + 63, 0, 0) && std::strstr(g_why.text, "params"), "dst on params' last byte");
        expect(rule(0x1000, 0x2000, 0x2000 + 64, 0, 0) == nullptr, "dst right after params");
        expect(rule(0x1000, 0x2000, 0x3000, 0x2000 - 19, 0) != nullptr, "valid ends in params");
        expect(rule(0x1000, 0x2000, 0x3000, 0x3000 + 59, 0) != nullptr, "valid on dst's last byte");
        expect(rule(0x1000, 0x2000, 0x3000, 0x1000, 0) != nullptr, "valid is src");
        expect(rule(0x1000, 0x1000, 0x3000, 0, 0) == nullptr, "the inputs may share memory");
        expect(rule(0x1000, 0x2002, 0x3000, 0, 4) != nullptr && rule(0x1000, 0x2002, 0x3000, 0, 0) == nullptr,
               "device params must be 4-byte aligned, host params not");
    }
    {  // the overlap rule of dis_homography_stabilize: pair | corrections, status, replaced (4 frames: 96 | 128, 4, 4)
        auto rule = [](uintptr_t pair, uintptr_t out, uintptr_t st, uintptr_t rep, int n) {
            return dis::check_homography_stabilize_buffers(pair, out, st, rep, n, &g_why);
        };
        expect(rule(0x1000, 0x2000, 0x3000, 0x4000, 4) == nullptr, "all apart");
        expect(rule(0x1000, 0x1000 + 96, 0, 0, 4) == nullptr, "corrections right after pair_params");
        expect(rule(0x1000, 0x1000 + 95, 0, 0, 4) && std::strstr(g_why.text, "corrections") && std::strstr(g_why.text, "pair_params"),
               "corrections on pair_params' last byte");
        expect(rule(0x1000, 0x1000 - 127, 0, 0, 4) != nullptr, "corrections end in pair_params");
        expect(rule(0x1000, 0x1000 - 128, 0, 0, 4) == nullptr, "corrections right before pair_params");
        expect(rule(0x1000, 0x2000, 0x2000 + 127, 0, 4) && std::strstr(g_why.text, "status"), "status on corrections' last byte");
        expect(rule(0x1000, 0x2000, 0x2000 + 128, 0, 4) == nullptr, "status right after corrections");
        expect(rule(0x1000, 0x2000, 0x3000, 0x3000 + 3, 4) && std::strstr(g_why.text, "replaced"), "replaced on status' last byte");
        expect(rule(0x1000, 0x2000, 0x3000, 0x2000 + 124, 4) != nullptr, "replaced in corrections");
        expect(rule(0, 0x2000, 0x3000, 0x4000, 1) == nullptr, "one frame: no pair_params");
        expect(rule(UINTPTR_MAX - 95, UINTPTR_MAX - 127, 0, 0, 4) != nullptr, "no wrap at the top of the address space");
    }
    {  // the path math
        const int n = 12, W = 160, H = 120;
        std::vector<float> pair((size_t)(n - 1) * 8, 0.0f), out((size_t)n * 8, 5.0f);
        std::vector<uint8_t> st((size_t)n, 9);
        int rep = -1;
        expect(dis_homography_stabilize(pair.data(), n, W, H, 3, 1.5f, 1.0f, out.data(), st.data(), &rep) == DIS_OK, "identity models");
        expect(all_zero_bits(out.data(), out.size()) && rep == 0, "identity models, zoom 1: +0.0f everywhere");
        for (uint8_t s : st) expect(s == 1, "identity models: status 1");
        // translations: radius above the frame count, the longest window, null optional outputs
        for (int k = 0; k + 1 < n; ++k) pair[8 * k] = 1.5f, pair[8 * k + 3] = -0.25f;
        expect(dis_homography_stabilize(pair.data(), n, W, H, 1024, 1.0e30f, 1.0f, out.data(), nullptr, nullptr) == DIS_OK,
               "radius 1024 over 12 frames");
        expect(std::fabs(out[0] + 5.5f * 1.5f) < 1e-5f && std::fabs(out[3] - 5.5f * 0.25f) < 1e-5f, "flat weights: the mean path");
        for (int k = 0; k < n; ++k) expect(all_zero_bits(out.data() + 8 * k + 6, 2), "affine inputs: q6 = q7 = +0.0f");
        expect(dis_homography_stabilize(pair.data(), n, W, H, 0, 1e-45f, 2.0f, out.data(), st.data(), &rep) == DIS_OK, "radius 0");
        expect(out[0] == 79.5f * 0.5f && out[1] == -0.5f && out[2] == 0.0f && out[3] == 59.5f * 0.5f && out[4] == 0.0f &&
                   out[5] == -0.5f && all_zero_bits(out.data() + 6, 2), "radius 0 over translations: M = Z");
        // projective pairs: finite corrections with a projective row
        for (int k = 0; k + 1 < n; ++k) pair[8 * k + 6] = (k & 1) ? 4e-5f : -6e-5f, pair[8 * k + 7] = 2e-5f;
        expect(dis_homography_stabilize(pair.data(), n, W, H, 3, 1.5f, 1.1f, out.data(), st.data(), &rep) == DIS_OK && rep == 0,
               "projective pairs");
        bool any = false;
        for (int k = 0; k < n; ++k) {
            expect(st[k] == 1, "projective pairs: status 1");
            for (int e = 0; e < 8; ++e) expect(std::isfinite(out[8 * k + e]), "projective pairs: finite");
            any = any || out[8 * k + 6] != 0.0f;
        }
        expect(any, "projective pairs leave a projective row");
        // one frame: pair_params is not read
        float one[8];
        uint8_t s1 = 9;
        expect(dis_homography_stabilize(nullptr, 1, 1, 1, 1024, 0.5f, 16.0f, one, &s1, &rep) == DIS_OK && s1 == 1 && rep == 0,
               "one frame of one pixel");
        expect(one[0] == 0.0f && one[1] == -0.9375f && one[5] == -0.9375f && one[6] == 0.0f && one[7] == 0.0f,
               "one pixel: the centre is the origin");
        // models that are not finite count as no motion
        pair[8 * 4 + 2] = nan, pair[8 * 7 + 6] = inf, pair[8 * 9 + 7] = -inf;
        expect(dis_homography_stabilize(pair.data(), n, W, H, 2, 1.0f, 1.0f, out.data(), st.data(), &rep) == DIS_OK && rep == 3,
               "three replaced models");
        for (float v : out) expect(std::isfinite(v), "replaced models leave finite corrections");
        // a pair whose linear part is zero: the later smoothed matrices cannot be inverted
        for (int e = 0; e < 8; ++e) pair[8 * 4 + e] = (e == 1 || e == 5) ? -1.0f : 0.0f;
        pair[8 * 7 + 6] = 0.0f, pair[8 * 9 + 7] = 0.0f;
        expect(dis_homography_stabilize(pair.data(), n, W, H, 1, 0.5f, 1.0f, out.data(), st.data(), &rep) == DIS_OK && rep == 0,
               "a collapsed path");
        expect(st[4] == 1 && st[6] == 0 && st[11] == 0 && all_zero_bits(out.data() + 8 * 6, 8 * 6),
               "frames behind the collapse: status 0, zeros");
        // a pair whose bottom-right entry becomes zero: the path is not finite from there on
        for (float& v : pair) v = 0.0f;
        pair[8 * 2] = 1.0f, pair[8 * 3 + 6] = -1.0f;  // C_3 is a shift by 1 in x: (A_3 . C_3)_22 = -1 * 1 + 1 = 0
        expect(dis_homography_stabilize(pair.data(), n, W, H, 1, 0.5f, 1.0f, out.data(), st.data(), &rep) == DIS_OK,
               "a path through a zero bottom-right entry");
        for (int k = 0; k < n; ++k)
            for (int e = 0; e < 8; ++e)
                expect(std::isfinite(out[8 * k + e]) && (st[k] == 1 || out[8 * k + e] == 0.0f), "such a frame falls back");
        // huge models overflow the path: whatever comes out is finite or zeroed
        for (float& v : pair) v = 3.0e38f;
        expect(dis_homography_stabilize(pair.data(), n, W, H, 3, 1.5f, 1.1f, out.data(), st.data(), &rep) == DIS_OK, "huge models");
        for (int k = 0; k < n; ++k)
            for (int e = 0; e < 8; ++e)
                expect(std::isfinite(out[8 * k + e]) && (st[k] == 1 || out[8 * k + e] == 0.0f), "an overflowed frame falls back");
        // refusals of the entry itself
        expect(dis_homography_stabilize(nullptr, 2, W, H, 1, 1.0f, 1.0f, out.data(), nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "null pair_params with two frames");
        expect(dis_homography_stabilize(pair.data(), 2, W, H, 1, 1.0f, 1.0f, nullptr, nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "null corrections");
        expect(dis_homography_stabilize(pair.data(), 2, W, H, 1, 1.0f, 1.0f, pair.data() + 3, nullptr, nullptr) ==
                   DIS_ERR_INVALID_ARGUMENT && dis::g_error.find("overlap") != std::string::npos, "corrections inside pair_params");
        expect(dis_homography_stabilize(pair.data(), 0, W, H, 1, 1.0f, 1.0f, out.data(), nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "no frames");
        expect(dis_homography_stabilize(pair.data(), 2, W, H, 1025, 1.0f, 1.0f, out.data(), nullptr, nullptr) ==
                   DIS_ERR_INVALID_ARGUMENT &&
                   dis_homography_stabilize(pair.data(), 2, W, H, 1, nan, 1.0f, out.data(), nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT &&
                   dis_homography_stabilize(pair.data(), 2, W, H, 1, 1.0f, 0.5f, out.data(), nullptr, nullptr) == DIS_ERR_INVALID_ARGUMENT,
               "radius, sigma, zoom");
    }
    far::motion(27, &failures);  // the far cases (far_cases.h; dis_warp_homography_u8's sizes are dis_warp_motion_u8's rule,
                                  // which args_stabilize_host runs at them)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
