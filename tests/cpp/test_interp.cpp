// C++ test of the facade's frame interpolation (include/dis/dis.hpp):
// dis::flowInterp in its f32 form (with bw and fill) and its f16 form
// (half_bits flows, no bw, no fill) against the bytes tests/interpref.py
// expects, dis::flowInterpWorkspace, and the exception of a refused call.
// Compiled and run on a GPU box by tests/test_gpu_interp.py, which passes a
// directory holding the raw inputs and expected outputs of a
// (W, H, n, C) = (37, 23, 3, 3) case at t = 0.25; exits non-zero on any failure.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "dis/dis.hpp"

static int failures = 0;
#define EXPECT(cond, msg)                                               \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

template <class T>
static std::vector<T> load(const std::string& path, size_t count)
{
    std::vector<T> v(count);
    std::FILE* f = std::fopen(path.c_str(), "rb");
    const size_t got = f ? std::fread(v.data(), sizeof(T), count, f) : 0;
    const bool at_end = f && std::fgetc(f) == EOF;
    if (f) std::fclose(f);
    if (got != count || !at_end) {
        std::printf("FAIL: %s does not hold %zu values\n", path.c_str(), count);
        ++failures;
    }
    return v;
}

int main(int argc, char** argv)
{
    const int W = 37, H = 23, n = 3, C = 3;
    const float t = 0.25f;
    const size_t px = (size_t)W * H * n;
    if (argc < 2) {
        std::printf("usage: test_interp <directory of raw inputs and expected outputs>\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const auto I0 = load<uint8_t>(dir + "I0.u8", px * C);
    const auto I1 = load<uint8_t>(dir + "I1.u8", px * C);
    const auto fw32 = load<float>(dir + "fw.f32", px * 2);
    const auto bw32 = load<float>(dir + "bw.f32", px * 2);
    const auto fw16 = load<dis::half_bits>(dir + "fw.f16", px * 2);
    const auto exp32 = load<uint8_t>(dir + "dst_f32_bw.u8", px * C);
    const auto exp_fill = load<uint8_t>(dir + "fill_f32_bw.u8", px);
    const auto exp16 = load<uint8_t>(dir + "dst_f16.u8", px * C);
    if (failures) return 1;
    try {
        EXPECT(dis::flowInterpWorkspace(n, W, H) == px * 8, "workspace bytes");
        std::vector<uint8_t> dst(px * C, 9), fill(px, 9);
        dis::flowInterp(I0.data(), I1.data(), C, fw32.data(), bw32.data(), n, W, H, t, dst.data(), fill.data());
        EXPECT(dst == exp32, "f32 flows, with bw");
        EXPECT(fill == exp_fill, "f32 flows, fill");
        std::fill(dst.begin(), dst.end(), 9);
        dis::flowInterp(I0.data(), I1.data(), C, fw16.data(), nullptr, n, W, H, t, dst.data());
        EXPECT(dst == exp16, "f16 flow, no bw");
        EXPECT(exp16 != exp32, "the two cases differ");
        bool refused = false;
        try {
            dis::flowInterp(I0.data(), I1.data(), C, fw32.data(), nullptr, n, W, H, 1.5f, dst.data());
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "t = 1.5 is refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
