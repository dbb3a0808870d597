// C++ test of the facade's flow warp (include/dis/dis.hpp): dis::flowWarp in
// its f32 form (the defaults: scale 1, Border::REPLICATE; with valid) and its
// f16 form (half_bits flow, scale 0.5, Border::ZERO, no valid) against the
// bytes tests/warpref.py expects, and the exception of a refused call.
// Compiled and run on a GPU box by tests/test_gpu_warp.py, which passes a
// directory holding the raw inputs and expected outputs of its
// (W, H, n, C) = (67, 33, 2, 3) case; exits non-zero on any failure.
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
    const int W = 67, H = 33, n = 2, C = 3;
    const size_t px = (size_t)W * H * n;
    if (argc < 2) {
        std::printf("usage: test_warp <directory of raw inputs and expected outputs>\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const auto src = load<uint8_t>(dir + "src.u8", px * C);
    const auto flow32 = load<float>(dir + "flow.f32", px * 2);
    const auto flow16 = load<dis::half_bits>(dir + "flow.f16", px * 2);
    const auto exp32 = load<uint8_t>(dir + "dst_f32.u8", px * C);
    const auto exp_valid = load<uint8_t>(dir + "valid_f32.u8", px);
    const auto exp16 = load<uint8_t>(dir + "dst_f16.u8", px * C);
    if (failures) return 1;
    try {
        std::vector<uint8_t> dst(px * C, 9), valid(px, 9);
        dis::flowWarp(src.data(), C, flow32.data(), n, W, H, dst.data());
        EXPECT(dst == exp32, "f32 flow, defaults");
        std::fill(dst.begin(), dst.end(), 9);
        dis::flowWarp(src.data(), C, flow32.data(), n, W, H, dst.data(), 1.0f, dis::Border::REPLICATE, valid.data());
        EXPECT(dst == exp32, "f32 flow, with valid");
        EXPECT(valid == exp_valid, "f32 flow, valid");
        std::fill(dst.begin(), dst.end(), 9);
        dis::flowWarp(src.data(), C, flow16.data(), n, W, H, dst.data(), 0.5f, dis::Border::ZERO);
        EXPECT(dst == exp16, "f16 flow, scale 0.5, Border::ZERO");
        EXPECT(exp16 != exp32, "the two cases differ");
        bool refused = false;
        try {
            dis::flowWarp(src.data(), 2, flow32.data(), n, W, H, dst.data());
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "two channels are refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
