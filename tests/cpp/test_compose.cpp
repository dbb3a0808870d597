// C++ test of the facade's flow composition (include/dis/dis.hpp):
// dis::flowCompose in its f32 form (without the byte planes, with them, and in
// place) and its half_bits form (an f16 second field into an f32 result), and
// dis::advectPoints, against the bytes tests/composeref.py expects, and the
// exception of a refused call. Compiled and run on a GPU box by
// tests/test_gpu_compose.py, which passes a directory holding the raw inputs
// and expected outputs of its (W, H, n) = (67, 33, 2) case; exits non-zero on
// any failure. Flows are compared as bit patterns (invalid pixels hold NaN).
#include <cstdio>
#include <cstring>
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main(int argc, char** argv)
{
    const int W = 67, H = 33, n = 2, count = 63;
    const size_t px = (size_t)W * H * n, pts = (size_t)n * count;
    if (argc < 2) {
        std::printf("usage: test_compose <directory of raw inputs and expected outputs>\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const auto a32 = load<float>(dir + "a.f32", px * 2);
    const auto b32 = load<float>(dir + "b.f32", px * 2);
    const auto b16 = load<dis::half_bits>(dir + "b.f16", px * 2);
    const auto valid_a = load<uint8_t>(dir + "valid_a.u8", px);
    const auto mask_b = load<uint8_t>(dir + "mask_b.u8", px);
    const auto exp_plain = load<float>(dir + "out_plain.f32", px * 2);
    const auto exp_gated = load<float>(dir + "out_gated.f32", px * 2);
    const auto exp_gated_valid = load<uint8_t>(dir + "valid_gated.u8", px);
    const auto exp_half = load<float>(dir + "out_half.f32", px * 2);
    const auto exp_half_valid = load<uint8_t>(dir + "valid_half.u8", px);
    const auto points = load<float>(dir + "points.f32", pts * 2);
    const auto exp_moved = load<float>(dir + "moved.f32", pts * 2);
    const auto exp_status = load<uint8_t>(dir + "status.u8", pts);
    if (failures) return 1;
    try {
        std::vector<float> out(px * 2, 9.0f);
        std::vector<uint8_t> valid(px, 9);
        dis::flowCompose(a32.data(), b32.data(), n, W, H, out.data());
        EXPECT(same_bits(out, exp_plain), "f32 fields, defaults");
        dis::flowCompose(a32.data(), b32.data(), n, W, H, out.data(), valid_a.data(), mask_b.data(), valid.data());
        EXPECT(same_bits(out, exp_gated), "f32 fields, valid_a and mask_b");
        EXPECT(valid == exp_gated_valid, "f32 fields, valid_out");
        EXPECT(!same_bits(exp_gated, exp_plain), "the planes change the result");
        std::vector<float> acc = a32;  // in place: the accumulator is both a and out
        dis::flowCompose(acc.data(), b32.data(), n, W, H, acc.data());
        EXPECT(same_bits(acc, exp_plain), "f32 fields, in place");
        std::fill(valid.begin(), valid.end(), 9);
        dis::flowCompose(a32.data(), b16.data(), n, W, H, out.data(), nullptr, nullptr, valid.data());
        EXPECT(same_bits(out, exp_half), "f16 second field into an f32 result");
        EXPECT(valid == exp_half_valid, "f16 second field, valid_out");
        EXPECT(!same_bits(exp_half, exp_plain), "the two forms differ");
        std::vector<float> moved(pts * 2, 9.0f);
        std::vector<uint8_t> status(pts, 9);
        dis::advectPoints(b32.data(), n, W, H, points.data(), count, moved.data(), status.data());
        EXPECT(same_bits(moved, exp_moved), "advectPoints");
        EXPECT(status == exp_status, "advectPoints, status");
        bool refused = false;
        try {
            dis::flowCompose(a32.data(), out.data(), n, W, H, out.data());  // out is b
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "out == b is refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
