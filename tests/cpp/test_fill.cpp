// C++ test of the facade's flow fill (include/dis/dis.hpp): dis::flowFill in its
// f32 form (without a mask, with one and the level map, and in place) and its
// half_bits form (an f16 field into an f32 result), dis::flowFillWorkspace, and
// the exception of a refused call. Compiled and run on a GPU box by
// tests/test_gpu_fill.py, which passes a directory holding the raw inputs of
// the first two fields of its (W, H, n) = (67, 33, 3) case and compares the
// FNV-1a digests printed here ("digest <name> <16 hex digits>") with those of
// the Python path's results; exits non-zero on any failure of its own.
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

template <class T>
static void digest(const char* name, const std::vector<T>& v)
{
    unsigned long long h = 0xcbf29ce484222325ull;  // FNV-1a, 64 bits, over the bytes
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    std::printf("digest %s %016llx\n", name, h);
}

int main(int argc, char** argv)
{
    const int W = 67, H = 33, n = 2;
    const size_t px = (size_t)W * H * n;
    if (argc < 2) {
        std::printf("usage: test_fill <directory of raw inputs>\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const auto f32 = load<float>(dir + "flow.f32", px * 2);
    const auto f16 = load<dis::half_bits>(dir + "flow.f16", px * 2);
    const auto mask = load<uint8_t>(dir + "mask.u8", px);
    if (failures) return 1;
    try {
        EXPECT(dis::flowFillWorkspace(n, W, H) == 8u * n * 800u, "flowFillWorkspace: 800 cells a field");
        EXPECT(dis::flowFillWorkspace(5, 1, 1) == 0, "flowFillWorkspace: none for 1 x 1");
        std::vector<float> out(px * 2, 9.0f);
        std::vector<uint8_t> level(px, 9);
        dis::flowFill(f32.data(), n, W, H, out.data());
        digest("plain", out);
        dis::flowFill(f32.data(), n, W, H, out.data(), mask.data(), level.data());
        digest("masked", out);
        digest("masked_level", level);
        std::vector<float> acc = f32;  // in place: the field is both flow and out
        dis::flowFill(acc.data(), n, W, H, acc.data(), mask.data());
        EXPECT(std::memcmp(acc.data(), out.data(), px * 8) == 0, "f32 field, in place");
        std::fill(level.begin(), level.end(), 9);
        dis::flowFill(f16.data(), n, W, H, out.data(), mask.data(), level.data());
        digest("half", out);
        digest("half_level", level);
        bool refused = false;
        try {
            dis::flowFill(f32.data(), n, W, H, out.data(), reinterpret_cast<const uint8_t*>(out.data()));  // mask is out
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "mask == out is refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
