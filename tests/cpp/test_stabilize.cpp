// C++ test of the facade's stabilisation entries (include/dis/dis.hpp):
// dis::stabilizePath (with and without status and replaced) and dis::warpMotion
// (both borders, with and without valid), and the exception of a refused call.
// Compiled by tests/cpp/stabilize.mk and run on a GPU box by
// tests/test_gpu_stabilize.py, which passes a directory holding frames.u8 (n
// images of W x H x C samples) and pair.f32 ((n - 1) * 6 floats) and W, H, C, n,
// radius and zoom, and compares the words printed here ("bits <name> <hex
// words>") and the files written back (stab.u8, valid.u8, zero.u8) with
// tests/stabref.py's; exits non-zero on any failure of its own.
#include <cstdio>
#include <cstdlib>
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

static void save(const std::string& path, const std::vector<uint8_t>& v)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), 1, v.size(), f) != v.size() || std::fclose(f) != 0) {
        std::printf("FAIL: cannot write %s\n", path.c_str());
        ++failures;
    }
}

static void bits(const char* name, const std::vector<float>& v)
{
    std::printf("bits %s", name);
    for (float x : v) {
        uint32_t w;
        std::memcpy(&w, &x, 4);
        std::printf(" %08x", w);
    }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 8) {
        std::printf("usage: test_stabilize <directory of raw inputs> W H C n radius zoom\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), C = std::atoi(argv[4]), n = std::atoi(argv[5]);
    const int radius = std::atoi(argv[6]);
    const float zoom = (float)std::atof(argv[7]);
    const size_t px = (size_t)W * H * n;
    const auto frames = load<uint8_t>(dir + "frames.u8", px * C);
    const auto pair = load<float>(dir + "pair.f32", (size_t)(n - 1) * 6);
    if (failures) return 1;
    try {
        const float sigma = (float)(radius > 1 ? radius : 1) / 2.0f;
        const std::vector<float> plain = dis::stabilizePath(pair.data(), n, W, H, radius, sigma);
        bits("plain", plain);
        std::vector<uint8_t> status((size_t)n, 9);
        int replaced = -1;
        const std::vector<float> corr = dis::stabilizePath(pair.data(), n, W, H, radius, sigma, zoom, status.data(), &replaced);
        bits("zoomed", corr);
        EXPECT(corr.size() == (size_t)n * 6, "n * 6 corrections");
        for (uint8_t s : status) EXPECT(s == 1, "every frame has a correction");
        EXPECT(replaced == 0, "no model was replaced");
        std::vector<uint8_t> stab(px * C, 7), valid(px, 7), zero(px * C, 7);
        dis::warpMotion(frames.data(), C, corr.data(), n, W, H, stab.data(), dis::Border::REPLICATE, valid.data());
        dis::warpMotion(frames.data(), C, corr.data(), n, W, H, zero.data(), dis::Border::ZERO);
        save(dir + "stab.u8", stab);
        save(dir + "valid.u8", valid);
        save(dir + "zero.u8", zero);
        bool refused = false;
        try {
            dis::stabilizePath(pair.data(), n, W, H, 1025, sigma);
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "radius = 1025 is refused");
        refused = false;
        try {
            dis::warpMotion(frames.data(), 2, corr.data(), n, W, H, stab.data());
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
