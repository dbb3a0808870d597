// C++ test of the facade's homography entries (include/dis/dis.hpp):
// dis::fitHomography in its f32 and half_bits forms (with mask, info and
// inliers), dis::homographyToFlow, dis::stabilizePathHomography and
// dis::warpHomography, and the exception of a refused call. Compiled by
// tests/cpp/homography.mk and run on a GPU box by tests/test_gpu_homography.py,
// which passes a directory holding flow.f32, flow.f16 and mask.u8 (n fields of W
// x H), frames.u8 (n images of W x H x 3 samples) and pair.f32 ((n - 1) * 8
// floats) and W, H, n, and compares the words printed here ("bits <name> <hex
// words>") and the files written back (warp.u8, valid.u8) with
// tests/homographyref.py's; exits non-zero on any failure of its own.
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

template <class T>
static void bits(const char* name, const std::vector<T>& v)
{
    std::printf("bits %s", name);
    for (T x : v) {
        uint32_t w;
        std::memcpy(&w, &x, 4);
        std::printf(" %08x", w);
    }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::printf("usage: test_homography <directory of raw inputs> W H n\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n = std::atoi(argv[4]), C = 3;
    const size_t px = (size_t)W * H * n;
    const auto flow = load<float>(dir + "flow.f32", px * 2);
    const auto flow16 = load<dis::half_bits>(dir + "flow.f16", px * 2);
    const auto mask = load<uint8_t>(dir + "mask.u8", px);
    const auto frames = load<uint8_t>(dir + "frames.u8", px * C);
    const auto pair = load<float>(dir + "pair.f32", (size_t)(n - 1) * 8);
    if (failures) return 1;
    try {
        std::vector<float> plain((size_t)n * 8, 5.0f), masked((size_t)n * 8, 5.0f), half((size_t)n * 8, 5.0f);
        std::vector<uint32_t> info((size_t)n * 4, 9);
        std::vector<uint8_t> inliers(px, 9);
        dis::fitHomography(flow.data(), n, W, H, plain.data());
        bits("plain", plain);
        dis::fitHomography(flow.data(), n, W, H, masked.data(), 2, 0.75f, mask.data(), info.data(), inliers.data());
        bits("masked", masked);
        bits("masked_info", info);
        size_t agree = 0;
        for (uint8_t b : inliers) {
            EXPECT(b == 0 || b == 255, "an inlier byte is 0 or 255");
            agree += b == 255;
        }
        std::printf("bits masked_agree %zu\n", agree);
        dis::fitHomography(flow16.data(), n, W, H, half.data(), 0, 1.0f, mask.data());
        bits("half", half);
        EXPECT(dis::fitHomographyWorkspace(n, W, H) == (size_t)n * (((size_t)W * H + 16383) / 16384 * 27 + 16) * 8,
               "the workspace formula");
        std::vector<float> field(px * 2, 5.0f);
        std::vector<dis::half_bits> field16(px * 2, 5);
        dis::homographyToFlow(plain.data(), n, W, H, field.data());
        dis::homographyToFlow(plain.data(), n, W, H, field16.data());
        unsigned long long sum = 0, sum16 = 0;
        for (float x : field) {
            uint32_t w;
            std::memcpy(&w, &x, 4);
            sum += w;
        }
        for (dis::half_bits x : field16) sum16 += x;
        std::printf("bits field_sum %llx\nbits field16_sum %llx\n", sum, sum16);
        std::vector<uint8_t> status((size_t)n, 9);
        int replaced = -1;
        const std::vector<float> corr = dis::stabilizePathHomography(pair.data(), n, W, H, 2, 1.0f, 1.25f, status.data(), &replaced);
        bits("corrections", corr);
        EXPECT(corr.size() == (size_t)n * 8 && replaced == 0, "n * 8 corrections, no model replaced");
        for (uint8_t s : status) EXPECT(s == 1, "every frame has a correction");
        std::vector<uint8_t> warp(px * C, 7), valid(px, 7), zero(px * C, 7);
        dis::warpHomography(frames.data(), C, corr.data(), n, W, H, warp.data(), dis::Border::REPLICATE, valid.data());
        dis::warpHomography(frames.data(), C, corr.data(), n, W, H, zero.data(), dis::Border::ZERO);
        save(dir + "warp.u8", warp);
        save(dir + "valid.u8", valid);
        save(dir + "zero.u8", zero);
        bool refused = false;
        try {
            dis::fitHomography(flow.data(), n, W, H, plain.data(), 17);
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "iterations = 17 is refused");
        refused = false;
        try {
            dis::warpHomography(frames.data(), 2, corr.data(), n, W, H, warp.data());
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "two channels are refused");
        refused = false;
        try {
            dis::stabilizePathHomography(pair.data(), n, W, H, 1025, 1.0f);
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "radius = 1025 is refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
