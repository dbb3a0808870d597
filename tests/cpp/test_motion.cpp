// C++ test of the facade's global-motion fit (include/dis/dis.hpp):
// dis::fitMotion in its f32 form (affine without a mask; similarity with mask,
// info and inliers) and its half_bits form (translation, no refit),
// dis::fitMotionWorkspace, dis::motionToFlow into f32 and half_bits fields, and
// the exception of a refused call. Compiled and run on a GPU box by
// tests/test_gpu_motion.py, which passes a directory holding the raw inputs of
// one of its cases and W, H, n, and compares the words printed here
// ("bits <name> <hex words>") with those of the Python path's results; exits
// non-zero on any failure of its own.
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

template <class T>
static void bits(const char* name, const std::vector<T>& v)  // T: four bytes
{
    std::printf("bits %s", name);
    for (const T& x : v) {
        uint32_t w;
        std::memcpy(&w, &x, 4);
        std::printf(" %08x", w);
    }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::printf("usage: test_motion <directory of raw inputs> W H n\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n = std::atoi(argv[4]);
    const size_t px = (size_t)W * H * n;
    const auto f32 = load<float>(dir + "flow.f32", px * 2);
    const auto f16 = load<dis::half_bits>(dir + "flow.f16", px * 2);
    const auto mask = load<uint8_t>(dir + "mask.u8", px);
    if (failures) return 1;
    try {
        const size_t chunks = ((size_t)W * H + 16383) / 16384;
        EXPECT(dis::fitMotionWorkspace(n, W, H) == (size_t)n * (chunks * 12 + 16) * 8, "fitMotionWorkspace");
        std::vector<float> params((size_t)n * 6, 9.0f);
        dis::fitMotion(f32.data(), n, W, H, params.data());  // affine, three refits within 1 px
        bits("plain", params);
        const std::vector<float> plain = params;
        std::vector<uint32_t> info((size_t)n * 4, 9);
        std::vector<uint8_t> inliers(px, 9);
        dis::fitMotion(f32.data(), n, W, H, params.data(), dis::MotionModel::SIMILARITY, 3, 1.0f, mask.data(), info.data(),
                       inliers.data());
        bits("masked", params);
        bits("masked_info", info);
        unsigned long long agree = 0;
        for (uint8_t b : inliers) {
            EXPECT(b == 0 || b == 255, "an inlier byte is 0 or 255");
            agree += b == 255;
        }
        std::printf("bits masked_agree %llu\n", agree);
        dis::fitMotion(f16.data(), n, W, H, params.data(), dis::MotionModel::TRANSLATION, 0, 1.0f, mask.data());
        bits("half", params);
        std::vector<float> field(px * 2, 9.0f);
        dis::motionToFlow(plain.data(), n, W, H, field.data());
        unsigned long long sum = 0;
        for (float v : field) {
            uint32_t w;
            std::memcpy(&w, &v, 4);
            sum += w;
        }
        std::printf("bits field_sum %llx\n", sum);
        std::vector<dis::half_bits> field16(px * 2, 9);
        dis::motionToFlow(plain.data(), n, W, H, field16.data());
        sum = 0;
        for (dis::half_bits v : field16) sum += v;
        std::printf("bits field16_sum %llx\n", sum);
        bool refused = false;
        try {
            dis::fitMotion(f32.data(), n, W, H, params.data(), dis::MotionModel::AFFINE, 17);
        } catch (const dis::Error& e) {
            refused = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(refused, "iterations = 17 is refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
