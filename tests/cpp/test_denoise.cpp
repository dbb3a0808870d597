// C++ test of the facade's temporal denoising (include/dis/dis.hpp):
// dis::denoiseWeights, dis::temporalDenoise in its f32 form (two neighbours, a
// mask for the second one only, with support) and its half_bits form (no masks,
// no support), and the exception of a refused call. Compiled and run on a GPU
// box by tests/test_gpu_denoise.py, which passes a directory holding the raw
// inputs of one of its cases and W, H, n, C, and compares the files written
// here (dst_f32.u8, support_f32.u8, dst_f16.u8, table.f32) with the
// restatement's results; exits non-zero on any failure of its own.
#include <cstdio>
#include <cstdlib>
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
static void store(const std::string& path, const std::vector<T>& v)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    const bool ok = f && std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) std::fclose(f);
    EXPECT(ok, "cannot write a result file");
}

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::printf("usage: test_denoise DIR W H n C\n");
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n = std::atoi(argv[4]), C = std::atoi(argv[5]);
    const size_t px = (size_t)W * H * n;
    const auto cur = load<uint8_t>(dir + "cur.u8", px * C);
    const auto nb0 = load<uint8_t>(dir + "nb0.u8", px * C), nb1 = load<uint8_t>(dir + "nb1.u8", px * C);
    const auto f0 = load<float>(dir + "flow0.f32", px * 2), f1 = load<float>(dir + "flow1.f32", px * 2);
    const auto h0 = load<dis::half_bits>(dir + "flow0.f16", px * 2), h1 = load<dis::half_bits>(dir + "flow1.f16", px * 2);
    const auto m1 = load<uint8_t>(dir + "mask1.u8", px);
    if (failures) return 1;
    try {
        const std::vector<float> table = dis::denoiseWeights(12.0f);
        EXPECT(table.size() == 256 && table[0] == 1.0f && table[255] < table[1], "the weight table");
        store(dir + "table.f32", table);
        const uint8_t* nbs[2] = {nb0.data(), nb1.data()};
        const float* fls[2] = {f0.data(), f1.data()};
        const uint8_t* masks[2] = {nullptr, m1.data()};
        std::vector<uint8_t> dst(px * C, 9), support(px, 9);
        dis::temporalDenoise(cur.data(), nbs, C, fls, 2, n, W, H, table.data(), dst.data(), masks, support.data());
        store(dir + "dst_f32.u8", dst);
        store(dir + "support_f32.u8", support);
        const dis::half_bits* hls[2] = {h0.data(), h1.data()};
        std::vector<uint8_t> dst16(px * C, 9);
        dis::temporalDenoise(cur.data(), nbs, C, hls, 2, n, W, H, table.data(), dst16.data());
        store(dir + "dst_f16.u8", dst16);
        bool thrown = false;
        try {  // dst cannot be cur
            dis::temporalDenoise(cur.data(), nbs, C, fls, 2, n, W, H, table.data(), const_cast<uint8_t*>(cur.data()));
        } catch (const dis::Error& e) {
            thrown = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(thrown, "dst = cur is refused with DIS_ERR_INVALID_ARGUMENT");
        thrown = false;
        try {
            dis::denoiseWeights(0.0f);
        } catch (const dis::Error& e) {
            thrown = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(thrown, "sigma = 0 is refused with DIS_ERR_INVALID_ARGUMENT");
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
