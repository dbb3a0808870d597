// C++ test of the facade's bidirectional call (include/dis/dis.hpp):
// calc(I0, I1, fw, bw) against two plain calc calls, byte for byte, and
// dis::flowConsistency on the result. Compiled and run on a GPU box by
// tests/test_gpu_bidir.py; exits non-zero on any failure.
#include <cstdio>
#include <cstring>
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

int main()
{
    const int W = 160, H = 120;
    const size_t px = (size_t)W * H;
    std::vector<uint8_t> I0(px), I1(px);
    dis::check(dis_synth_pair(7, W, H, I0.data(), I1.data(), nullptr));
    try {
        dis::DenseInverseSearch eng(dis::Preset::MEDIUM, W, H);
        std::vector<float> f01(px * 2), f10(px * 2), fw(px * 2), bw(px * 2);
        eng.calc(I0.data(), I1.data(), f01.data());
        eng.calc(I1.data(), I0.data(), f10.data());
        eng.calc(I0.data(), I1.data(), fw.data(), bw.data());
        EXPECT(std::memcmp(fw.data(), f01.data(), px * 2 * sizeof(float)) == 0, "forward flow == calc(I0, I1)");
        EXPECT(std::memcmp(bw.data(), f10.data(), px * 2 * sizeof(float)) == 0, "backward flow == calc(I1, I0)");
        EXPECT(std::memcmp(fw.data(), bw.data(), px * 2 * sizeof(float)) != 0, "the two directions differ");
        // a plain call after the bidirectional one is unchanged
        std::vector<float> again(px * 2);
        eng.calc(I0.data(), I1.data(), again.data());
        EXPECT(std::memcmp(again.data(), f01.data(), px * 2 * sizeof(float)) == 0, "calc after bidir unchanged");

        std::vector<uint8_t> mask(px, 7);
        std::vector<float> err(px);
        dis::flowConsistency(fw.data(), bw.data(), 1, W, H, mask.data(), err.data());
        size_t good = 0, other = 0;
        for (size_t i = 0; i < px; ++i) {
            good += mask[i] == 255;
            other += mask[i] != 255 && mask[i] != 0;
        }
        EXPECT(other == 0, "mask bytes are 0 or 255");
        EXPECT(good > 0 && good < px, "both mask values occur");
        bool thrown = false;
        try {
            eng.calc(I0.data(), I1.data(), fw.data(), fw.data());
        } catch (const dis::Error& e) {
            thrown = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        EXPECT(thrown, "overlapping outputs are refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
