// C++ test of the facade's colour frame input (include/dis/dis.hpp):
// dis::framesToGray against the formula written out below, set_frame_format +
// the unchanged calc overloads on BGR and RGBA frames against a gray engine on
// the reduced frames, the vector overload's size check, and a refused format.
// Compiled and run on a GPU box by tests/test_gpu_color.py; exits non-zero on
// any failure.
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

template <class F>
static bool throws_invalid(F&& f)
{
    try {
        f();
    } catch (const dis::Error& e) {
        return e.status() == DIS_ERR_INVALID_ARGUMENT;
    }
    return false;
}

static uint8_t luma(unsigned r, unsigned g, unsigned b) { return (uint8_t)((r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14); }

// colour frames whose channels differ: the gray pixel plus a per-channel pattern
static std::vector<uint8_t> colourise(const std::vector<uint8_t>& gray, int C, unsigned seed)
{
    std::vector<uint8_t> out(gray.size() * C);
    unsigned s = seed;
    for (size_t i = 0; i < gray.size(); ++i)
        for (int c = 0; c < C; ++c) {
            s = s * 1664525u + 1013904223u;
            const int v = (int)gray[i] + (int)((s >> 24) % 81) - 40;
            out[i * C + c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
    return out;
}

int main()
{
    const int W = 101, H = 67;  // pads on both axes, W no multiple of 16
    const size_t px = (size_t)W * H;
    std::vector<uint8_t> G0(px), G1(px);
    dis::check(dis_synth_pair(9, W, H, G0.data(), G1.data(), nullptr));
    try {
        dis::DenseInverseSearch gray(dis::Preset::MEDIUM, W, H), eng(dis::Preset::MEDIUM, W, H);
        EXPECT(eng.frame_format() == dis::FrameFormat::GRAY8, "GRAY8 is the default");
        for (int C = 3; C <= 4; ++C) {
            const dis::FrameFormat fmt = C == 3 ? dis::FrameFormat::BGR8 : dis::FrameFormat::RGBA8;
            const std::vector<uint8_t> C0 = colourise(G0, C, 1), C1 = colourise(G1, C, 2);
            // framesToGray: two frames in one call, against the formula
            std::vector<uint8_t> both(C0), red(2 * px), want(2 * px);
            both.insert(both.end(), C1.begin(), C1.end());
            dis::framesToGray(both.data(), fmt, 2, W, H, red.data());
            for (size_t i = 0; i < 2 * px; ++i) {
                const uint8_t* p = &both[i * C];
                want[i] = C == 3 ? luma(p[2], p[1], p[0]) : luma(p[0], p[1], p[2]);
            }
            EXPECT(std::memcmp(red.data(), want.data(), 2 * px) == 0, "framesToGray == the formula");
            EXPECT(std::memcmp(red.data(), G0.data(), px) != 0, "the reduced frame is not the gray frame it was made from");
            // the colour engine on the colour frames == the gray engine on the reduced frames
            std::vector<float> exp(px * 2), got(px * 2), fw(px * 2), bw(px * 2), efw(px * 2), ebw(px * 2);
            gray.calc(red.data(), red.data() + px, exp.data());
            eng.set_frame_format(fmt);
            EXPECT(eng.frame_format() == fmt && dis::channels(fmt) == C, "the format is set");
            eng.calc(C0.data(), C1.data(), got.data());
            EXPECT(std::memcmp(got.data(), exp.data(), px * 2 * sizeof(float)) == 0, "colour calc == gray calc");
            EXPECT(eng.calc(C0, C1) == got, "the vector overload takes W*H*channels bytes");
            EXPECT(throws_invalid([&] { eng.calc(G0, G1); }), "the vector overload refuses gray-sized frames");
            gray.calc(red.data(), red.data() + px, efw.data(), ebw.data());
            eng.calc(C0.data(), C1.data(), fw.data(), bw.data());
            EXPECT(std::memcmp(fw.data(), efw.data(), px * 2 * sizeof(float)) == 0 &&
                       std::memcmp(bw.data(), ebw.data(), px * 2 * sizeof(float)) == 0,
                   "bidirectional colour calc == gray calc");
            EXPECT(throws_invalid([&] { eng.calc(C0.data(), C1.data(), got.data(), (size_t)W * C - 1); }),
                   "a stride smaller than a colour row is refused");
        }
        EXPECT(throws_invalid([&] { eng.set_frame_format(static_cast<dis::FrameFormat>(5)); }), "format 5 is refused");
        EXPECT(eng.frame_format() == dis::FrameFormat::RGBA8, "a refused format changes nothing");
        // back to gray: the gray frames again, bit for bit
        eng.set_frame_format(dis::FrameFormat::GRAY8);
        std::vector<float> a(px * 2), b(px * 2);
        eng.calc(G0.data(), G1.data(), a.data());
        gray.calc(G0.data(), G1.data(), b.data());
        EXPECT(std::memcmp(a.data(), b.data(), px * 2 * sizeof(float)) == 0, "gray after colour == a gray engine");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
