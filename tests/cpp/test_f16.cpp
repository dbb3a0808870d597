// C++ test of the facade's f16 flow format (include/dis/dis.hpp):
// set_flow_format + calc(half_bits*) against the oracle's flow narrowed on the
// host (round to nearest even, written out below), dis::flowConvert both ways,
// and the exceptions of a flow pointer whose type does not match the engine's
// format. Compiled and run on a GPU box by tests/test_gpu_f16.py, which passes
// the oracle's float flow of the MEDIUM preset on dis_synth_pair(7, 160, 120)
// as a raw file; exits non-zero on any failure.
#include <cmath>
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

// IEEE binary32 -> binary16, round to nearest, ties to even; subnormals kept;
// overflow to infinity; NaN to a quiet NaN
static uint16_t narrow_rne(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    const uint32_t e = (x >> 23) & 0xffu, m = x & 0x7fffffu;
    if (e == 0xff) return (uint16_t)(sign | 0x7c00u | (m ? 0x200u | (m >> 13) : 0u));
    const int E = (int)e - 127 + 15;  // the half's biased exponent
    if (E >= 31) return (uint16_t)(sign | 0x7c00u);
    uint32_t mant, shift;
    uint16_t base;
    if (E <= 0) {  // subnormal half (or zero): the implicit bit joins the mantissa
        if (E < -10) return sign;  // below half of the smallest subnormal
        mant = m | 0x800000u;
        shift = (uint32_t)(14 - E);
        base = sign;
    } else {
        mant = m;
        shift = 13;
        base = (uint16_t)(sign | (E << 10));
    }
    const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1), half = 1u << (shift - 1);
    // (a carry out of the mantissa moves into the exponent, up to infinity: the encoding is monotone)
    return (uint16_t)(base + q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0));
}

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

int main(int argc, char** argv)
{
    const int W = 160, H = 120;
    const size_t px = (size_t)W * H;
    if (argc < 2) {
        std::printf("usage: test_f16 <oracle flow, %zu raw floats>\n", px * 2);
        return 2;
    }
    std::vector<float> ora(px * 2);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(ora.data(), sizeof(float), px * 2, fp) != px * 2) {
        std::printf("FAIL: cannot read %s\n", argv[1]);
        return 2;
    }
    std::fclose(fp);
    std::vector<uint8_t> I0(px), I1(px);
    dis::check(dis_synth_pair(7, W, H, I0.data(), I1.data(), nullptr));
    try {
        dis::DenseInverseSearch eng(dis::Preset::MEDIUM, W, H);
        std::vector<float> f32(px * 2);
        eng.calc(I0.data(), I1.data(), f32.data());
        EXPECT(std::memcmp(f32.data(), ora.data(), px * 2 * sizeof(float)) == 0, "F32 flow == oracle");

        EXPECT(eng.flow_format() == dis::FlowFormat::F32, "F32 is the default");
        std::vector<dis::half_bits> h(px * 2, 0x7e00), exp(px * 2);
        EXPECT(throws_invalid([&] { eng.calc(I0.data(), I1.data(), h.data()); }), "half_bits flow on an F32 engine throws");
        eng.set_flow_format(dis::FlowFormat::F16);
        EXPECT(eng.flow_format() == dis::FlowFormat::F16, "format is F16 after set_flow_format");
        EXPECT(throws_invalid([&] { eng.calc(I0.data(), I1.data(), f32.data()); }), "float flow on an F16 engine throws");
        EXPECT(throws_invalid([&] { eng.calc(I0.data(), I1.data(), f32.data(), f32.data() + px); }),
               "float bidirectional flows on an F16 engine throw");
        EXPECT(throws_invalid([&] { eng.calc_batch(1, I0.data(), I1.data(), f32.data()); }),
               "float batch flow on an F16 engine throws");
        EXPECT(throws_invalid([&] { eng.set_flow_format(static_cast<dis::FlowFormat>(2)); }), "format 2 is refused");
        EXPECT(eng.flow_format() == dis::FlowFormat::F16, "a refused format changes nothing");

        eng.calc(I0.data(), I1.data(), h.data());
        bool nonzero = false;
        for (size_t i = 0; i < px * 2; ++i) {
            exp[i] = narrow_rne(ora[i]);
            nonzero |= (exp[i] & 0x7fff) != 0;
        }
        EXPECT(nonzero, "the oracle flow is not all zero");
        EXPECT(std::memcmp(h.data(), exp.data(), px * 2 * sizeof(dis::half_bits)) == 0, "F16 flow == narrow(oracle)");

        // flowConvert: the engine's narrowing of its own F32 flow, and back
        std::vector<dis::half_bits> conv(px * 2);
        dis::flowConvert(f32.data(), dis::FlowFormat::F32, conv.data(), dis::FlowFormat::F16, px * 2);
        EXPECT(std::memcmp(conv.data(), exp.data(), px * 2 * sizeof(dis::half_bits)) == 0, "flowConvert F32 -> F16");
        std::vector<float> wide(px * 2), back(px * 2);
        dis::flowConvert(h.data(), dis::FlowFormat::F16, wide.data(), dis::FlowFormat::F32, px * 2);
        dis::flowConvert(wide.data(), dis::FlowFormat::F32, conv.data(), dis::FlowFormat::F16, px * 2);
        EXPECT(std::memcmp(conv.data(), h.data(), px * 2 * sizeof(dis::half_bits)) == 0, "F16 -> F32 -> F16 round trip");
        bool close = true;
        for (size_t i = 0; i < px * 2; ++i)  // half an f16 ulp at |v| < 64 is 2^-6
            close &= std::fabs(wide[i] - ora[i]) <= 0.015625f || std::fabs(ora[i]) >= 64.0f;
        EXPECT(close, "widened F16 flow within half an ulp of the oracle");
        dis::flowConvert(wide.data(), dis::FlowFormat::F32, back.data(), dis::FlowFormat::F32, px * 2);
        EXPECT(std::memcmp(back.data(), wide.data(), px * 2 * sizeof(float)) == 0, "equal formats copy");
        EXPECT(throws_invalid([&] {
                   dis::flowConvert(wide.data(), static_cast<dis::FlowFormat>(5), back.data(), dis::FlowFormat::F32, 4);
               }),
               "flowConvert refuses a bad format");

        // back to F32: the float overloads work again, bit for bit
        eng.set_flow_format(dis::FlowFormat::F32);
        std::vector<float> again(px * 2);
        eng.calc(I0.data(), I1.data(), again.data());
        EXPECT(std::memcmp(again.data(), ora.data(), px * 2 * sizeof(float)) == 0, "F32 flow after F16 == oracle");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
