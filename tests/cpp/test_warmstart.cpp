// test_warmstart.cpp -- the C++ facade's warm-start overload
// (dis::DenseInverseSearch::calc(I0, I1, flow, init, dis::InitKind),
// initPlaneSize) against numbers tests/test_gpu_warmstart.py computed with the
// oracle: the oracle's C = 2 run equals a C = 1 engine started from the
// oracle's level-2 dense flow. Built by that test's own compile line.
//
// argv[1]: int32 W, H, iw, ih, iterations; u8 I0, I1 (W * H each); float
// plane (iw * ih * 2); float expected flow (W * H * 2).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dis/dis.hpp"

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[5];
    if (std::fread(h, sizeof(int32_t), 5, f) != 5) return 2;
    const int W = h[0], H = h[1], iw = h[2], ih = h[3], it = h[4];
    std::vector<uint8_t> I0, I1;
    std::vector<float> plane, expect;
    if (!read_n(f, I0, (size_t)W * H) || !read_n(f, I1, (size_t)W * H) || !read_n(f, plane, (size_t)iw * ih * 2) ||
        !read_n(f, expect, (size_t)W * H * 2))
        return 2;
    std::fclose(f);
    try {
        dis_params p{};
        p.coarsest_scale = 1;
        p.finest_scale = 0;
        p.patch_size = 8;
        p.iterations = it;
        p.patch_overlap = 0.5f;
        p.patch_normalization = 1;
        dis::DenseInverseSearch eng(p, W, H);
        const auto sz = eng.initPlaneSize();
        if (sz.first != iw || sz.second != ih) {
            std::printf("initPlaneSize %d x %d, expected %d x %d\n", sz.first, sz.second, iw, ih);
            return 1;
        }
        std::vector<float> flow((size_t)W * H * 2), plain(flow.size()), null_init(flow.size());
        eng.calc(I0.data(), I1.data(), flow.data(), plane.data(), dis::InitKind::COARSE);
        if (std::memcmp(flow.data(), expect.data(), flow.size() * sizeof(float)) != 0) {
            std::printf("warm-started flow differs from the oracle's split run\n");
            return 1;
        }
        // init == nullptr is the plain call
        eng.calc(I0.data(), I1.data(), plain.data());
        eng.calc(I0.data(), I1.data(), null_init.data(), nullptr, dis::InitKind::FULLRES);
        if (std::memcmp(plain.data(), null_init.data(), plain.size() * sizeof(float)) != 0) {
            std::printf("null init differs from the plain call\n");
            return 1;
        }
        // flow in, flow out: the full-resolution form with init == flow
        std::vector<float> sep(flow.size()), inout(plain);
        eng.calc(I0.data(), I1.data(), sep.data(), plain.data(), dis::InitKind::FULLRES);
        eng.calc(I0.data(), I1.data(), inout.data(), inout.data(), dis::InitKind::FULLRES);
        if (std::memcmp(sep.data(), inout.data(), sep.size() * sizeof(float)) != 0) {
            std::printf("init == flow differs from separate buffers\n");
            return 1;
        }
        // a refused call throws dis::Error with the status
        bool threw = false;
        try {
            eng.calc(I0.data(), I1.data(), inout.data(), inout.data() + 2, dis::InitKind::FULLRES);
        } catch (const dis::Error& e) {
            threw = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        if (!threw) {
            std::printf("partial overlap was not refused\n");
            return 1;
        }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("facade warm start ok\n");
    return 0;
}
