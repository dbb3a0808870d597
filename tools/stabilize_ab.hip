// stabilize_ab.hip -- the staged form of dis_warp_motion_u8's kernel against its
// direct form (csrc/dis_warpmotion.hip, launch_warp_motion's direct_only), in
// one process: the A/B DESIGN.md 3m quotes (tools/stabilize_probe.py runs this
// program and keeps its JSON line).
//
//   hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -ffp-contract=off -std=c++17 \
//       -Iinclude -Ioptical-flow-using-dense-inverse-search_amd/csrc tools/stabilize_ab.hip -o tools/stabilize_ab
//   tools/stabilize_ab [images=64] [rounds=12] [launches=10] [width=1920] [height=1080]
//   tools/stabilize_ab routes W H C border p0 p1 p2 p3 p4 p5
//
// The second form (tests/test_gpu_stabilize.py) launches the library's choice of
// kernel once on one W x H image of C channels under the model p, with the
// kernel's route counters, and prints "routes <staged blocks> <direct blocks>
// <pixels of staged blocks that read global memory>": what tests/stabref.py's
// routes() restates.
//
// `images` device-resident frames of random bytes, each under its own small
// rotation (0.6 degrees, scale 1.01, about the centre, plus a translation that
// differs per image): the model of a stabiliser's correction. With 3 channels
// (the only ones the library stages): both forms warmed up, their outputs
// compared byte for byte, then `rounds` rounds that alternate the two forms,
// each timed over `launches` launches between two events. Reported per form: the
// per-launch times of the rounds (median, min, max); "gain" = direct median / staged median; "spread" =
// the larger of the two forms' (max - min) / median.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../optical-flow-using-dense-inverse-search_amd/csrc/dis_warpmotion.hip"

#define CHECK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            std::fprintf(stderr, "%s: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

static int routes_mode(int argc, char** argv)
{
    if (argc != 12) {
        std::fprintf(stderr, "usage: stabilize_ab routes W H C border p0 p1 p2 p3 p4 p5\n");
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), C = std::atoi(argv[4]), border = std::atoi(argv[5]);
    if (dis::warp_motion_blocks(1, W, H) < 1 || (C != 1 && C != 3 && C != 4) || (size_t)W * H > (size_t(1) << 24)) {
        std::fprintf(stderr, "stabilize_ab: bad arguments\n");
        return 2;
    }
    float p[6];
    for (int e = 0; e < 6; ++e) p[e] = std::strtof(argv[6 + e], nullptr);
    const size_t px = (size_t)W * H;
    std::vector<uint8_t> host(px * C);
    std::mt19937 rng(11);
    for (uint8_t& b : host) b = (uint8_t)rng();
    uint8_t *dsrc = nullptr, *ddst = nullptr, *dvalid = nullptr;
    float* dpar = nullptr;
    unsigned* dcnt = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dsrc), px * C));
    CHECK(hipMalloc(reinterpret_cast<void**>(&ddst), px * C));
    CHECK(hipMalloc(reinterpret_cast<void**>(&dvalid), px));
    CHECK(hipMalloc(reinterpret_cast<void**>(&dpar), sizeof p));
    CHECK(hipMalloc(reinterpret_cast<void**>(&dcnt), 3 * sizeof(unsigned)));
    CHECK(hipMemcpy(dsrc, host.data(), px * C, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dpar, p, sizeof p, hipMemcpyHostToDevice));
    CHECK(hipMemset(dcnt, 0, 3 * sizeof(unsigned)));
    CHECK(dis::launch_warp_motion(dsrc, (size_t)W * C, (size_t)W * C * H, C, dpar, 1, W, H, border, ddst, dvalid, nullptr,
                                  dis::Timing{}, 0, dcnt));
    CHECK(hipDeviceSynchronize());
    unsigned cnt[3];
    CHECK(hipMemcpy(cnt, dcnt, sizeof cnt, hipMemcpyDeviceToHost));
    std::printf("routes %u %u %u\n", cnt[0], cnt[1], cnt[2]);
    CHECK(hipFree(dsrc));
    CHECK(hipFree(ddst));
    CHECK(hipFree(dvalid));
    CHECK(hipFree(dpar));
    CHECK(hipFree(dcnt));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "routes") return routes_mode(argc, argv);
    const int n = argc > 1 ? std::atoi(argv[1]) : 64, rounds = argc > 2 ? std::atoi(argv[2]) : 12;
    const int launches = argc > 3 ? std::atoi(argv[3]) : 10;
    const int W = argc > 4 ? std::atoi(argv[4]) : 1920, H = argc > 5 ? std::atoi(argv[5]) : 1080;
    if (n < 1 || rounds < 2 || launches < 1 || dis::warp_motion_blocks(n, W, H) < 1) {
        std::fprintf(stderr, "stabilize_ab: bad arguments\n");
        return 2;
    }
    const size_t px = (size_t)n * W * H;
    std::vector<float> params((size_t)n * 6);
    const double c = 1.01 * std::cos(0.6 * M_PI / 180.0), s = 1.01 * std::sin(0.6 * M_PI / 180.0);
    const double cx = (W - 1) / 2.0, cy = (H - 1) / 2.0;
    for (int i = 0; i < n; ++i) {
        const double tx = 3.0 * std::sin(1.0 + i), ty = 3.0 * std::cos(2.0 + 0.7 * i);
        const double q[6] = {cx - (c * cx - s * cy) + tx, c - 1.0, -s, cy - (s * cx + c * cy) + ty, s, c - 1.0};
        for (int e = 0; e < 6; ++e) params[(size_t)i * 6 + e] = (float)q[e];
    }
    float* dpar = nullptr;
    uint8_t *dvalid = nullptr, *dvalid2 = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dpar), params.size() * sizeof(float)));
    CHECK(hipMemcpy(dpar, params.data(), params.size() * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMalloc(reinterpret_cast<void**>(&dvalid), px));
    CHECK(hipMalloc(reinterpret_cast<void**>(&dvalid2), px));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::string json = "{\"probe\": \"stabilize_ab\", \"images\": " + std::to_string(n) + ", \"width\": " + std::to_string(W) +
                       ", \"height\": " + std::to_string(H) + ", \"rounds\": " + std::to_string(rounds) +
                       ", \"launches_per_round\": " + std::to_string(launches) +
                       ", \"model\": \"rotation 0.6 deg, scale 1.01, translation within 3 px\", \"cases\": {";
    for (int C : {3}) {
        std::vector<uint8_t> host(px * C);
        std::mt19937 rng(7 + C);
        for (size_t i = 0; i < host.size(); i += 4) {
            const uint32_t r = rng();
            for (size_t k = 0; k < 4 && i + k < host.size(); ++k) host[i + k] = (uint8_t)(r >> (8 * k));
        }
        uint8_t *dsrc = nullptr, *da = nullptr, *db = nullptr;
        CHECK(hipMalloc(reinterpret_cast<void**>(&dsrc), px * C));
        CHECK(hipMalloc(reinterpret_cast<void**>(&da), px * C));
        CHECK(hipMalloc(reinterpret_cast<void**>(&db), px * C));
        CHECK(hipMemcpy(dsrc, host.data(), px * C, hipMemcpyHostToDevice));
        auto run = [&](int direct, uint8_t* dst, uint8_t* valid) {
            return dis::launch_warp_motion(dsrc, (size_t)W * C, (size_t)W * C * H, C, dpar, n, W, H, 0, dst, valid, nullptr,
                                           dis::Timing{}, direct);
        };
        for (int k = 0; k < 3; ++k) {  // warm-up, and the outputs to compare
            CHECK(run(0, da, dvalid));
            CHECK(run(1, db, dvalid2));
        }
        CHECK(hipDeviceSynchronize());
        std::vector<uint8_t> a(px * C), b(px * C), va(px), vb(px);
        CHECK(hipMemcpy(a.data(), da, px * C, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(b.data(), db, px * C, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(va.data(), dvalid, px, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(vb.data(), dvalid2, px, hipMemcpyDeviceToHost));
        const bool same = a == b && va == vb;
        size_t inside = 0;
        for (uint8_t v : va) inside += v == 255;
        std::vector<double> t[2];
        for (int r = 0; r < rounds; ++r)
            for (int direct = 0; direct < 2; ++direct) {
                CHECK(hipEventRecord(e0, nullptr));
                for (int k = 0; k < launches; ++k) CHECK(run(direct, direct ? db : da, direct ? dvalid2 : dvalid));
                CHECK(hipEventRecord(e1, nullptr));
                CHECK(hipEventSynchronize(e1));
                float ms = 0.0f;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                t[direct].push_back((double)ms / launches);
            }
        double med[2], lo[2], hi[2];
        for (int d = 0; d < 2; ++d) {
            med[d] = median(t[d]);
            lo[d] = *std::min_element(t[d].begin(), t[d].end());
            hi[d] = *std::max_element(t[d].begin(), t[d].end());
        }
        const double spread = std::max((hi[0] - lo[0]) / med[0], (hi[1] - lo[1]) / med[1]);
        char buf[512];
        std::snprintf(buf, sizeof buf,
                      "%s\"c%d\": {\"same_bytes\": %s, \"valid_fraction\": %.4f, \"staged_ms\": {\"median\": %.4f, \"min\": %.4f, "
                      "\"max\": %.4f}, \"direct_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"gain\": %.4f, "
                      "\"spread\": %.4f}",
                      "", C, same ? "true" : "false", (double)inside / (double)px, med[0], lo[0], hi[0], med[1],
                      lo[1], hi[1], med[1] / med[0], spread);
        json += buf;
        CHECK(hipFree(dsrc));
        CHECK(hipFree(da));
        CHECK(hipFree(db));
        if (!same) {
            std::fprintf(stderr, "stabilize_ab: the two forms differ at %d channels\n", C);
            std::printf("%s}}\n", json.c_str());
            return 1;
        }
    }
    std::printf("%s}}\n", json.c_str());
    CHECK(hipFree(dpar));
    CHECK(hipFree(dvalid));
    CHECK(hipFree(dvalid2));
    return 0;
}
