// args_motion_host.cpp -- the argument rules of dis_flow_fit_motion and
// dis_motion_to_flow (csrc/dis_args.h): the chunk count (motion_chunks), the
// workspace size at its edges (check_motion_workspace), the grid limits
// (motion_blocks, motion_flow_blocks) and the overlap rule over the six ranges
// of the entry point. Built with -fsanitize=address,undefined by
// tests/cpp/motion.mk (target args_motion) and run by tests/test_motion_host.py.
// Nothing is dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "dis_args.h"
#include "far_cases.h"

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++failures;
    }
}

static size_t ws(int n, int w, int h)
{
    size_t b = 7;
    return dis::check_motion_workspace(n, w, h, &b) ? (size_t)-1 : b;
}

// dis_flow_fit_motion's six ranges: flow, mask | params, info, inliers, workspace.
struct Fit {
    uintptr_t flow, mask, params, info, inliers, ws;
    size_t px, fsz, n, ws_bytes;
    bool has_mask, has_info, has_inliers;
};
static dis::PairMessage g_why;
static const char* rule(const Fit& c)
{
    const dis::NamedRange r[6] = {{c.flow, c.px * c.fsz, "flow"}, {c.mask, c.has_mask ? c.px : 0, "mask"},
                                  {c.params, 24 * c.n, "params"}, {c.info, c.has_info ? 16 * c.n : 0, "info"},
                                  {c.inliers, c.has_inliers ? c.px : 0, "inliers"}, {c.ws, c.ws_bytes, "workspace"}};
    return dis::check_disjoint(r, 2, 6, &g_why);
}
static Fit plain()
{
    // two fields of 50 pixels, f32: 800 bytes of flow, planes of 100, 48 of params, 32 of info, a workspace of 448
    return {0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 100, 8, 2, 448, true, true, true};
}

int main()
{
    {  // the chunks
        expect(dis::motion_chunks(1, 1) == 1 && dis::motion_chunks(5, 3) == 1, "a small field is one chunk");
        expect(dis::motion_chunks(256, 64) == 1 && dis::motion_chunks(257, 64) == 2, "16384 pixels fill a chunk");
        expect(dis::motion_chunks(160, 120) == 2 && dis::motion_chunks(1920, 1080) == 127, "hand-counted sizes");
        expect(dis::motion_chunks(dis::kMaxExactSide, 128) == 131072, "2^31 pixels: 2^17 chunks");
    }
    {  // the workspace
        expect(ws(1, 1, 1) == 224 && ws(3, 5, 3) == 3 * 224, "(12 + 16) doubles a field of one chunk");
        expect(ws(1, 257, 64) == (2 * 12 + 16) * 8 && ws(2, 160, 120) == 2 * 320, "two chunks");
        expect(ws(32, 1920, 1080) == 32u * (127 * 12 + 16) * 8, "32 fields of 1080p: 394,240 bytes");
        expect(ws(1, dis::kMaxExactSide, 128) == (size_t(131072) * 12 + 16) * 8, "the largest field");
        expect(ws(16383, dis::kMaxExactSide, 128) == size_t(16383) * (size_t(131072) * 12 + 16) * 8,
               "the most of the largest fields a grid holds");
        size_t b = 7;
        expect(dis::check_motion_workspace(16384, dis::kMaxExactSide, 128, &b) != nullptr && b == 7, "one field more");
        expect(dis::check_motion_workspace(1, dis::kMaxExactSide, 129, &b) != nullptr, "more than 2^31 pixels");
        expect(dis::check_motion_workspace(1, 65536, 32768, &b) == nullptr, "exactly 2^31 pixels");
        expect(dis::check_motion_workspace(1, 65536, 32769, &b) != nullptr, "2^31 pixels and a row");
        expect(dis::check_motion_workspace(1, dis::kMaxExactSide + 1, 1, &b) != nullptr, "a side above 2^24");
        expect(dis::check_motion_workspace(1, 1, dis::kMaxExactSide + 1, &b) != nullptr, "the other side above 2^24");
        expect(dis::check_motion_workspace(0, 4, 4, &b) != nullptr && dis::check_motion_workspace(1, 0, 4, &b) != nullptr &&
                   dis::check_motion_workspace(1, 4, 0, &b) != nullptr && dis::check_motion_workspace(-1, 4, 4, &b) != nullptr,
               "n, width, height below 1");
        expect(dis::check_motion_workspace(INT32_MAX, 1, 1, &b) == nullptr && b == size_t(INT32_MAX) * 224,
               "2^31 - 1 fields of one pixel");
        expect(dis::check_motion_workspace(INT32_MAX, 129, 127, &b) == nullptr, "2^31 - 1 fields of 16383 pixels");
        expect(dis::check_motion_workspace(INT32_MAX, 129, 128, &b) != nullptr, "2^31 - 1 fields of two chunks");
    }
    {  // the grids
        expect(dis::motion_blocks(1, 1, 1) == 1 && dis::motion_blocks(32, 1920, 1080) == 32 * 127, "a block per chunk");
        expect(dis::motion_blocks(16383, dis::kMaxExactSide, 128) == 16383ll * 131072, "below the limit");
        expect(dis::motion_blocks(16384, dis::kMaxExactSide, 128) == -1, "2^31 blocks");
        expect(dis::motion_blocks(0, 4, 4) == -1 && dis::motion_blocks(-2, 4, 4) == -1, "no fields");
        expect(dis::motion_flow_blocks(1, 1, 1) == 1 && dis::motion_flow_blocks(1, 1024, 1) == 1 &&
                   dis::motion_flow_blocks(1, 1025, 1) == 2, "256 lanes of four pixels");
        expect(dis::motion_flow_blocks(2, 67, 33) == (2 * 33 * 17 + 255) / 256, "a row's last lane is partial");
        expect(dis::motion_flow_blocks(INT32_MAX, 1, 256) == INT32_MAX, "one-pixel rows: the limit");
        expect(dis::motion_flow_blocks(INT32_MAX, 1, 257) == -1, "and past it");
        expect(dis::motion_flow_blocks(INT32_MAX, dis::kMaxExactSide, dis::kMaxExactSide) == -1, "no overflow on the way");
        expect(dis::motion_flow_blocks(0, 4, 4) == -1, "no fields");
        expect(dis::check_motion_flow(INT32_MAX, 1, 257) != nullptr && dis::check_motion_flow(INT32_MAX, 1, 256) == nullptr,
               "dis_motion_to_flow's sizes: its own grid");
        expect(dis::check_motion_flow(1, 65536, 32769) != nullptr && dis::check_motion_flow(1, dis::kMaxExactSide + 1, 1) != nullptr &&
                   dis::check_motion_flow(0, 1, 1) != nullptr && dis::check_motion_flow(1, 65536, 32768) == nullptr,
               "dis_motion_to_flow's sizes: the sides and the pixels");
    }
    {  // the overlap rule
        expect(rule(plain()) == nullptr, "all apart");
        Fit c = plain();
        c.params = c.flow + 800;
        expect(rule(c) == nullptr, "params right after flow");
        c.params = c.flow + 799;
        expect(rule(c) != nullptr && std::strstr(g_why.text, "params") && std::strstr(g_why.text, "flow"), "params on flow's last byte");
        c = plain();
        c.params = c.flow - 47;
        expect(rule(c) != nullptr, "params ends in flow");
        c = plain();
        c.info = c.mask + 99;
        expect(rule(c) != nullptr && std::strstr(g_why.text, "info") && std::strstr(g_why.text, "mask"), "info on mask's last byte");
        c.has_info = false;
        expect(rule(c) == nullptr, "an absent info takes no part");
        c = plain();
        c.inliers = c.mask;
        expect(rule(c) != nullptr, "inliers is mask");
        c.has_mask = false;
        expect(rule(c) == nullptr, "an absent mask takes no part");
        c = plain();
        c.inliers = c.flow + 400;
        expect(rule(c) != nullptr, "inliers inside flow");
        c.fsz = 4;  // f16: flow ends where inliers begins
        expect(rule(c) == nullptr, "inliers after an f16 flow");
        c = plain();
        c.info = c.params + 47;
        expect(rule(c) != nullptr && std::strstr(g_why.text, "params") && std::strstr(g_why.text, "info"), "info on params' last byte");
        c.info = c.params + 48;
        expect(rule(c) == nullptr, "info right after params");
        c = plain();
        c.inliers = c.info - 99;
        expect(rule(c) != nullptr, "inliers ends in info");
        c = plain();
        c.ws = c.params + 8;
        expect(rule(c) != nullptr && std::strstr(g_why.text, "workspace"), "workspace in params");
        c.ws = c.flow - 440;
        expect(rule(c) != nullptr, "workspace ends in flow");
        c.ws = c.inliers + 96;
        expect(rule(c) != nullptr, "workspace begins in inliers");
        c.ws_bytes = 0;  // a host call
        expect(rule(c) == nullptr, "a host call's workspace takes no part");
        c = plain();
        c.flow = UINTPTR_MAX - 799;  // the last 800 bytes of the address space
        c.params = UINTPTR_MAX - 47;
        expect(rule(c) != nullptr, "no wrap at the top of the address space");
    }
    far::motion(12, &failures);  // the far cases (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
