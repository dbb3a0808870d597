// args_fill_host.cpp -- the argument rules of dis_flow_fill (csrc/dis_args.h):
// the levels and the workspace size (fill_levels, check_fill_workspace) at
// hand-counted sizes and at the largest sides, the grid limit
// (fill_tile_blocks), and the aliasing rule with its one allowed pair (out ==
// flow) over the five ranges of the entry point. Built with
// -fsanitize=address,undefined by tests/cpp/fill.mk (target args_fill) and run
// by tests/test_fill_host.py. Nothing is dereferenced.
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

static size_t cells(int w, int h)
{
    dis::FillLevels g;
    dis::fill_levels(w, h, &g);
    return g.cells;
}

// dis_flow_fill's five ranges: flow, mask | out, level, workspace.
struct Fill {
    uintptr_t flow, mask, out, level, ws;
    size_t px, fsz, osz, ws_bytes;
    bool has_mask, has_level;
};
static dis::PairMessage g_why;
static const char* rule(const Fill& c)
{
    const dis::NamedRange r[5] = {{c.flow, c.px * c.fsz, "flow"}, {c.mask, c.has_mask ? c.px : 0, "mask"},
                                  {c.out, c.px * c.osz, "out"}, {c.level, c.has_level ? c.px : 0, "level"},
                                  {c.ws, c.ws_bytes, "workspace"}};
    const dis::MayAlias may[1] = {{2, 0}};
    return dis::check_disjoint_or_same(r, 2, 5, may, c.fsz == c.osz ? 1 : 0, &g_why);
}
static Fill plain()
{
    // 100 pixels, f32 in and out: fields of 800 bytes, planes of 100, a workspace of 400, all apart
    return {0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 100, 8, 8, 400, true, true};
}

int main()
{
    {  // the levels
        dis::FillLevels g;
        dis::fill_levels(1, 1, &g);
        expect(g.L == 0 && g.cells == 0, "1 x 1: no level above the field");
        dis::fill_levels(2, 1, &g);
        expect(g.L == 1 && g.cells == 1 && g.w[1] == 1 && g.h[1] == 1 && g.off[1] == 0, "2 x 1");
        dis::fill_levels(3, 5, &g);  // 2 x 3, 1 x 2, 1 x 1
        expect(g.L == 3 && g.cells == 9 && g.w[1] == 2 && g.h[1] == 3 && g.w[2] == 1 && g.h[2] == 2, "3 x 5");
        expect(g.off[1] == 0 && g.off[2] == 6 && g.off[3] == 8, "3 x 5: where the levels begin");
        expect(cells(67, 33) == 800 && cells(160, 120) == 6409 && cells(1920, 1080) == 691302, "hand-counted sizes");
        dis::fill_levels(1920, 1080, &g);
        expect(g.L == 11 && g.w[5] == 60 && g.h[5] == 34, "1080p: L = 11");
        dis::fill_levels(dis::kMaxExactSide, dis::kMaxExactSide, &g);
        expect(g.L == 24 && g.L < dis::kMaxFillLevels && g.w[24] == 1 && g.h[24] == 1, "2^24 squared: L = 24");
        expect(g.cells == ((size_t(1) << 48) - 1) / 3, "2^24 squared: (4^24 - 1) / 3 cells");
        dis::fill_levels(dis::kMaxExactSide, 1, &g);
        expect(g.L == 24 && g.cells == (size_t(1) << 24) - 1, "2^24 x 1");
        dis::fill_levels(1, dis::kMaxExactSide - 1, &g);
        expect(g.L == 24 && g.h[1] == (1 << 23) && g.w[1] == 1, "1 x 2^24 - 1");
    }
    {  // the workspace size and the refusals that need no device
        size_t b = 77;
        expect(!dis::check_fill_workspace(1, 1, 1, &b) && b == 0, "1 x 1: 0 bytes");
        expect(!dis::check_fill_workspace(1, 2, 1, &b) && b == 8, "2 x 1: 8 bytes");
        expect(!dis::check_fill_workspace(2, 3, 5, &b) && b == 144, "two 3 x 5 fields");
        expect(!dis::check_fill_workspace(32, 1920, 1080, &b) && b == size_t(8) * 32 * 691302, "32 1080p fields");
        b = 77;
        expect(dis::check_fill_workspace(0, 4, 4, &b) && b == 77, "n = 0");
        expect(dis::check_fill_workspace(-1, 4, 4, &b) != nullptr, "n < 0");
        expect(dis::check_fill_workspace(1, 0, 4, &b) != nullptr, "width 0");
        expect(dis::check_fill_workspace(1, 4, -2, &b) != nullptr, "height < 0");
        expect(dis::check_fill_workspace(1, dis::kMaxExactSide + 1, 1, &b) != nullptr, "width beyond 2^24");
        expect(dis::check_fill_workspace(1, 1, dis::kMaxExactSide + 1, &b) != nullptr, "height beyond 2^24");
        expect(!dis::check_fill_workspace(1, dis::kMaxExactSide, 1, &b) && b == 8 * ((size_t(1) << 24) - 1), "2^24 x 1");
        expect(dis::check_fill_workspace(INT32_MAX, dis::kMaxExactSide, dis::kMaxExactSide, &b) != nullptr,
               "more blocks than a grid holds");
        expect(b == 8 * ((size_t(1) << 24) - 1), "a refusal leaves *bytes alone");
    }
    {  // the grid limit: 64 x 32 tiles, n * tiles <= 2^31 - 1
        expect(dis::fill_tile_blocks(1, 1, 1) == 1 && dis::fill_tile_blocks(3, 64, 32) == 3, "one tile a field");
        expect(dis::fill_tile_blocks(1, 65, 33) == 4 && dis::fill_tile_blocks(2, 1920, 1080) == 2 * 30 * 34, "tiles");
        expect(dis::fill_tile_blocks(0x7fffffff, 64, 32) == 0x7fffffffLL, "exactly a grid");
        expect(dis::fill_tile_blocks(0x7fffffff, 65, 32) == -1, "one column more");
        expect(dis::fill_tile_blocks(1, dis::kMaxExactSide, dis::kMaxExactSide) == -1, "2^24 squared");
        expect(dis::fill_tile_blocks(1, 64 * 46340, 32 * 46340) == 46340LL * 46340, "below the limit");
        expect(dis::fill_tile_blocks(0, 4, 4) == -1, "n = 0");
    }
    expect(!rule(plain()), "disjoint buffers");
    {  // out is flow itself
        Fill c = plain();
        c.out = c.flow;
        expect(!rule(c), "out == flow, equal formats");
        c.out = c.flow + 1;
        expect(rule(c) && std::strcmp(rule(c), "out and flow overlap") == 0, "out one byte into flow");
        c.out = c.flow + 8;
        expect(rule(c) != nullptr, "out one vector into flow");
        c.out = c.flow - 1;
        expect(rule(c) != nullptr, "out one byte before flow");
        c.out = c.flow + 799;
        expect(rule(c) != nullptr, "out on flow's last byte");
        c.out = c.flow + 800;
        expect(!rule(c), "out right after flow");
        c.out = c.flow - 800;
        expect(!rule(c), "out right before flow");
        c.out = c.flow;
        c.osz = 4;  // f16 out over an f32 flow
        expect(rule(c) != nullptr, "out == flow, out narrower");
        c.osz = 8;
        c.fsz = 4;
        expect(rule(c) != nullptr, "out == flow, flow narrower");
        c.osz = 4;
        expect(!rule(c), "out == flow, both f16");
    }
    {  // every other pair is refused, exact starts included
        Fill c = plain();
        c.out = c.mask;
        expect(rule(c) && std::strcmp(rule(c), "out and mask overlap") == 0, "out == mask");
        c = plain();
        c.out = c.mask - 799;
        expect(rule(c) != nullptr, "out ends on mask's first byte");
        c = plain();
        c.level = c.flow;
        expect(rule(c) && std::strcmp(rule(c), "level and flow overlap") == 0, "level == flow");
        c.level = c.mask;
        expect(rule(c) != nullptr, "level == mask");
        c.level = c.mask + 99;
        expect(rule(c) != nullptr, "level on mask's last byte");
        c.level = c.mask + 100;
        expect(!rule(c), "level right after mask");
        c = plain();
        c.level = c.out + 799;
        expect(rule(c) && std::strcmp(rule(c), "out and level overlap") == 0, "level on out's last byte");
        c = plain();
        c.ws = c.flow;
        expect(rule(c) && std::strcmp(rule(c), "workspace and flow overlap") == 0, "workspace == flow");
        c.ws = c.mask + 50;
        expect(rule(c) != nullptr, "workspace inside mask");
        c.ws = c.out - 399;
        expect(rule(c) && std::strcmp(rule(c), "out and workspace overlap") == 0, "workspace ends on out's first byte");
        c.ws = c.out - 400;
        expect(!rule(c), "workspace right before out");
        c.ws = c.level + 99;
        expect(rule(c) && std::strcmp(rule(c), "level and workspace overlap") == 0, "workspace on level's last byte");
        c = plain();  // in place, and the others inside the shared buffer
        c.out = c.flow;
        c.level = c.flow + 16;
        expect(rule(c) != nullptr, "out == flow with level inside them");
        c.level = 0x40000;
        c.ws = c.flow + 400;
        expect(rule(c) != nullptr, "out == flow with the workspace inside them");
    }
    {  // absent buffers are empty ranges, whatever their address
        Fill c = plain();
        c.has_mask = c.has_level = false;
        c.mask = c.level = 0;
        c.ws = 0;
        c.ws_bytes = 0;  // (a host call, or a 1 x 1 field)
        expect(!rule(c), "flow and out alone");
        c.level = c.flow;  // (an address, but no buffer)
        expect(!rule(c), "absent level at flow's address");
        c.has_level = true;
        expect(rule(c) != nullptr, "present level at flow's address");
        c = plain();
        c.has_mask = false;
        c.mask = c.out + 4;
        expect(!rule(c), "absent mask inside out");
        c.has_mask = true;
        expect(rule(c) != nullptr, "present mask inside out");
        c = plain();
        c.ws = c.out;
        c.ws_bytes = 0;
        expect(!rule(c), "an empty workspace at out's address");
    }
    {  // ranges that end with the last byte of the address space do not wrap
        const uintptr_t top = UINTPTR_MAX;
        Fill c = plain();
        c.flow = top - 799;
        expect(!rule(c), "flow ends at the top");
        c.out = c.flow;
        expect(!rule(c), "in place at the top");
        c.out = c.flow + 1;
        expect(rule(c) != nullptr, "out one byte into flow at the top");
        c = plain();
        c.ws = top - 399;
        expect(!rule(c), "workspace ends at the top");
        c.level = top - 50;
        expect(rule(c) != nullptr, "level inside the workspace at the top");
    }
    far::fill(&failures);  // the far cases (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
