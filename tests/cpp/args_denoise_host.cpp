// args_denoise_host.cpp -- the argument rules of dis_temporal_denoise_u8
// (csrc/dis_args.h): the grid of 64 x 16 tiles at its edges (denoise_blocks),
// the sizes (check_denoise_sizes), a weight's bounds (denoise_weight_ok) and
// the buffers by address (check_denoise_buffers: null entries, the flows'
// alignment and the overlap rule over up to 27 ranges). Built with
// -fsanitize=address,undefined by tests/cpp/denoise.mk (target args_denoise)
// and run by tests/test_denoise_host.py. Nothing is dereferenced.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

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

// A call of K neighbours over 100 pixels of 3 channels (images of 300 bytes),
// f32 flows of 800 bytes, planes of 100 bytes, every buffer 0x1000 apart.
struct Call {
    uintptr_t cur, nb[8], fl[8], mk[8], dst, support;
    int K;
    bool has_masks;
    size_t image_bytes, flow_bytes, px, dst_bytes, align;
};
static dis::PairMessage g_why;
static const char* rule(const Call& c)
{
    return dis::check_denoise_buffers(c.cur, c.nb, c.fl, c.has_masks ? c.mk : nullptr, c.K, c.image_bytes, c.flow_bytes,
                                      c.px, c.dst, c.dst_bytes, c.support, c.align, &g_why);
}
static Call plain(int K)
{
    Call c{};
    c.cur = 0x10000;
    for (int k = 0; k < 8; ++k) c.nb[k] = 0x20000 + 0x1000 * k, c.fl[k] = 0x30000 + 0x1000 * k, c.mk[k] = 0x40000 + 0x1000 * k;
    c.dst = 0x50000;
    c.support = 0x51000;
    c.K = K;
    c.has_masks = true;
    c.image_bytes = 300, c.flow_bytes = 800, c.px = 100, c.dst_bytes = 300, c.align = 0;
    return c;
}
static bool says(const char* got, const char* want) { return got && std::strstr(got, want); }

int main()
{
    {  // the grid
        expect(dis::denoise_blocks(1, 1, 1) == 1 && dis::denoise_blocks(3, 64, 16) == 3, "one tile holds 64 x 16 pixels");
        expect(dis::denoise_blocks(1, 65, 16) == 2 && dis::denoise_blocks(1, 64, 17) == 2, "one pixel more is one tile more");
        expect(dis::denoise_blocks(2, 129, 33) == 2 * 3 * 3, "two tiles and a pixel in each dimension");
        expect(dis::denoise_blocks(32, 1920, 1080) == 32 * 30 * 68, "1080p: 30 x 68 tiles");
        expect(dis::denoise_blocks(0, 4, 4) == -1 && dis::denoise_blocks(-1, 4, 4) == -1, "n < 1");
        expect(dis::denoise_blocks(1, 0, 4) == -1 && dis::denoise_blocks(1, 4, 0) == -1, "an empty side");
        // 2^24 x 2^24: 2^18 x 2^20 tiles = 2^38 > a grid; 2^24 x 8176: 2^18 x 511 tiles, 16 of them fit, 17 do not
        expect(dis::denoise_blocks(1, dis::kMaxExactSide, dis::kMaxExactSide) == -1, "the largest frame exceeds a grid");
        expect(dis::denoise_blocks(16, dis::kMaxExactSide, 8176) == 16ll * 262144 * 511, "16 * 2^18 * 511 < 2^31");
        expect(dis::denoise_blocks(17, dis::kMaxExactSide, 8176) == -1, "17 * 2^18 * 511 > 2^31 - 1");
        expect(dis::denoise_blocks(INT_MAX, 64, 16) == INT_MAX && dis::denoise_blocks(INT_MAX, 65, 16) == -1, "n at the limit");
        expect(dis::denoise_blocks(INT_MAX, INT_MAX, INT_MAX) == -1, "no overflow at the largest integers");
    }
    {  // the sizes
        expect(!dis::check_denoise_sizes(1, 1, 1, 1, 1) && !dis::check_denoise_sizes(8, 2, 5, 3, 4), "valid calls");
        expect(!dis::check_denoise_sizes(8, 1, dis::kMaxExactSide, 1, 3), "the largest side");
        expect(dis::check_denoise_sizes(0, 1, 4, 4, 1) && dis::check_denoise_sizes(9, 1, 4, 4, 1), "K outside 1..8");
        expect(dis::check_denoise_sizes(-1, 1, 4, 4, 1) && dis::check_denoise_sizes(INT_MIN, 1, 4, 4, 1), "negative K");
        expect(dis::check_denoise_sizes(1, 0, 4, 4, 1) && dis::check_denoise_sizes(1, 1, 0, 4, 1) &&
                   dis::check_denoise_sizes(1, 1, 4, -1, 1), "n, width, height < 1");
        expect(dis::check_denoise_sizes(1, 1, dis::kMaxExactSide + 1, 1, 1) &&
                   dis::check_denoise_sizes(1, 1, 1, dis::kMaxExactSide + 1, 1), "a side past 2^24");
        for (int c : {0, 2, 5, -1, INT_MAX}) expect(dis::check_denoise_sizes(1, 1, 4, 4, c) != nullptr, "channels not 1, 3, 4");
        expect(dis::check_denoise_sizes(1, 17, dis::kMaxExactSide, 8176, 1) != nullptr, "the grid");
    }
    {  // a weight
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        expect(dis::denoise_weight_ok(0.0f) && dis::denoise_weight_ok(-0.0f) && dis::denoise_weight_ok(1.0f) &&
                   dis::denoise_weight_ok(1e-45f), "0, -0, 1 and the smallest denormal pass");
        expect(!dis::denoise_weight_ok(std::nextafter(1.0f, 2.0f)) && !dis::denoise_weight_ok(-1e-45f), "just outside");
        expect(!dis::denoise_weight_ok(inf) && !dis::denoise_weight_ok(-inf) && !dis::denoise_weight_ok(nan), "not finite");
    }
    {  // the buffers
        for (int K = 1; K <= 8; ++K) expect(!rule(plain(K)), "disjoint buffers pass for every K");
        Call c = plain(0);
        expect(rule(c) != nullptr, "K = 0");
        c = plain(9);
        expect(rule(c) != nullptr, "K = 9 (nothing past the eighth entry is read)");
        c = plain(3), c.nb[2] = 0;
        expect(says(rule(c), "null entry"), "a null neighbour");
        c = plain(3), c.fl[0] = 0;
        expect(says(rule(c), "null entry"), "a null flow");
        c = plain(3), c.nb[3] = 0, c.fl[3] = 0;
        expect(!rule(c), "entries past K take no part");
        c = plain(3), c.mk[1] = 0;
        expect(!rule(c), "a null mask entry is allowed");
        c = plain(3), c.has_masks = false, c.dst = c.mk[1];
        expect(!rule(c), "without masks their addresses take no part");
        c = plain(3), c.mk[1] = 0, c.support = 0;
        expect(!rule(c), "no support");
        // alignment of device flows
        c = plain(2), c.align = 8, c.fl[1] += 4;
        expect(says(rule(c), "aligned"), "an f32 flow 4 bytes off");
        c = plain(2), c.align = 4, c.flow_bytes = 400, c.fl[1] += 4;
        expect(!rule(c), "an f16 flow 4 bytes off is pair-aligned");
        c.fl[0] += 2;
        expect(says(rule(c), "aligned"), "an f16 flow 2 bytes off");
        c = plain(2), c.fl[1] += 1;
        expect(!rule(c), "host flows need no alignment");
        // overlaps: dst and support against every input and each other
        c = plain(8), c.dst = c.cur;
        expect(says(rule(c), "dst and cur overlap"), "dst = cur");
        c = plain(8), c.dst = c.cur + 299;
        expect(says(rule(c), "dst and cur overlap"), "dst on cur's last byte");
        c = plain(8), c.dst = c.cur + 300;
        expect(!rule(c), "dst right behind cur");
        c = plain(8), c.dst = c.cur - 300;
        expect(!rule(c), "dst right before cur");
        c = plain(8), c.dst = c.cur - 299;
        expect(says(rule(c), "dst and cur overlap"), "dst ends in cur");
        for (int k = 0; k < 8; ++k) {
            char want[64];
            c = plain(8), c.dst = c.nb[k] + 299;
            std::snprintf(want, sizeof want, "dst and neighbours[%d] overlap", k);
            expect(says(rule(c), want), "dst on a neighbour's last byte");
            c = plain(8), c.dst = c.fl[k] + 799;
            std::snprintf(want, sizeof want, "dst and flows[%d] overlap", k);
            expect(says(rule(c), want), "dst on a flow's last byte");
            c = plain(8), c.support = c.mk[k] - 99;
            std::snprintf(want, sizeof want, "support and masks[%d] overlap", k);
            expect(says(rule(c), want), "support ends in a mask");
            c = plain(8), c.support = c.nb[k];
            expect(rule(c) != nullptr, "support = a neighbour");
            c = plain(8), c.support = c.fl[k] + 400;
            expect(rule(c) != nullptr, "support inside a flow");
            c = plain(8), c.support = c.mk[k] + 100;
            expect(!rule(c), "support right behind a mask");
        }
        c = plain(7), c.dst = c.nb[7];
        expect(!rule(c), "the eighth neighbour of a call of seven takes no part");
        c = plain(2), c.support = c.dst + 299;
        expect(says(rule(c), "dst and support overlap"), "support on dst's last byte");
        c = plain(2), c.support = c.dst + 300;
        expect(!rule(c), "support right behind dst");
        c = plain(2), c.support = c.cur + 150;
        expect(says(rule(c), "support and cur overlap"), "support inside cur");
        // inputs may share memory (a frame is its own neighbour's buffer, one mask for all)
        c = plain(3), c.nb[0] = c.cur, c.nb[1] = c.nb[2], c.mk[0] = c.mk[1] = c.mk[2], c.fl[1] = c.fl[0];
        expect(!rule(c), "inputs may overlap each other");
        // ranges at the top of the address space do not wrap
        c = plain(1), c.dst = UINTPTR_MAX - 299, c.support = 0;
        expect(!rule(c), "dst ending at the last byte");
        c.cur = UINTPTR_MAX - 10;
        c.image_bytes = 11;
        expect(says(rule(c), "dst and cur overlap"), "cur inside it");
    }
    far::denoise(&failures);  // the far cases (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
