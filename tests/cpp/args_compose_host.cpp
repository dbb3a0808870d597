// args_compose_host.cpp -- the aliasing rule of dis_flow_compose and
// dis_flow_advect_points (csrc/dis_args.h, check_disjoint_or_same) and the
// points extent (check_points) at their edges: an output starting exactly at
// the input it may be against one byte in, a pair that was not listed, absent
// buffers, and ranges ending at the top of the address space. Built with
// -fsanitize=address,undefined by tests/cpp/compose.mk (target args_compose)
// and run by tests/test_compose_host.py. Nothing is dereferenced.
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

// dis_flow_compose's six ranges: a, b, valid_a, mask_b | out, valid_out; px
// pixels, asz / osz bytes per vector of a / out. Returns the refusal or null.
struct Compose {
    uintptr_t a, b, va, mb, out, vo;
    size_t px, asz, bsz, osz;
    bool has_va, has_mb, has_vo;
};
static dis::PairMessage g_why;
static const char* rule(const Compose& c)
{
    const dis::NamedRange r[6] = {{c.a, c.px * c.asz, "a"}, {c.b, c.px * c.bsz, "b"},
                                  {c.va, c.has_va ? c.px : 0, "valid_a"}, {c.mb, c.has_mb ? c.px : 0, "mask_b"},
                                  {c.out, c.px * c.osz, "out"}, {c.vo, c.has_vo ? c.px : 0, "valid_out"}};
    const dis::MayAlias may[2] = {{5, 2}, {4, 0}};
    return dis::check_disjoint_or_same(r, 4, 6, may, c.asz == c.osz ? 2 : 1, &g_why);
}
static Compose plain()
{
    // 100 pixels, f32 everywhere: fields of 800 bytes, planes of 100, all apart
    return {0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 100, 8, 8, 8, true, true, true};
}

int main()
{
    expect(!rule(plain()), "disjoint buffers");
    {  // out is a itself
        Compose c = plain();
        c.out = c.a;
        expect(!rule(c), "out == a, equal formats");
        c.out = c.a + 1;
        expect(rule(c) && std::strcmp(rule(c), "out and a overlap") == 0, "out one byte into a");
        c.out = c.a - 1;
        expect(rule(c) != nullptr, "out one byte before a");
        c.out = c.a + 799;
        expect(rule(c) != nullptr, "out on a's last byte");
        c.out = c.a + 800;
        expect(!rule(c), "out right after a");
        c.out = c.a - 800;
        expect(!rule(c), "out right before a");
        c.out = c.a;
        c.osz = 4;  // f16 out over an f32 a
        expect(rule(c) != nullptr, "out == a, out narrower");
        c.osz = 8;
        c.asz = 4;
        expect(rule(c) != nullptr, "out == a, a narrower");
        c.osz = 4;
        expect(!rule(c), "out == a, both f16");
    }
    {  // valid_out is valid_a itself
        Compose c = plain();
        c.vo = c.va;
        expect(!rule(c), "valid_out == valid_a");
        c.vo = c.va + 1;
        expect(rule(c) && std::strcmp(rule(c), "valid_out and valid_a overlap") == 0, "valid_out one byte into valid_a");
        c.vo = c.va + 99;
        expect(rule(c) != nullptr, "valid_out on valid_a's last byte");
        c.vo = c.va + 100;
        expect(!rule(c), "valid_out right after valid_a");
        c.vo = c.va;
        c.out = c.a;
        expect(!rule(c), "both in place");
        c.asz = 4;  // the planes do not depend on the formats
        c.out = 0x50000;
        expect(!rule(c), "valid_out == valid_a with a in f16");
    }
    {  // the pairs that were not listed stay refused, exact starts included
        Compose c = plain();
        c.out = c.b;
        expect(rule(c) && std::strcmp(rule(c), "out and b overlap") == 0, "out == b");
        c = plain();
        c.vo = c.mb;
        expect(rule(c) != nullptr, "valid_out == mask_b");
        c = plain();
        c.vo = c.a;
        expect(rule(c) != nullptr, "valid_out == a");
        c = plain();
        c.out = c.va;
        expect(rule(c) != nullptr, "out == valid_a");
        c = plain();
        c.out = c.mb - 799;
        expect(rule(c) != nullptr, "out ends on mask_b's first byte");
        c = plain();
        c.vo = c.out + 799;
        expect(rule(c) && std::strcmp(rule(c), "out and valid_out overlap") == 0, "valid_out on out's last byte");
        c.vo = c.out + 800;
        expect(!rule(c), "valid_out right after out");
        c = plain();  // in place, and valid_out inside the shared buffer
        c.out = c.a;
        c.vo = c.a + 8;
        expect(rule(c) != nullptr, "out == a with valid_out inside them");
    }
    {  // absent buffers are empty ranges, whatever their address
        Compose c = plain();
        c.has_va = c.has_mb = c.has_vo = false;
        c.va = c.mb = c.vo = 0;
        expect(!rule(c), "no byte planes");
        c.vo = c.a;  // (an address, but no buffer)
        expect(!rule(c), "absent valid_out at a's address");
        c.has_vo = true;
        expect(rule(c) != nullptr, "present valid_out at a's address");
        c = plain();
        c.has_va = false;
        c.va = c.out + 4;
        expect(!rule(c), "absent valid_a inside out");
        c.has_va = true;
        expect(rule(c) != nullptr, "present valid_a inside out");
        c = plain();
        c.has_va = false;  // valid_out at the address of an absent valid_a: nothing to be equal to, nothing to overlap
        c.vo = c.va;
        expect(!rule(c), "valid_out at an absent valid_a's address");
    }
    {  // ranges that end with the last byte of the address space do not wrap
        const uintptr_t top = UINTPTR_MAX;
        Compose c = plain();
        c.a = top - 799;
        expect(!rule(c), "a ends at the top");
        c.out = c.a;
        expect(!rule(c), "out == a at the top");
        c.out = c.a - 1;
        expect(rule(c) != nullptr, "out one byte before a at the top");
        c.out = c.a - 800;
        expect(!rule(c), "out right before a at the top");
        c = plain();
        c.vo = top - 99;
        c.va = top - 99;
        expect(!rule(c), "valid_out == valid_a at the top");
        c.va = top - 98;
        expect(rule(c) != nullptr, "valid_a one byte into valid_out at the top");
        c.va = top;  // (its extent would wrap; an absent one is empty)
        c.has_va = false;
        expect(!rule(c), "absent valid_a at the top");
        c = plain();
        c.out = top - 799;
        c.b = 0;
        expect(!rule(c), "out at the top, b at the bottom");
    }
    {  // the advect rule: flow, points | points_out, status
        const size_t pts = 50;
        auto adv = [&](uintptr_t flow, uintptr_t p, uintptr_t po, uintptr_t st, bool has_st) {
            const dis::NamedRange r[4] = {{flow, 800, "flow"}, {p, pts * 8, "points"}, {po, pts * 8, "points_out"},
                                          {st, has_st ? pts : 0, "status"}};
            const dis::MayAlias may[1] = {{2, 1}};
            return dis::check_disjoint_or_same(r, 2, 4, may, 1, &g_why);
        };
        expect(!adv(0x1000, 0x2000, 0x3000, 0x4000, true), "advect: disjoint");
        expect(!adv(0x1000, 0x2000, 0x2000, 0x4000, true), "advect: points_out == points");
        expect(adv(0x1000, 0x2000, 0x2008, 0x4000, true) != nullptr, "advect: points_out one point in");
        expect(adv(0x1000, 0x2000, 0x2000 + 399, 0, false) != nullptr, "advect: points_out on the last byte");
        expect(!adv(0x1000, 0x2000, 0x2000 + 400, 0, false), "advect: points_out right after points");
        expect(adv(0x1000, 0x2000, 0x1000, 0, false) != nullptr, "advect: points_out == flow");
        expect(adv(0x1000, 0x2000, 0x2000, 0x2000, true) != nullptr, "advect: status == points");
        expect(!adv(0x1000, 0x2000, 0x2000, 0x2000, false), "advect: absent status at points");
        expect(adv(0x1000, 0x2000, 0x3000, 0x3000 + 399, true) != nullptr, "advect: status on points_out's last byte");
    }
    {  // the points extent
        size_t pts = 7;
        expect(!dis::check_points(1, 1, &pts) && pts == 1, "one point");
        expect(!dis::check_points(3, 1000, &pts) && pts == 3000, "3 x 1000 points");
        expect(!dis::check_points(1 << 20, 1 << 20, &pts) && pts == (size_t(1) << 40), "2^40 points");
        pts = 7;
        expect(dis::check_points(1 << 20, (1 << 20) + 1, &pts) && pts == 7, "2^40 + 2^20 points");
        expect(dis::check_points(INT32_MAX, INT32_MAX, &pts) != nullptr, "the largest ints");
        expect(dis::check_points(0, 5, &pts) && dis::check_points(5, 0, &pts) && dis::check_points(-1, 5, &pts) &&
                   dis::check_points(5, -1, &pts), "n or count < 1");
    }
    far::compose(&failures);  // the far cases (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
