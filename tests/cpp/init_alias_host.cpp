// init_alias_host.cpp -- the buffer aliasing rules of a warm-started call
// (csrc/dis_alias.h) on the CPU, built with -fsanitize=address,undefined by
// tests/test_init_host.py. Addresses are plain integers: nothing is
// dereferenced, so ranges at the ends of the address space can be tried too.
#include <cstdint>
#include <cstdio>

#include "dis_alias.h"

static int failures = 0;

static void expect(bool ok, bool want, const char* what)
{
    if (ok != want) {
        std::printf("FAIL: %s (accepted %d, wanted %d)\n", what, (int)ok, (int)want);
        ++failures;
    }
}

static bool accepted(uintptr_t init, size_t ib, uintptr_t flow, size_t fb, uintptr_t i0, uintptr_t i1, size_t frb)
{
    return dis::check_init_aliasing(init, ib, flow, fb, i0, i1, frb) == nullptr;
}

int main()
{
    const uintptr_t F = 0x100000, I0 = 0x800000, I1 = 0x900000;
    const size_t fb = 4096, frb = 512;
    // ranges_overlap
    expect(dis::ranges_overlap(10, 5, 15, 5), false, "adjacent ranges");
    expect(dis::ranges_overlap(10, 6, 15, 5), true, "one shared byte");
    expect(dis::ranges_overlap(15, 5, 10, 6), true, "one shared byte, swapped");
    expect(dis::ranges_overlap(10, 0, 10, 8), false, "empty range");
    expect(dis::ranges_overlap(UINTPTR_MAX - 7, 8, UINTPTR_MAX - 3, 4), true, "top of the address space");
    expect(dis::ranges_overlap(UINTPTR_MAX - 7, 4, UINTPTR_MAX - 3, 4), false, "top of the address space, adjacent");
    expect(dis::ranges_overlap(0, 1, UINTPTR_MAX, 1), false, "both ends");
    // init against flow
    expect(accepted(F, fb, F, fb, I0, I1, frb), true, "init is flow (full resolution)");
    expect(accepted(F, 120, F, fb, I0, I1, frb), true, "init is flow's start (a coarse plane)");
    expect(accepted(F + fb, fb, F, fb, I0, I1, frb), true, "init right after flow");
    expect(accepted(F - fb, fb, F, fb, I0, I1, frb), true, "init right before flow");
    expect(accepted(F + 8, fb, F, fb, I0, I1, frb), false, "init one vector into flow");
    expect(accepted(F - 8, fb, F, fb, I0, I1, frb), false, "init one vector before flow");
    expect(accepted(F + fb - 8, 120, F, fb, I0, I1, frb), false, "init over flow's last vector");
    expect(accepted(F + 64, 120, F, fb, I0, I1, frb), false, "a coarse plane inside flow");
    expect(accepted(F - 64, 16 * fb, F, fb, I0, I1, frb), false, "init contains flow");
    // init against the frames
    expect(accepted(I0, fb, F, fb, I0, I1, frb), false, "init is frame 0");
    expect(accepted(I1 + frb - 1, fb, F, fb, I0, I1, frb), false, "init over frame 1's last byte");
    expect(accepted(I1 + frb, fb, F, fb, I0, I1, frb), true, "init right after frame 1");
    expect(accepted(I0 - fb, fb, F, fb, I0, I1, frb), true, "init right before frame 0");
    expect(accepted(I0 - fb, fb + 1, F, fb, I0, I1, frb), false, "init over frame 0's first byte");
    // every small placement against a brute-force byte map
    for (uintptr_t init = 0; init < 48; ++init)
        for (size_t ib = 1; ib < 12; ++ib) {
            const uintptr_t flow = 16, i0 = 32, i1 = 40;
            const size_t fbb = 8, fr = 4;
            bool hit_flow = false, hit_frames = false;
            for (uintptr_t b = init; b < init + ib; ++b) {
                hit_flow |= b >= flow && b < flow + fbb;
                hit_frames |= (b >= i0 && b < i0 + fr) || (b >= i1 && b < i1 + fr);
            }
            const bool want = !hit_frames && (!hit_flow || init == flow);
            if (accepted(init, ib, flow, fbb, i0, i1, fr) != want) {
                std::printf("FAIL: brute force init %lu bytes %lu\n", (unsigned long)init, (unsigned long)ib);
                ++failures;
            }
        }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
