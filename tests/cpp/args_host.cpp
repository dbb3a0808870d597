// args_host.cpp -- the argument rules of the C-ABI (csrc/dis_args.h) on the
// CPU, built with -fsanitize=address,undefined by tests/test_init_host.py.
// Addresses are plain integers: nothing is dereferenced, so ranges at the ends
// of the address space can be tried too.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "dis_args.h"
#include "far_cases.h"

static int failures = 0;

static void expect(bool ok, bool want, const char* what)
{
    if (ok != want) {
        std::printf("FAIL: %s (accepted %d, wanted %d)\n", what, (int)ok, (int)want);
        ++failures;
    }
}

static void expect_eq(size_t got, size_t want, const char* what)
{
    if (got != want) {
        std::printf("FAIL: %s (got %zu, wanted %zu)\n", what, got, want);
        ++failures;
    }
}

static bool accepted(uintptr_t init, size_t ib, uintptr_t flow, size_t fb, uintptr_t i0, uintptr_t i1, size_t frb)
{
    return dis::check_init_aliasing(init, ib, flow, fb, i0, i1, frb) == nullptr;
}

static void init_aliasing()
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
}

static void dims()
{
    const int S = dis::kMaxExactSide;
    const long long P = dis::kMaxKeyPixels;
    expect(!dis::check_dims(1, 1, 1), true, "1 x 1 x 1");
    expect(!dis::check_dims(0, 16, 4), false, "n = 0");
    expect(!dis::check_dims(-3, 16, 4), false, "n = -3");
    expect(!dis::check_dims(2, 0, 4), false, "width = 0");
    expect(!dis::check_dims(2, -5, 4), false, "width = -5");
    expect(!dis::check_dims(2, 16, 0), false, "height = 0");
    expect(!dis::check_dims(2, 16, -1), false, "height = -1");
    expect(!dis::check_dims(INT32_MAX, INT32_MAX, INT32_MAX), true, "no limit asked for");
    expect(!dis::check_dims(1, S, 1, S), true, "width = 2^24");
    expect(!dis::check_dims(1, S + 1, 1, S), false, "width = 2^24 + 1");
    expect(!dis::check_dims(1, 1, S, S), true, "height = 2^24");
    expect(!dis::check_dims(1, 1, S + 1, S), false, "height = 2^24 + 1");
    expect(!dis::check_dims(INT32_MAX, S, S, S), true, "n is not limited here");
    expect(!dis::check_dims(1, 1 << 16, 1 << 15, S, P), true, "width * height = 2^31");
    expect(!dis::check_dims(1, 1 << 16, (1 << 15) + 1, S, P), false, "width * height = 2^31 + 2^16");
    expect(!dis::check_dims(1, S, S, S, P), false, "width * height = 2^48");
}

static bool stack_ok(int w, int h, int c, int n, size_t stride, size_t image_stride, dis::ImageStack* out)
{
    return dis::check_image_stack(w, h, c, n, stride, image_stride, out) == nullptr;
}

// the refusals of tests/test_warp_host.py and tests/test_interp_host.py as integers
static void image_stacks()
{
    const int W = 16, H = 4, C = 3, N = 2;
    const size_t row = (size_t)W * C;
    dis::ImageStack s{};
    expect(stack_ok(W, H, C, N, 0, 0, &s), true, "tight by default");
    expect_eq(s.stride, row, "default stride");
    expect_eq(s.image_stride, row * H, "default image stride");
    expect_eq(s.bytes, row * H * N, "tight extent");
    expect(stack_ok(W, H, C, N, row, row * H, &s), true, "tight, spelt out");
    expect_eq(s.bytes, row * H * N, "tight extent, spelt out");
    expect(stack_ok(W, H, C, N, row - 1, 0, &s), false, "stride < row");
    expect(stack_ok(W, H, C, N, 0, row * H - 1, &s), false, "image_stride < image");
    expect(stack_ok(W, H, C, N, row + 5, (row + 5) * H - 1, &s), false, "image_stride < padded image");
    expect(stack_ok(W, H, C, N, row + 5, (row + 5) * H, &s), true, "image_stride = padded image");
    expect(stack_ok(W, H, C, N, row + 5, 0, &s), true, "padded rows, default image stride");
    expect_eq(s.image_stride, (row + 5) * H, "default image stride of padded rows");
    // padding after the last row or image is not part of the source
    expect(stack_ok(W, H, 1, 1, W + 5, (W + 5) * H + 7, &s), true, "one padded image");
    expect_eq(s.bytes, (size_t)(H - 1) * (W + 5) + W, "one padded image ends with its last sample");
    expect(stack_ok(37, 5, 3, 2, 37 * 3 + 5, (37 * 3 + 5) * 5 + 7, &s), true, "two padded images");
    expect_eq(s.bytes, (size_t)((37 * 3 + 5) * 5 + 7) + 4 * (37 * 3 + 5) + 37 * 3, "two padded images' extent");
    for (int bad = 0; bad < 4; ++bad)
        expect(stack_ok(bad == 0 ? 0 : W, bad == 1 ? 0 : H, bad == 2 ? 0 : C, bad == 3 ? 0 : N, 0, 0, &s), false,
               "a zero dimension");
    expect(stack_ok(W, -1, C, N, 0, 0, &s), false, "a negative height");
    // the size limits, at and one past each bound
    const size_t smax = (size_t(1) << 48) / H;
    expect(stack_ok(W, H, C, 1, smax, 0, &s), true, "stride = 2^48 / height");
    expect_eq(s.bytes, (H - 1) * smax + row, "extent at the stride limit");
    expect(stack_ok(W, H, C, 1, smax + 1, 0, &s), false, "stride = 2^48 / height + 1");
    expect(stack_ok(W, 3, C, 1, (size_t(1) << 48) / 3, 0, &s), true, "stride = floor(2^48 / 3)");
    expect(stack_ok(W, 3, C, 1, (size_t(1) << 48) / 3 + 1, 0, &s), false, "stride = floor(2^48 / 3) + 1");
    const size_t imax = (size_t(1) << 62) / N;
    expect(stack_ok(W, H, C, N, 0, imax, &s), true, "image_stride = 2^62 / n");
    expect_eq(s.bytes, imax + row * H, "extent at the image stride limit");
    expect(stack_ok(W, H, C, N, 0, imax + 1, &s), false, "image_stride = 2^62 / n + 1");
    expect(stack_ok(W, H, C, 3, 0, (size_t(1) << 62) / 3, &s), true, "image_stride = floor(2^62 / 3)");
    expect(stack_ok(W, H, C, 3, 0, (size_t(1) << 62) / 3 + 1, &s), false, "image_stride = floor(2^62 / 3) + 1");
    expect(stack_ok(W, H, C, N, SIZE_MAX, 0, &s), false, "stride = SIZE_MAX");
    expect(stack_ok(W, H, C, N, 0, SIZE_MAX, &s), false, "image_stride = SIZE_MAX");
    // tight rows of 2^24 bytes, 2^24 of them, 2^14 images: both limits met at once
    expect(stack_ok(1 << 22, 1 << 24, 4, 1 << 14, 0, 0, &s), true, "the largest tight stack");
    expect_eq(s.bytes, size_t(1) << 62, "the largest tight stack's extent");
    expect(stack_ok(1 << 22, 1 << 24, 4, (1 << 14) + 1, 0, 0, &s), false, "one image more");
    expect(stack_ok((1 << 22) + 1, 1 << 24, 4, 1, 0, 0, &s), false, "one pixel wider");
}

static bool batch_ok(int n, int max_batch, size_t stride, size_t pair_stride, dis::FrameBatch* out)
{
    return dis::check_frame_batch(64, 48, n, max_batch, stride, pair_stride, out) == nullptr;
}

static void frame_batches()
{
    dis::FrameBatch b{};
    expect(batch_ok(3, 3, 0, 0, &b), true, "tight by default");
    expect_eq(b.stride, 64, "default stride");
    expect_eq(b.pair_stride, 64 * 48, "default pair stride");
    expect_eq(b.bytes, 3 * 64 * 48, "tight extent");
    expect(batch_ok(0, 3, 0, 0, &b), false, "n = 0");
    expect(batch_ok(-1, 3, 0, 0, &b), false, "n = -1");
    expect(batch_ok(4, 3, 0, 0, &b), false, "n = max_batch + 1");
    expect(batch_ok(1, 3, 63, 0, &b), false, "stride < width");
    expect(batch_ok(2, 3, 70, 0, &b), true, "padded rows");
    expect_eq(b.pair_stride, 70 * 48, "default pair stride of padded rows");
    expect_eq(b.bytes, 70 * 48 + 47 * 70 + 64, "padded rows' extent ends with the last sample");
    expect(batch_ok(2, 3, 70, 70 * 48 - 1, &b), false, "pair_stride < padded frame");
    expect(batch_ok(2, 3, 70, 70 * 48 + 9, &b), true, "padded frames");
    expect_eq(b.bytes, 70 * 48 + 9 + 47 * 70 + 64, "padded frames' extent");
    // a single pair does not use pair_stride
    expect(batch_ok(1, 3, 70, 5, &b), true, "n = 1 with a small pair_stride");
    expect_eq(b.bytes, 47 * 70 + 64, "one pair's extent");
}

static const char* disjoint(const dis::NamedRange* in, int nin, const dis::NamedRange* out, int nout)
{
    static dis::PairMessage why;
    dis::NamedRange r[8];
    for (int k = 0; k < nin + nout; ++k) r[k] = k < nin ? in[k] : out[k - nin];
    return dis::check_disjoint(r, nin, nin + nout, &why);
}

static void expect_msg(const char* got, const char* want, const char* what)
{
    if ((got == nullptr) != (want == nullptr) || (got && std::strcmp(got, want))) {
        std::printf("FAIL: %s (got %s, wanted %s)\n", what, got ? got : "acceptance", want ? want : "acceptance");
        ++failures;
    }
}

static void disjointness()
{
    const uintptr_t T = UINTPTR_MAX;
    {
        const dis::NamedRange in[2] = {{0x1000, 64, "src"}, {0x2000, 64, "flow"}};
        dis::NamedRange out[2] = {{0x3000, 64, "dst"}, {0x4000, 16, "valid"}};
        expect_msg(disjoint(in, 2, out, 2), nullptr, "all apart");
        out[1].p = 0x2000 + 63;
        expect_msg(disjoint(in, 2, out, 2), "valid and flow overlap", "valid starts in flow");
        out[0].p = 0x1000 - 63;
        expect_msg(disjoint(in, 2, out, 2), "dst and src overlap", "the first pair is reported");
        out[0].p = 0x1000 - 64;
        out[1] = {0x1000 - 1, 0, "valid"};
        expect_msg(disjoint(in, 2, out, 2), nullptr, "dst ends where src starts; an empty valid");
        out[1] = {0x1000 - 1, 1, "valid"};
        expect_msg(disjoint(in, 2, out, 2), "dst and valid overlap", "outputs against each other");
        expect_msg(disjoint(nullptr, 0, out, 2), "dst and valid overlap", "outputs alone");
        expect_msg(disjoint(in, 2, nullptr, 0), nullptr, "inputs may overlap each other");
    }
    {  // ranges ending at the top of the address space: the sums a + na would wrap to 0
        const dis::NamedRange in[1] = {{T - 63, 64, "src"}};
        dis::NamedRange out[1] = {{T - 127, 64, "dst"}};
        expect_msg(disjoint(in, 1, out, 1), nullptr, "dst right below a src that ends at the top");
        out[0].bytes = 65;
        expect_msg(disjoint(in, 1, out, 1), "dst and src overlap", "dst one byte into a src that ends at the top");
        out[0] = {T, 1, "dst"};
        expect_msg(disjoint(in, 1, out, 1), "dst and src overlap", "dst is the last byte");
        out[0] = {0, 64, "dst"};
        expect_msg(disjoint(in, 1, out, 1), nullptr, "the two ends of the address space");
        out[0] = {T - 63, 0, "dst"};
        expect_msg(disjoint(in, 1, out, 1), nullptr, "an empty dst at the top");
    }
    // every placement of 2 inputs and 2 outputs of 0..5 bytes in a 24-byte
    // space against a byte map (one bit per byte): whether a pair overlaps and
    // which is the first (check_disjoint, tried above, only words it)
    struct Place {
        uintptr_t p;
        size_t bytes;
        uint32_t map;
    };
    static Place pl[6 * 25];
    int np = 0;
    for (size_t len = 0; len <= 5; ++len)
        for (uintptr_t p = 0; p + len <= 24; ++p) pl[np++] = {p, len, (uint32_t)(((1u << len) - 1) << p)};
    long long tried = 0, refused = 0;
    dis::NamedRange r[4] = {{0, 0, "a"}, {0, 0, "b"}, {0, 0, "c"}, {0, 0, "d"}};  // two inputs, two outputs
    const auto place = [](dis::NamedRange& r, const Place& at) { r.p = at.p, r.bytes = at.bytes; };
    for (int a = 0; a < np; ++a)
        for (int b = 0; b < np; ++b)
            for (int c = 0; c < np; ++c) {
                place(r[0], pl[a]), place(r[1], pl[b]), place(r[2], pl[c]);
                const uint32_t ma = pl[a].map, mb = pl[b].map, mc = pl[c].map;
                for (int d = 0; d < np; ++d) {
                    place(r[3], pl[d]);
                    const uint32_t md = pl[d].map;
                    int x = -1, y = -1, wx = -1, wy = -1;
                    if (mc & ma) wx = 2, wy = 0;
                    else if (mc & mb) wx = 2, wy = 1;
                    else if (mc & md) wx = 2, wy = 3;
                    else if (md & ma) wx = 3, wy = 0;
                    else if (md & mb) wx = 3, wy = 1;
                    const bool got = dis::first_overlap(r, 2, 4, &x, &y);
                    ++tried;
                    refused += got;
                    if (got != (wx >= 0) || (got && (x != wx || y != wy))) {
                        if (failures < 20)
                            std::printf("FAIL: brute force a %d b %d c %d d %d: got pair %d %d, wanted %d %d\n", a, b, c,
                                        d, x, y, wx, wy);
                        ++failures;
                    }
                }
            }
    std::printf("disjointness: %lld placements, %lld refused\n", tried, refused);
}

int main()
{
    init_aliasing();
    dims();
    image_stacks();
    frame_batches();
    disjointness();
    far::flat_families(&failures);  // the far cases of warp, interp, consistency and frames-to-gray (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
