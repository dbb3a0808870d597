// args_color_host.cpp -- the frame-batch rule of the C-ABI (csrc/dis_args.h,
// check_frame_batch) with a pixel size: hand-computed strides and byte extents
// for 3 and 4 bytes per pixel, and today's values for 1. Built with
// -fsanitize=address,undefined by tests/cpp/color.mk (target args_color) and
// run by tests/test_color_host.py. Nothing is dereferenced.
#include <cstdint>
#include <cstdio>

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

static void expect_batch(const char* what, int px, int n, size_t stride, size_t pair_stride, size_t want_stride,
                         size_t want_pair, size_t want_bytes)
{
    dis::FrameBatch b{};
    const char* why = px == 1 ? dis::check_frame_batch(64, 48, n, 4, stride, pair_stride, &b)  // the old call
                              : dis::check_frame_batch(64, 48, n, 4, stride, pair_stride, &b, px);
    if (why || b.stride != want_stride || b.pair_stride != want_pair || b.bytes != want_bytes) {
        std::printf("FAIL: %s (%s; stride %zu pair %zu bytes %zu, wanted %zu %zu %zu)\n", what, why ? why : "accepted",
                    b.stride, b.pair_stride, b.bytes, want_stride, want_pair, want_bytes);
        ++failures;
    }
}

static bool refused(int px, int n, size_t stride, size_t pair_stride)
{
    dis::FrameBatch b{};
    return dis::check_frame_batch(64, 48, n, 4, stride, pair_stride, &b, px) != nullptr;
}

int main()
{
    // 64 x 48 frames. One byte per pixel: a row is 64 bytes, a frame 3072.
    expect_batch("gray, tight, 1 pair", 1, 1, 0, 0, 64, 3072, 3072);
    expect_batch("gray, tight, 3 pairs", 1, 3, 0, 0, 64, 3072, 2 * 3072 + 3072);
    expect_batch("gray, stride 80, 2 pairs 4000 apart", 1, 2, 80, 4000, 80, 4000, 4000 + 47 * 80 + 64);
    {  // the defaulted argument is 1
        dis::FrameBatch a{}, b{};
        expect(!dis::check_frame_batch(64, 48, 2, 4, 70, 0, &a) && !dis::check_frame_batch(64, 48, 2, 4, 70, 0, &b, 1) &&
                   a.stride == b.stride && a.pair_stride == b.pair_stride && a.bytes == b.bytes && a.bytes == 70 * 48 + 47 * 70 + 64,
               "pixel_bytes defaults to 1");
    }
    // three bytes per pixel: a row is 192 bytes, a frame 9216
    expect_batch("3 bytes, tight, 1 pair", 3, 1, 0, 0, 192, 9216, 9216);
    expect_batch("3 bytes, tight, 4 pairs", 3, 4, 0, 0, 192, 9216, 3 * 9216 + 9216);
    expect_batch("3 bytes, stride 200", 3, 2, 200, 0, 200, 9600, 9600 + 47 * 200 + 192);
    expect_batch("3 bytes, stride 208, pairs 10000 apart", 3, 3, 208, 10000, 208, 10000, 2 * 10000 + 47 * 208 + 192);
    expect(refused(3, 1, 191, 0), "3 bytes: a stride of 191 is smaller than a row");
    expect(refused(3, 1, 64, 0), "3 bytes: the gray stride is smaller than a row");
    expect(!refused(3, 1, 192, 0), "3 bytes: a stride of exactly a row");
    expect(refused(3, 2, 0, 9215), "3 bytes: pair_stride smaller than a frame");
    expect(!refused(3, 2, 0, 9216), "3 bytes: pair_stride of exactly a frame");
    expect(!refused(3, 1, 0, 5), "3 bytes: one pair does not use pair_stride");
    // four bytes per pixel: a row is 256 bytes, a frame 12288
    expect_batch("4 bytes, tight, 1 pair", 4, 1, 0, 0, 256, 12288, 12288);
    expect_batch("4 bytes, tight, 2 pairs", 4, 2, 0, 0, 256, 12288, 12288 + 12288);
    expect_batch("4 bytes, stride 272, pairs 13100 apart", 4, 2, 272, 13100, 272, 13100, 13100 + 47 * 272 + 256);
    expect(refused(4, 1, 255, 0), "4 bytes: a stride of 255 is smaller than a row");
    expect(refused(4, 2, 272, 272 * 48 - 1), "4 bytes: pair_stride smaller than a padded frame");
    // n and the pixel size itself
    expect(refused(3, 0, 0, 0) && refused(3, 5, 0, 0), "n outside [1, max_batch]");
    expect(refused(0, 1, 0, 0) && refused(-1, 1, 0, 0), "pixel_bytes < 1");
    // the extents feed the overlap rules: a flow right after the last sample is disjoint, one byte earlier is not
    {
        dis::FrameBatch b{};
        dis::check_frame_batch(64, 48, 2, 4, 200, 0, &b, 3);
        const uintptr_t I0 = 0x100000;
        expect(!dis::ranges_overlap(I0, b.bytes, I0 + b.bytes, 4096), "flow right after the colour frames");
        expect(dis::ranges_overlap(I0, b.bytes, I0 + b.bytes - 1, 4096), "flow over the colour frames' last sample");
        expect(dis::check_init_aliasing(I0 + 3072, 64, 0x900000, 4096, I0, 0x500000, b.bytes) != nullptr,
               "init inside the colour frames, past a gray frame's extent");
        expect(dis::check_init_aliasing(I0 + 3072, 64, 0x900000, 4096, I0, 0x500000, 3072) == nullptr,
               "the same init after a gray frame");
    }
    far::color(&failures);  // dis_flow_color with more fields than a launch's y extent (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
