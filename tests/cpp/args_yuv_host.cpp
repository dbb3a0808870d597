// args_yuv_host.cpp -- the argument rules of dis_yuv420_to_frames_u8 and
// dis_frames_to_yuv420_u8 (csrc/dis_args.h): check_yuv420_layout's strides and
// byte extents by hand, plane_stacks_overlap against a byte-by-byte count on
// small cases, the chroma planes of interleaved and planar surfaces, the overlap
// list and the grid. Built with -fsanitize=address,undefined by tests/cpp/yuv.mk
// (target args_yuv) and run by tests/test_yuv_host.py. Nothing is dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

static bool refused(int n, int w, int h, int step, size_t ys, size_t yi, size_t cs, size_t ci)
{
    dis::Yuv420Layout l{};
    return dis::check_yuv420_layout(n, w, h, step, ys, yi, cs, ci, &l) != nullptr;
}

// the rule by counting: every byte of every image of both planes, on a small address range
static bool overlap_by_bytes(const dis::PlaneStack& a, const dis::PlaneStack& b, int n)
{
    std::vector<char> seen(4096, 0);
    for (int i = 0; i < n; ++i)
        for (size_t k = 0; k < a.image_bytes; ++k) seen[a.p + i * a.image_stride + k] = 1;
    for (int i = 0; i < n; ++i)
        for (size_t k = 0; k < b.image_bytes; ++k)
            if (seen[b.p + i * b.image_stride + k]) return true;
    return false;
}

int main()
{
    using namespace dis;
    // 20 x 4 pixels. NV12: rows of 20 bytes, a chroma row is 10 pairs = 20 bytes; an image is 120 bytes.
    {
        Yuv420Layout l{};
        expect(!check_yuv420_layout(2, 20, 4, 2, 0, 0, 0, 0, &l) && l.y_stride == 20 && l.y_image_stride == 80 &&
                   l.c_stride == 20 && l.c_image_stride == 40 && l.y_bytes == 80 && l.c_bytes == 20 + 18 + 1,
               "interleaved, every stride defaulted");
        expect(!check_yuv420_layout(3, 20, 4, 2, 32, 192, 32, 192, &l) && l.y_stride == 32 && l.y_image_stride == 192 &&
                   l.c_stride == 32 && l.c_image_stride == 192 && l.y_bytes == 3 * 32 + 20 && l.c_bytes == 32 + 19,
               "NV12 with a stride of 32 in one buffer");
        expect(!check_yuv420_layout(2, 20, 4, 1, 0, 0, 0, 0, &l) && l.c_stride == 10 && l.c_image_stride == 20 &&
                   l.c_bytes == 10 + 9 + 1,
               "planar, every stride defaulted");
        expect(!check_yuv420_layout(1, 2, 2, 1, 0, 0, 0, 0, &l) && l.y_bytes == 4 && l.c_bytes == 1, "2 x 2 planar");
        expect(!check_yuv420_layout(1, 2, 2, 2, 0, 0, 0, 0, &l) && l.y_bytes == 4 && l.c_bytes == 1 && l.c_stride == 2,
               "2 x 2 interleaved: a plane pointer owns one byte");
    }
    expect(refused(0, 20, 4, 2, 0, 0, 0, 0) && refused(1, 0, 4, 2, 0, 0, 0, 0) && refused(1, 20, -2, 2, 0, 0, 0, 0),
           "n, width, height < 1");
    expect(refused(1, 19, 4, 2, 0, 0, 0, 0) && refused(1, 20, 3, 2, 0, 0, 0, 0) && refused(1, 1, 1, 1, 0, 0, 0, 0),
           "odd sides");
    expect(refused(1, (1 << 24) + 2, 2, 1, 0, 0, 0, 0) && refused(1, 2, (1 << 24) + 2, 1, 0, 0, 0, 0) &&
               !refused(1, 1 << 24, 2, 1, 0, 0, 0, 0),
           "sides above 2^24");
    expect(refused(1, 20, 4, 0, 0, 0, 0, 0) && refused(1, 20, 4, 3, 0, 0, 0, 0) && refused(1, 20, 4, -1, 0, 0, 0, 0),
           "c_step other than 1 or 2");
    expect(refused(1, 20, 4, 2, 19, 0, 0, 0) && !refused(1, 20, 4, 2, 20, 0, 0, 0), "y_stride against a row");
    expect(refused(2, 20, 4, 2, 24, 95, 0, 0) && !refused(2, 20, 4, 2, 24, 96, 0, 0), "y_image_stride against an image");
    expect(refused(1, 20, 4, 2, 0, 0, 19, 0) && !refused(1, 20, 4, 2, 0, 0, 20, 0), "interleaved c_stride against a row");
    expect(refused(1, 20, 4, 1, 0, 0, 9, 0) && !refused(1, 20, 4, 1, 0, 0, 10, 0), "planar c_stride against a row");
    expect(refused(2, 20, 4, 1, 0, 0, 16, 31) && !refused(2, 20, 4, 1, 0, 0, 16, 32), "c_image_stride against an image");
    expect(refused(1, 20, 4, 1, size_t(1) << 60, 0, 0, 0) && refused(4, 20, 4, 1, 0, size_t(1) << 61, 0, 0),
           "strides too large for the products");

    // the grid: a lane per 16 x 2 pixels, 256 lanes a block
    expect(yuv420_blocks(1, 2, 2) == 1 && yuv420_blocks(1, 16, 512) == 1 && yuv420_blocks(1, 18, 512) == 2 &&
               yuv420_blocks(64, 1920, 1080) == (64ll * 540 * 120 + 255) / 256,
           "blocks of a launch");
    expect(yuv420_blocks(0x7fffffff, 4096, 4096) < 0 && yuv420_blocks(0, 16, 16) < 0 && yuv420_blocks(1, 0, 16) < 0 &&
               yuv420_blocks(0x7fffffff, 2, 2) > 0,
           "the grid limit");

    // plane against plane, against counting: every pair of offsets of two planes of 3 images
    {
        int wrong = 0, overlapping = 0;
        for (size_t S : {40u, 56u})
            for (size_t ea : {1u, 17u, 40u})
                for (size_t eb : {1u, 23u, 40u})
                    for (uintptr_t pa = 200; pa < 200 + 2 * S; pa += 3)
                        for (uintptr_t pb = 100; pb < 460; ++pb) {
                            const PlaneStack a{pa, S, ea, "a"}, b{pb, S, eb, "b"};
                            const bool got = plane_stacks_overlap(a, b, 3), want = overlap_by_bytes(a, b, 3);
                            wrong += got != want || plane_stacks_overlap(b, a, 3) != want;
                            overlapping += want;
                        }
        expect(wrong == 0 && overlapping > 1000, "one image stride: the rule is the byte count's");
        // two image strides: the whole extents, which is never less than the byte count
        int missed = 0;
        for (uintptr_t pb = 100; pb < 460; ++pb) {
            const PlaneStack a{200, 40, 17, "a"}, b{pb, 48, 9, "b"};
            missed += overlap_by_bytes(a, b, 3) && !plane_stacks_overlap(a, b, 3);
            const bool whole = ranges_overlap(200, 2 * 40 + 17, pb, 2 * 48 + 9);
            missed += plane_stacks_overlap(a, b, 3) != whole;
        }
        expect(missed == 0, "two image strides: the whole extents");
        const PlaneStack a{200, 40, 17, "a"}, none{0, 40, 17, "none"}, empty{200, 40, 0, "empty"};
        expect(!plane_stacks_overlap(a, none, 3) && !plane_stacks_overlap(empty, a, 3) && plane_stacks_overlap(a, a, 1),
               "absent planes share nothing; a plane shares itself");
        const PlaneStack top{UINTPTR_MAX - 99, 40, 20, "top"}, below{UINTPTR_MAX - 139, 40, 40, "below"};
        expect(!plane_stacks_overlap(top, below, 1) && plane_stacks_overlap(top, below, 2) &&
                   !plane_stacks_overlap(top, PlaneStack{UINTPTR_MAX - 19, 40, 20, "after"}, 1),
               "planes at the top of the address space");
    }

    // a whole NV12 buffer of 3 images of 20 x 4, rows 32 apart: the planes lie in each other's extents
    {
        Yuv420Layout l{};
        check_yuv420_layout(3, 20, 4, 2, 32, 192, 32, 192, &l);
        const uintptr_t y = 0x10000, cb = y + 32 * 4, cr = cb + 1;
        PlaneStack r[4] = {{0x90000, 20 * 3 * 4, 3 * 20 * 3 + 60, "src"}, {y, l.y_image_stride, l.y_bytes, "y"}};
        expect(yuv420_chroma_planes(cb, cr, 2, l, r + 2) == 1 && r[2].p == cb && r[2].image_bytes == l.c_bytes + 1 &&
                   r[2].image_bytes == 32 + 20,
               "NV12: Cb and Cr are one plane");
        PairMessage why;
        expect(check_plane_stacks(r, 1, 3, 3, &why) == nullptr, "NV12 surfaces of one buffer are accepted");
        PlaneStack nv21[1];
        expect(yuv420_chroma_planes(cr, cb, 2, l, nv21) == 1 && nv21[0].p == cb, "NV21: the plane begins at the lower pointer");
        // the chroma plane one byte earlier meets the last Y sample of every image ... only if that byte is a sample:
        // rows are 32 apart and 20 long, so the Y plane's last sample is 12 bytes before the chroma
        r[2].p = cb - 12;
        expect(check_plane_stacks(r, 1, 3, 3, &why) == nullptr, "chroma right after the last Y sample");
        r[2].p = cb - 13;
        const char* msg = check_plane_stacks(r, 1, 3, 3, &why);
        expect(msg && !std::strcmp(msg, "y and cb/cr overlap"), "chroma over the last Y sample, by name");
        // past its own image into the next one's Y plane
        r[2].p = y + 192 - (32 + 20) + 1;
        expect(check_plane_stacks(r, 1, 3, 3, &why) != nullptr, "chroma reaching the next image's Y plane");
        r[2].p = y + 192 - (32 + 20);
        expect(check_plane_stacks(r, 1, 3, 3, &why) == nullptr, "chroma ending where the next image begins");
        // an output over the input
        r[2].p = cb;
        r[0].p = y + 3 * 192 - 1 - 12;  // the last chroma sample of the last image
        msg = check_plane_stacks(r, 1, 3, 3, &why);
        expect(msg && !std::strcmp(msg, "cb/cr and src overlap"), "src over the last chroma sample");
        r[0].p = y + 3 * 192 - 12;
        expect(check_plane_stacks(r, 1, 3, 3, &why) == nullptr, "src right after the surface's last sample");
        // inputs may share: the same list with everything read and only src written is judged by src alone
        const PlaneStack in[3] = {r[1], r[1], {0x90000, 240, 240, "dst"}};
        expect(check_plane_stacks(in, 2, 3, 3, &why) == nullptr, "two inputs may be one buffer");
    }
    // I420 / YV12: two planes; interleaved samples that are not neighbours are two planes too
    {
        Yuv420Layout l{};
        check_yuv420_layout(2, 20, 4, 1, 0, 120, 0, 120, &l);
        const uintptr_t y = 0x20000, cb = y + 80, cr = cb + 20;
        PlaneStack r[3] = {{y, 120, l.y_bytes, "y"}};
        expect(yuv420_chroma_planes(cb, cr, 1, l, r + 1) == 2 && r[1].p == cb && r[2].p == cr && r[1].image_bytes == 20,
               "I420: two planes");
        PairMessage why;
        expect(check_plane_stacks(r, 0, 3, 2, &why) == nullptr, "I420 surfaces of one buffer are accepted");
        yuv420_chroma_planes(cb, cr - 1, 1, l, r + 1);
        const char* msg = check_plane_stacks(r, 0, 3, 2, &why);
        expect(msg && !std::strcmp(msg, "cb and cr overlap"), "Cr beginning on the last Cb sample");
        yuv420_chroma_planes(cb, cb + 1, 1, l, r + 1);
        expect(r[1].image_bytes == 20 && check_plane_stacks(r, 0, 3, 2, &why) != nullptr,
               "planar Cb and Cr one byte apart are not one plane");
        check_yuv420_layout(2, 20, 4, 2, 0, 120, 0, 120, &l);
        expect(yuv420_chroma_planes(cb, cb + 2, 2, l, r + 1) == 2 && check_plane_stacks(r, 0, 3, 2, &why) != nullptr,
               "interleaved samples two bytes apart are two planes that share bytes");
        expect(yuv420_chroma_planes(0, 0, 2, l, r + 1) == 2 && r[1].image_bytes == 0 && r[2].image_bytes == 0 &&
                   check_plane_stacks(r, 0, 3, 2, &why) == nullptr,
               "absent chroma (a gray target)");
    }
    far::yuv(&failures);  // the far cases (far_cases.h)
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
