// test_yuv.cpp -- the C++ facade's 4:2:0 entries (include/dis/dis.hpp:
// dis::Yuv420 and its makers, dis::framesToYuv420, dis::yuv420ToFrames) on host
// buffers, against hand values. Built and run by tests/test_gpu_yuv.py.
#include <cstdio>
#include <vector>

#include "dis/dis.hpp"

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++failures;
    }
}

int main()
{
    const int W = 20, H = 4, n = 2;
    // the views: where the planes of one buffer lie
    {
        uint8_t* const p = reinterpret_cast<uint8_t*>(0x1000);
        const dis::Yuv420 a = dis::Yuv420::nv12(p, W, H), b = dis::Yuv420::nv21(p, W, H, 32), c = dis::Yuv420::i420(p, W, H),
                          d = dis::Yuv420::yv12(p, W, H, 32);
        expect(a.y == p && a.cb == p + 80 && a.cr == p + 81 && a.c_step == 2 && a.y_stride == 20 && a.c_stride == 20 &&
                   a.y_image_stride == 120 && a.c_image_stride == 120,
               "nv12 view");
        expect(b.cr == p + 128 && b.cb == p + 129 && b.c_step == 2 && b.y_stride == 32 && b.c_stride == 32 &&
                   b.y_image_stride == 192,
               "nv21 view with a stride");
        expect(c.cb == p + 80 && c.cr == p + 100 && c.c_step == 1 && c.c_stride == 10 && c.c_image_stride == 120, "i420 view");
        expect(d.cr == p + 128 && d.cb == p + 128 + 32 && d.c_stride == 16 && d.y_image_stride == 192, "yv12 view with a stride");
    }
    try {
        // pure red (BGR), BT.601 full: (Y, Cb, Cr) = (76, 85, 255); image 1 is white: (255, 128, 128)
        std::vector<uint8_t> bgr(n * W * H * 3, 0);
        for (int i = 0; i < W * H; ++i) bgr[3 * i + 2] = 255;
        for (int i = W * H * 3; i < 2 * W * H * 3; ++i) bgr[i] = 255;
        for (int planar = 0; planar < 2; ++planar) {
            std::vector<uint8_t> surf(n * W * H * 3 / 2, 7);
            const dis::Yuv420 v = planar ? dis::Yuv420::i420(surf.data(), W, H) : dis::Yuv420::nv12(surf.data(), W, H);
            dis::framesToYuv420(bgr.data(), dis::FrameFormat::BGR8, n, v, dis::YuvMatrix::BT601, dis::YuvRange::FULL);
            bool ok = true;
            for (int k = 0; k < n; ++k) {
                const uint8_t* const s = surf.data() + k * W * H * 3 / 2;
                for (int i = 0; i < W * H; ++i) ok = ok && s[i] == (k ? 255 : 76);
                for (int i = 0; i < W * H / 4; ++i) {
                    const uint8_t cb = planar ? s[W * H + i] : s[W * H + 2 * i];
                    const uint8_t cr = planar ? s[W * H + W * H / 4 + i] : s[W * H + 2 * i + 1];
                    ok = ok && cb == (k ? 128 : 85) && cr == (k ? 128 : 255);
                }
            }
            expect(ok, planar ? "framesToYuv420, i420" : "framesToYuv420, nv12");
            // and back, as RGBA with alpha 9: red comes back within 1 (full range), white exactly
            std::vector<uint8_t> rgba(n * W * H * 4, 0);
            dis::yuv420ToFrames(v, n, rgba.data(), dis::FrameFormat::RGBA8, dis::YuvMatrix::BT601, dis::YuvRange::FULL, 9);
            ok = true;
            for (int i = 0; i < W * H; ++i) {
                const uint8_t* const a = rgba.data() + 4 * i;
                const uint8_t* const b = rgba.data() + 4 * (W * H + i);
                ok = ok && a[0] >= 254 && a[1] <= 1 && a[2] <= 1 && a[3] == 9;
                ok = ok && b[0] == 255 && b[1] == 255 && b[2] == 255 && b[3] == 9;
            }
            expect(ok, planar ? "yuv420ToFrames, i420" : "yuv420ToFrames, nv12");
        }
        // limited range: (16, 128, 128) is black, (235, 128, 128) white; a gray target needs no chroma
        std::vector<uint8_t> surf(W * H * 3 / 2, 128), out(W * H * 3, 1), gray(W * H, 1);
        for (int i = 0; i < W * H; ++i) surf[i] = i < W * H / 2 ? 16 : 235;
        dis::yuv420ToFrames(dis::Yuv420::nv12(surf.data(), W, H), 1, out.data(), dis::FrameFormat::BGR8);
        bool ok = true;
        for (int i = 0; i < W * H * 3; ++i) ok = ok && out[i] == (i < W * H * 3 / 2 ? 0 : 255);
        expect(ok, "limited black and white");
        dis::Yuv420 luma = dis::Yuv420::nv12(surf.data(), W, H);
        luma.cb = luma.cr = nullptr;
        dis::yuv420ToFrames(luma, 1, gray.data(), dis::FrameFormat::GRAY8);
        ok = true;
        for (int i = 0; i < W * H; ++i) ok = ok && gray[i] == (i < W * H / 2 ? 0 : 255);
        expect(ok, "gray target without chroma");
        // refusals surface as dis::Error
        bool threw = false;
        try {
            dis::yuv420ToFrames(dis::Yuv420::nv12(surf.data(), W - 1, H), 1, out.data(), dis::FrameFormat::BGR8);
        } catch (const dis::Error& e) {
            threw = e.status() == DIS_ERR_INVALID_ARGUMENT;
        }
        expect(threw, "an odd width is refused");
    } catch (const dis::Error& e) {
        std::printf("FAIL: dis::Error %d: %s\n", (int)e.status(), e.what());
        ++failures;
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
