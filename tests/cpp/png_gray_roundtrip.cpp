// The CLI's 8-bit grey PNG encoder (cli/png.hpp write_gray, the --bidir mask)
// through its own decoder: argv[1] = a file to write. Compiled and run by
// tests/test_bidir_host.py; exits non-zero on any difference.
#include <cstdio>

#include "png.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const int sizes[][2] = {{1, 1}, {5, 3}, {160, 96}, {67, 33}};
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        std::vector<uint8_t> px((size_t)w * h);
        for (size_t i = 0; i < px.size(); ++i) px[i] = (i % 7 == 0) ? 255 : (uint8_t)((i * 37) & (i % 3 ? 0 : 255));
        png::write_gray(argv[1], px.data(), w, h);
        const png::Gray g = png::read_gray(argv[1]);
        if (g.width != w || g.height != h || g.px != px) {
            std::printf("FAIL: %d x %d\n", w, h);
            return 1;
        }
    }
    std::printf("OK\n");
    return 0;
}
