// luma_check.cpp -- the CLI's host luma (cli/png.hpp, png::detail::luma) against
// a table of all 2^24 (R, G, B) values that tests/lumaref.py wrote: byte
// (r << 16 | g << 8 | b) of the file is lumaref's gray of that colour.
//   luma_check TABLE   -> "<k> mismatches", exit 0 when k == 0
#include <cstdio>
#include <vector>

#include "png.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 3;
    std::vector<uint8_t> table;
    try {
        table = png::detail::read_file(argv[1]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    if (table.size() != (size_t)1 << 24) {
        std::fprintf(stderr, "table holds %zu bytes, not 2^24\n", table.size());
        return 2;
    }
    long long bad = 0;
    for (int r = 0; r < 256; ++r)
        for (int g = 0; g < 256; ++g)
            for (int b = 0; b < 256; ++b) {
                const uint8_t want = table[(size_t)r << 16 | (size_t)g << 8 | (size_t)b];
                if (png::detail::luma(r, g, b) != want && bad++ < 5)
                    std::printf("(%d, %d, %d): png %d, table %d\n", r, g, b, png::detail::luma(r, g, b), want);
            }
    std::printf("%lld mismatches\n", bad);
    return bad ? 1 : 0;
}
