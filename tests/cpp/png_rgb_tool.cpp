// Test harness for the colour side of the CLI's PNG codec (cli/png.hpp):
//   png_rgb_tool rgb IN.png OUT.raw      -> png::read_rgb's 8-bit RGB bytes (int32 w, h header)
//   png_rgb_tool write W H IN.raw OUT.png -> png::write_rgb of RGB bytes
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "png.hpp"

int main(int argc, char** argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "rgb" && argc == 4) {
            const png::Rgb g = png::read_rgb(argv[2]);
            FILE* f = std::fopen(argv[3], "wb");
            if (!f) return 2;
            std::fwrite(&g.width, 4, 1, f);
            std::fwrite(&g.height, 4, 1, f);
            std::fwrite(g.px.data(), 1, g.px.size(), f);
            std::fclose(f);
            return 0;
        }
        if (mode == "write" && argc == 6) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
            std::vector<uint8_t> d((size_t)w * h * 3);
            FILE* f = std::fopen(argv[4], "rb");
            if (!f || std::fread(d.data(), 1, d.size(), f) != d.size()) return 2;
            std::fclose(f);
            png::write_rgb(argv[5], d.data(), w, h);
            return 0;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 3;
}
