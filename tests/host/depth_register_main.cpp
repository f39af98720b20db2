/*
 * depth_register_main.cpp -- dvo_depth::build (rgbd_odometry_amd/csrc/dvo_depth_register.h: the body of dvo_depth_register_host) as a
 * stand-alone program, so that tests/test_depth_register_cpu.py can run it under the address and undefined-behaviour sanitizers.
 *
 *   depth_register_main RIG_FILE DEPTH_FILE FORMAT ROWS COLS
 *
 * RIG_FILE: the bytes of one dvo_depth_rig.  DEPTH_FILE: depth_rows * depth_cols raw values, row-major, FORMAT 0 = float metres,
 * 1 = 16-bit millimetres.  Output: one line "image rows cols", then rows * cols pixels as four hex digits each, row-major, on one line.
 * Exit status 3: the arguments were refused (and nothing but "refused" is printed; the output buffer is checked to be untouched).
 * The depth image and the output are allocated to their exact sizes, so that an access past either end is the sanitizer's to see.
 */
#include "dvo_depth_register.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

int main(int argc, char **argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s rig_file depth_file format rows cols\n", argv[0]); return 2; }
    const int format = std::atoi(argv[3]), rows = std::atoi(argv[4]), cols = std::atoi(argv[5]);
    dvo_depth_rig rig;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f || std::fread(&rig, 1, sizeof(rig), f) != sizeof(rig)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        std::fclose(f);
    }
    const size_t bpp = format == dvo_depth::kFormatU16 ? 2 : 4;
    const size_t dpx = (rig.depth_rows >= 1 && rig.depth_cols >= 1) ? (size_t)rig.depth_rows * (size_t)rig.depth_cols : 1;
    std::unique_ptr<unsigned char[]> depth(new unsigned char[dpx * bpp]);
    std::memset(depth.get(), 0, dpx * bpp);
    const bool known = format == dvo_depth::kFormatU16 || format == dvo_depth::kFormatF32;      /* else: refused below, nothing to read */
    if (known && rig.depth_rows >= 1 && rig.depth_cols >= 1) {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f || std::fread(depth.get(), 1, dpx * bpp, f) != dpx * bpp) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        std::fclose(f);
    }
    const size_t npx = (rows >= 1 && cols >= 1) ? (size_t)rows * (size_t)cols : 1;
    std::unique_ptr<unsigned short[]> out(new unsigned short[npx]);
    for (size_t i = 0; i < npx; i++) out[i] = 0xABCD;
    if (!dvo_depth::build(&rig, depth.get(), format, rows, cols, out.get())) {
        for (size_t i = 0; i < npx; i++)
            if (out[i] != 0xABCD) { std::fprintf(stderr, "a refused call wrote its output\n"); return 4; }
        std::printf("refused\n");
        return 3;
    }
    std::printf("image %d %d\n", rows, cols);
    for (size_t i = 0; i < npx; i++) std::printf("%04x", out[i]);
    std::printf("\n");
    return 0;
}
