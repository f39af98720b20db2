/*
 * mask_levels_main.cpp -- dvo_mask::build (rgbd_odometry_amd/csrc/dvo_mask_levels.h: the body of dvo_mask_levels_host) as a stand-alone
 * program, so that tests/test_frame_masks_cpu.py can run it under the address and undefined-behaviour sanitizers.
 *
 *   mask_levels_main MASK_FILE ROWS COLS N_LEVELS FIRST_SHIFT MARGIN
 *
 * MASK_FILE: rows * cols bytes, row-major.  Output: per level a line "level l rows cols" followed by rows * cols bytes of the plane as
 * two hex digits each, column-major, on one line.  Exit status 3: the arguments were refused (and nothing but "refused" is printed).
 * Every plane is allocated to its exact size, so that a write past a level's end is the sanitizer's to see.
 */
#include "dvo_mask_levels.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s mask_file rows cols n_levels first_shift margin\n", argv[0]); return 2; }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n_levels = std::atoi(argv[4]), first_shift = std::atoi(argv[5]),
              margin = std::atoi(argv[6]);
    std::vector<unsigned char> mask;
    if (rows >= 1 && cols >= 1) {
        mask.resize((size_t)rows * cols);
        FILE *f = std::fopen(argv[1], "rb");
        if (!f || std::fread(mask.data(), 1, mask.size(), f) != mask.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        std::fclose(f);
    }
    int lr[dvo_mask::kMaxLevels], lc[dvo_mask::kMaxLevels];
    if (!dvo_mask::geometry(rows, cols, n_levels, first_shift, margin, lr, lc)) { std::printf("refused\n"); return 3; }
    std::vector<std::unique_ptr<unsigned char[]>> planes;
    std::vector<unsigned char *> keep;
    for (int l = 0; l < n_levels; l++) {
        planes.emplace_back(new unsigned char[(size_t)lr[l] * lc[l]]);
        keep.push_back(planes.back().get());
    }
    int r2[dvo_mask::kMaxLevels], c2[dvo_mask::kMaxLevels];
    if (!dvo_mask::build(rows, cols, mask.data(), n_levels, first_shift, margin, keep.data(), r2, c2)) { std::printf("refused\n"); return 3; }
    for (int l = 0; l < n_levels; l++) {
        if (r2[l] != lr[l] || c2[l] != lc[l]) { std::fprintf(stderr, "level sizes disagree\n"); return 4; }
        std::printf("level %d %d %d\n", l, lr[l], lc[l]);
        for (size_t i = 0; i < (size_t)lr[l] * lc[l]; i++) std::printf("%02x", keep[l][i]);
        std::printf("\n");
    }
    return 0;
}
