/* The arithmetic of dvo_tracker_place_guess (rgbd_odometry_amd/csrc/dvo_place_guess.h) without a device: for the intrinsics and the
 * level shift of the command line, one line per shift of [-r, r]^2 -- dy dx, the nine entries of R0 (column-major) and t0, as
 * hexadecimal doubles.  tests/test_tracker_place_shift_cpu.py compares them with the numpy restatement. */
#include <cstdio>
#include <cstdlib>

#include "dvo_place_guess.h"

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s fx fy level_shift radius\n", argv[0]); return 2; }
    const float fx = (float)std::atof(argv[1]), fy = (float)std::atof(argv[2]);
    const int shift = std::atoi(argv[3]), r = std::atoi(argv[4]);
    for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++) {
            double R0[9], t0[3] = {1.0, 1.0, 1.0};
            dvo_host::place_guess(fx, fy, shift, dy, dx, R0, t0);
            std::printf("%d %d", dy, dx);
            for (double v : R0) std::printf(" %a", v);
            for (double v : t0) std::printf(" %a", v);
            std::printf("\n");
        }
    return 0;
}
