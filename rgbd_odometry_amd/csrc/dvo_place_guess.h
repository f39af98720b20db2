/*
 * dvo_place_guess.h -- the arithmetic of dvo_tracker_place_guess (include/dvo_amd.h): a shift of the descriptor level as a rotation.
 * Host code in double, nothing of HIP: dvo_capi_tracker_places.cpp calls it, tests/host/place_guess_main.cpp runs it without a device.
 */
#ifndef DVO_PLACE_GUESS_H_
#define DVO_PLACE_GUESS_H_

#include <cmath>

namespace dvo_host {

/* fx, fy: the stream's intrinsics at camera resolution; level_shift = first_shift + the places level.  a = (dx / fx_L, dy / fy_L, 1) is
 * the ray of the level's pixel (cx_L + dx, cy_L + dy), d = a / |a|, v = d x e3 = (d_y, -d_x, 0);  R0 = I + [v]x + [v]x^2 / (1 + d_z) is
 * the smallest rotation with R0 d = e3 (column-major), t0 = 0 */
inline void place_guess(float fx, float fy, int level_shift, int dy, int dx, double *R0, double *t0) {
    const double sc = std::ldexp(1.0, -level_shift);
    const double ax = (double)dx / ((double)fx * sc), ay = (double)dy / ((double)fy * sc);
    const double nrm = std::sqrt(ax * ax + ay * ay + 1.0);
    const double d[3] = {ax / nrm, ay / nrm, 1.0 / nrm};
    const double V[3][3] = {{0.0, 0.0, -d[0]}, {0.0, 0.0, -d[1]}, {d[0], d[1], 0.0}};
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) {
            double v2 = 0.0;
            for (int k = 0; k < 3; k++) v2 += V[r][k] * V[k][q];
            R0[q * 3 + r] = (r == q ? 1.0 : 0.0) + V[r][q] + v2 / (1.0 + d[2]);
        }
    t0[0] = t0[1] = t0[2] = 0.0;
}

}  // namespace dvo_host
#endif
