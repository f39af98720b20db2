/*
 * points_direct_main.cpp -- the integer helpers of the direct 4-byte point form (rgbd_odometry_amd/csrc/dvo_points_direct.h: pt4d_fits,
 * pt4d_pack, pt4d_unpack) as a stand-alone program, so that tests/test_points_direct_cpu.py can run them under the address and
 * undefined-behaviour sanitizers.
 *
 *   points_direct_main
 *
 * Packs and unpacks every depth below 8192 mm at a grid of pixels that includes the corners (0 / 1023, 0 / 511), checks that the three
 * fields never overlap (the packed word is the sum of its fields, and changing one field changes no other), and that refusal happens
 * exactly at d = 8192, xx = 1024, yy = 512.  Prints "ok <words checked>" and exits 0, or the first failure and exits 1.
 */
#include "dvo_points_direct.h"

#include <cstdio>
#include <vector>

static int fail(const char *what, unsigned xx, unsigned yy, unsigned d) {
    std::printf("FAILED %s at xx=%u yy=%u d=%u\n", what, xx, yy, d);
    return 1;
}

int main() {
    using namespace dvo;
    if (PT4D_MAX_COLS != 1024u || PT4D_MAX_ROWS != 512u || PT4D_MAX_DEPTH != 8192u) return fail("field widths", PT4D_MAX_COLS, PT4D_MAX_ROWS, PT4D_MAX_DEPTH);
    std::vector<unsigned> xs, ys;
    for (unsigned x = 0; x < PT4D_MAX_COLS; x += 37) xs.push_back(x);
    for (unsigned x : {1u, 15u, 16u, 511u, 512u, 1022u, 1023u}) xs.push_back(x);
    for (unsigned y = 0; y < PT4D_MAX_ROWS; y += 29) ys.push_back(y);
    for (unsigned y : {1u, 15u, 16u, 255u, 256u, 510u, 511u}) ys.push_back(y);
    unsigned long long n = 0;
    for (unsigned xx : xs)
        for (unsigned yy : ys)
            for (unsigned d = 0; d < PT4D_MAX_DEPTH; d++) {
                if (!pt4d_fits(xx, yy, d)) return fail("fits refused a value inside the fields", xx, yy, d);
                const unsigned w = pt4d_pack(xx, yy, d);
                if (w != xx + (yy << 10) + (d << 19)) return fail("packed word is not column | row << 10 | depth << 19", xx, yy, d);
                unsigned x2 = ~0u, y2 = ~0u, d2 = ~0u;
                pt4d_unpack(w, x2, y2, d2);
                if (x2 != xx || y2 != yy || d2 != d) return fail("unpack(pack) is not the identity", xx, yy, d);
                n++;
            }
    /* refusal exactly at the first value past each field, whatever the other two are */
    for (unsigned xx : {0u, 1023u})
        for (unsigned yy : {0u, 511u})
            for (unsigned d : {0u, 8191u}) {
                if (!pt4d_fits(xx, yy, d)) return fail("corner refused", xx, yy, d);
                if (pt4d_fits(1024u, yy, d) || pt4d_fits(xx, 512u, d) || pt4d_fits(xx, yy, 8192u)) return fail("first value past a field accepted", xx, yy, d);
                if (pt4d_fits(~0u, yy, d) || pt4d_fits(xx, ~0u, d) || pt4d_fits(xx, yy, ~0u) || pt4d_fits(xx, yy, 65535u)) return fail("large value accepted", xx, yy, d);
            }
    for (unsigned v = 0; v < 70000; v++) {
        if (pt4d_fits(v, 0, 0) != (v < 1024u)) return fail("column bound", v, 0, 0);
        if (pt4d_fits(0, v, 0) != (v < 512u)) return fail("row bound", 0, v, 0);
        if (pt4d_fits(0, 0, v) != (v < 8192u)) return fail("depth bound", 0, 0, v);
    }
    std::printf("ok %llu\n", n);
    return 0;
}
