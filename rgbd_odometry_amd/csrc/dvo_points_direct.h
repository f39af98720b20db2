/* The direct 4-byte form of a reference point: { pixel column | pixel row << 10 | depth in whole millimetres << 19 }.
 *
 * The fused kernel's workgroups turn the block-relative 4-byte points of a level (dvo_device_math.h: pt4_decode) into this form once,
 * while they stage the list into LDS; the level's sweeps then decode a point without block arithmetic and without chunk headers
 * (dvo_fused.hip: pt4d_decode2).  The form lives in LDS only: no stored format changes.
 *
 * Field widths are compile-time constants (a vector instruction of gfx950 reads one scalar register: run-time widths would cost
 * what the form saves).  A list with a point outside them keeps the block-relative form in LDS.
 *
 * Only the integer helpers live here, so that a host program can compile them (tests/host/points_direct_main.cpp). */
#ifndef DVO_POINTS_DIRECT_H_
#define DVO_POINTS_DIRECT_H_

#if defined(__HIPCC__)
#define DVO_PT4D_FN __host__ __device__ inline
#else
#define DVO_PT4D_FN inline
#endif

namespace dvo {

enum : unsigned {
    PT4D_X_BITS = 10,                               /* pixel column: levels of at most 1024 columns */
    PT4D_Y_BITS = 9,                                /* pixel row: at most 512 rows */
    PT4D_D_BITS = 13,                               /* depth: below 8192 mm */
    PT4D_Y_SHIFT = PT4D_X_BITS,
    PT4D_D_SHIFT = PT4D_X_BITS + PT4D_Y_BITS,
    PT4D_MAX_COLS = 1u << PT4D_X_BITS,
    PT4D_MAX_ROWS = 1u << PT4D_Y_BITS,
    PT4D_MAX_DEPTH = 1u << PT4D_D_BITS              /* first depth (mm) the form cannot hold */
};
static_assert(PT4D_X_BITS + PT4D_Y_BITS + PT4D_D_BITS == 32, "one 32-bit word");

DVO_PT4D_FN bool pt4d_fits(unsigned xx, unsigned yy, unsigned d) {
    return xx < PT4D_MAX_COLS && yy < PT4D_MAX_ROWS && d < PT4D_MAX_DEPTH;
}
/* only for values that fit */
DVO_PT4D_FN unsigned pt4d_pack(unsigned xx, unsigned yy, unsigned d) {
    return xx | (yy << PT4D_Y_SHIFT) | (d << PT4D_D_SHIFT);
}
DVO_PT4D_FN void pt4d_unpack(unsigned w, unsigned &xx, unsigned &yy, unsigned &d) {
    xx = w & (PT4D_MAX_COLS - 1u);
    yy = (w >> PT4D_Y_SHIFT) & (PT4D_MAX_ROWS - 1u);
    d = w >> PT4D_D_SHIFT;
}

}  // namespace dvo

#endif
