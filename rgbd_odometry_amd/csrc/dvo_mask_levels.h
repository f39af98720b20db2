/*
 * dvo_mask_levels.h -- per-level keep planes of an ignore mask (include/dvo_amd.h, "ignore masks"): the definition, in plain C++.
 * No device, no context, no other header of the library: dvo_mask_levels_host is build() below, the device builder
 * (dvo_frame_masks.hip) shares level_size() and footprint() with it, and a stand-alone program can include the file as it is.
 *
 * A mask is rows x cols bytes, row-major, non-zero = "ignore this pixel".  Level l (s = first_shift + l) is rows_l x cols_l, the
 * engine's cvRound sizes.  Level pixel (y, x) stands for the camera pixels Y in [y 2^s, (y+1) 2^s), X in [x 2^s, (x+1) 2^s), clipped
 * to the image; where the clipping leaves nothing (a level size that was rounded up) it stands for the clamped pixel rows - 1 /
 * cols - 1.  The first pixel of that block is the pixel the INTER_NEAREST pyramid samples.
 *   drop0(y, x) = some mask byte of the footprint is non-zero
 *   drop(y, x)  = some drop0(y', x') with |y - y'| <= margin and |x - x'| <= margin inside the level (Chebyshev dilation)
 *   keep(y, x)  = drop ? 0 : 255, stored column-major (y + x * rows_l) like every plane of the frame store
 */
#ifndef DVO_MASK_LEVELS_H_
#define DVO_MASK_LEVELS_H_

#include <stddef.h>
#include <vector>

#if defined(__HIPCC__)
#define DVO_MASK_HD __host__ __device__ inline
#else
#define DVO_MASK_HD inline
#endif

namespace dvo_mask {

constexpr int kMaxLevels = 8;      /* == DVO_MAX_LEVELS */
constexpr int kMaxMargin = 8;      /* == DVO_MASK_MAX_MARGIN */

/* cvRound(n * 2^-shift) for n >= 0: round half to even, in integers */
DVO_MASK_HD int level_size(int n, int shift) {
    if (shift <= 0) return n;
    if (shift >= 32) return 0;                             /* n < 2^31: below one half */
    const long long q = (long long)n >> shift, r = (long long)n & ((1LL << shift) - 1), half = 1LL << (shift - 1);
    return (int)(q + ((r > half || (r == half && (q & 1))) ? 1 : 0));
}

/* camera pixels [lo, hi) along one axis of length n that level coordinate v stands for at shift s (s < 31) */
DVO_MASK_HD void footprint(int v, int s, int n, int *lo, int *hi) {
    const long long a = (long long)v << s, b = ((long long)v + 1) << s;
    if (a >= n) { *lo = n - 1; *hi = n; return; }
    *lo = (int)a;
    *hi = (int)(b < n ? b : (long long)n);
}

/* the level sizes; false for arguments every mask entry point refuses */
inline bool geometry(int rows, int cols, int n_levels, int first_shift, int margin, int *level_rows, int *level_cols) {
    if (rows < 1 || cols < 1 || n_levels < 1 || n_levels > kMaxLevels || first_shift < 0 || margin < 0 || margin > kMaxMargin) return false;
    for (int l = 0; l < n_levels; l++) {
        const int r = level_size(rows, first_shift + l), c = level_size(cols, first_shift + l);
        if (r < 1 || c < 1) return false;                  /* an empty level (this also bounds the shift below 31) */
        if (level_rows) level_rows[l] = r;
        if (level_cols) level_cols[l] = c;
    }
    return true;
}

/* keep_out[l]: level_rows[l] * level_cols[l] bytes.  False: refused, nothing written */
inline bool build(int rows, int cols, const unsigned char *mask, int n_levels, int first_shift, int margin, unsigned char *const *keep_out,
                  int *level_rows, int *level_cols) {
    int lr[kMaxLevels], lc[kMaxLevels];
    if (!mask || !keep_out || !geometry(rows, cols, n_levels, first_shift, margin, lr, lc)) return false;
    for (int l = 0; l < n_levels; l++)
        if (!keep_out[l]) return false;
    std::vector<unsigned char> d0, d1;
    for (int l = 0; l < n_levels; l++) {
        const int s = first_shift + l, R = lr[l], C = lc[l];
        d0.assign((size_t)R * C, 0);
        d1.assign((size_t)R * C, 0);
        for (int y = 0; y < R; y++) {
            int y0, y1;
            footprint(y, s, rows, &y0, &y1);
            for (int x = 0; x < C; x++) {
                int x0, x1;
                footprint(x, s, cols, &x0, &x1);
                unsigned char any = 0;
                for (int Y = y0; Y < y1 && !any; Y++)
                    for (int X = x0; X < x1; X++)
                        if (mask[(size_t)Y * cols + X]) { any = 1; break; }
                d0[(size_t)y + (size_t)x * R] = any;
            }
        }
        for (int x = 0; x < C; x++)                        /* the square window is separable: along the rows, then along the columns */
            for (int y = 0; y < R; y++) {
                unsigned char any = 0;
                for (int yy = (y - margin > 0 ? y - margin : 0); yy <= y + margin && yy < R; yy++) any |= d0[(size_t)yy + (size_t)x * R];
                d1[(size_t)y + (size_t)x * R] = any;
            }
        for (int x = 0; x < C; x++)
            for (int y = 0; y < R; y++) {
                unsigned char any = 0;
                for (int xx = (x - margin > 0 ? x - margin : 0); xx <= x + margin && xx < C; xx++) any |= d1[(size_t)y + (size_t)xx * R];
                keep_out[l][(size_t)y + (size_t)x * R] = any ? 0 : 255;
            }
        if (level_rows) level_rows[l] = R;
        if (level_cols) level_cols[l] = C;
    }
    return true;
}

}  // namespace dvo_mask
#endif
