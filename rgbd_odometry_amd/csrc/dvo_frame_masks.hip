/*
 * dvo_frame_masks.hip -- per-pair ignore masks of the frame stage (include/dvo_amd.h, "ignore masks"; host side dvo_capi_frames.cpp).
 *
 * Two kernels, neither of which touches Canny, the distance transform or the alignment:
 *   mask_levels_kernel       a camera-resolution mask -> the keep planes of every pyramid level, ONE launch (dvo_frames_set_pair_mask,
 *                            never per frame).  A workgroup owns a 16 x 16 tile of one level: it ORs the footprints of the tile and of a
 *                            halo of `margin` level pixels into LDS (drop0), then every thread takes the OR over its (2 margin + 1)^2 window.
 *                            level_size() and footprint() are the host builder's own (dvo_mask_levels.h): the planes are byte-equal to
 *                            dvo_mask_levels_host.
 *   edge_mask_levels_kernel  the per-tick path: edge &= keep in the frame store, ONE launch for all levels and all images of a chunk,
 *                            between Canny and the now-level stage.  The grid is the concatenation of the levels' grids (as the
 *                            *_levels_kernel's of dvo_frames.hip), blockIdx.y is the image.  The image's keep plane comes from the device
 *                            table of its pair; a pair without a mask ends its workgroups at once.
 *
 * Every index is bounded by the sizes the host passes.
 */
#include "dvo_launch.h"
#include "dvo_mask_levels.h"

namespace dvo {

namespace {

constexpr int MT = 16;                                           /* tile edge of the builder, in level pixels */
constexpr int MW = MT + 2 * dvo_mask::kMaxMargin;                /* ... with its halo */
constexpr int EM_BLOCK = 256;
constexpr size_t EM_BYTES = (size_t)EM_BLOCK * 16;               /* edge bytes per workgroup: one 16-byte word per thread */

struct MaskLevels {
    int n, rows, cols, margin;
    int shift[DVO_LEVELS], lrows[DVO_LEVELS], lcols[DVO_LEVELS];
    unsigned first[DVO_LEVELS + 1];
    unsigned char *keep[DVO_LEVELS];
};
struct EdgeMaskLevels {
    int n;
    unsigned first[DVO_LEVELS + 1];
    unsigned char *edge[DVO_LEVELS];
    size_t stride[DVO_LEVELS], npx[DVO_LEVELS];
    const unsigned char *const *tab;                             /* image i, level l: tab[i * DVO_LEVELS + l], NULL = no mask */
};

DVO_DEV int mask_level_of_block(const unsigned *first, int n, unsigned bx) {
    int l = 0;
    while (l + 1 < n && bx >= first[l + 1]) l++;
    return l;
}

}  // namespace

__global__ void __launch_bounds__(MT * MT)
mask_levels_kernel(const unsigned char *__restrict__ mask, const MaskLevels t) {
    __shared__ unsigned char d0[MW * MW];
    const int l = mask_level_of_block(t.first, t.n, blockIdx.x);
    const int R = t.lrows[l], C = t.lcols[l], s = t.shift[l], m = t.margin;
    const int tiles_y = (R + MT - 1) / MT;
    const int tb = (int)(blockIdx.x - t.first[l]);
    const int y0 = (tb % tiles_y) * MT, x0 = (tb / tiles_y) * MT;
    const int W = MT + 2 * m;
    for (int i = threadIdx.x; i < W * W; i += MT * MT) {
        const int y = y0 - m + i % W, x = x0 - m + i / W;
        unsigned char any = 0;
        if (y >= 0 && y < R && x >= 0 && x < C) {
            int ya, yb, xa, xb;
            dvo_mask::footprint(y, s, t.rows, &ya, &yb);
            dvo_mask::footprint(x, s, t.cols, &xa, &xb);
            for (int Y = ya; Y < yb && !any; Y++)
                for (int X = xa; X < xb; X++)
                    if (mask[(size_t)Y * t.cols + X]) { any = 1; break; }
        }
        d0[i] = any;
    }
    __syncthreads();
    const int ly = threadIdx.x % MT, lx = threadIdx.x / MT;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= R || x >= C) return;
    unsigned char any = 0;
    for (int hx = lx; hx <= lx + 2 * m; hx++)                    /* halo entries outside the level are zero */
        for (int hy = ly; hy <= ly + 2 * m; hy++) any |= d0[hy + hx * W];
    t.keep[l][(size_t)y + (size_t)x * R] = any ? 0 : 255;
}

__global__ void __launch_bounds__(EM_BLOCK)
edge_mask_levels_kernel(const EdgeMaskLevels t) {
    const int l = mask_level_of_block(t.first, t.n, blockIdx.x);
    const unsigned char *__restrict__ keep = t.tab[(size_t)blockIdx.y * DVO_LEVELS + l];
    if (!keep) return;
    unsigned char *__restrict__ e = t.edge[l] + (size_t)blockIdx.y * t.stride[l];
    const size_t n = t.npx[l];
    const unsigned tb = blockIdx.x - t.first[l];
    const size_t base = (size_t)tb * EM_BYTES;
    /* 16-byte words where both planes allow it (the store's npx strides are not all multiples of 16), bytes otherwise */
    const bool vec = ((reinterpret_cast<size_t>(e) | reinterpret_cast<size_t>(keep)) & 15) == 0;
    if (vec) {
        const size_t n16 = n / 16, w = base / 16 + threadIdx.x;
        if (w < n16) {
            uint4 v = reinterpret_cast<uint4 *>(e)[w];
            const uint4 k = reinterpret_cast<const uint4 *>(keep)[w];
            v.x &= k.x; v.y &= k.y; v.z &= k.z; v.w &= k.w;
            reinterpret_cast<uint4 *>(e)[w] = v;
        }
        const size_t i = n16 * 16 + threadIdx.x;                 /* the tail, by the level's last workgroup */
        if (tb + 1 == t.first[l + 1] - t.first[l] && threadIdx.x < 16 && i < n) e[i] &= keep[i];
    } else {
        for (int k = 0; k < 16; k++) {
            const size_t i = base + (size_t)k * EM_BLOCK + threadIdx.x;
            if (i < n) e[i] &= keep[i];
        }
    }
}

size_t mask_levels_bytes(int n, const int *rows, const int *cols, size_t *off) {
    size_t o = 0;
    for (int l = 0; l < n; l++) {
        if (off) off[l] = o;
        o += ((size_t)rows[l] * cols[l] + 15) / 16 * 16;         /* every plane starts on a 16-byte boundary */
    }
    return o;
}

hipError_t launch_mask_levels(const unsigned char *mask, int rows, int cols, int n, int first_shift, int margin, const int *lrows,
                              const int *lcols, unsigned char *const *keep, hipStream_t s) {
    if (n < 1 || n > DVO_LEVELS || margin < 0 || margin > dvo_mask::kMaxMargin) return hipErrorInvalidValue;
    MaskLevels t;
    t.n = n; t.rows = rows; t.cols = cols; t.margin = margin;
    t.first[0] = 0;
    for (int l = 0; l < n; l++) {
        t.shift[l] = first_shift + l; t.lrows[l] = lrows[l]; t.lcols[l] = lcols[l]; t.keep[l] = keep[l];
        t.first[l + 1] = t.first[l] + (unsigned)(((lrows[l] + MT - 1) / MT) * ((lcols[l] + MT - 1) / MT));
    }
    hipLaunchKernelGGL(mask_levels_kernel, dim3(t.first[n]), dim3(MT * MT), 0, s, mask, t);
    return hipGetLastError();
}

hipError_t launch_edge_mask_levels(int n, const int *rows, const int *cols, unsigned char *const *edge, const size_t *edge_stride, int count,
                                   const unsigned char *const *tab, hipStream_t s) {
    if (n < 1 || n > DVO_LEVELS || count < 1) return hipErrorInvalidValue;
    EdgeMaskLevels t;
    t.n = n; t.tab = tab;
    t.first[0] = 0;
    for (int l = 0; l < n; l++) {
        t.edge[l] = edge[l]; t.stride[l] = edge_stride[l]; t.npx[l] = (size_t)rows[l] * cols[l];
        t.first[l + 1] = t.first[l] + (unsigned)((t.npx[l] + EM_BYTES - 1) / EM_BYTES);
    }
    hipLaunchKernelGGL(edge_mask_levels_kernel, dim3(t.first[n], count), dim3(EM_BLOCK), 0, s, t);
    return hipGetLastError();
}

}  // namespace dvo
