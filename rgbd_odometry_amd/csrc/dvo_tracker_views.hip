/*
 * dvo_tracker_views.hip -- the debug views of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_views / dvo_tracker_get_view /
 * dvo_tracker_get_residue_histogram; host side dvo_capi_tracker.cpp): what SolveDVO::loop shows after every frame -- the reference points
 * reprojected on the distance transform (sOverlay, SolveDVO.cpp:1186-1226, :2294), the same points coloured by their residual on the now
 * grey image (visualizeDistanceResidueHeatMap, :1528-1583) and the residue histogram (processResidueHistogram, :1398-1410) -- rendered
 * in HBM from the forms the alignment reads, at the pose and level of dvo_tracker_get_information.
 *
 * TWO launches for a whole index list:
 *   1. tracker_views_background_kernel: pixel tiles x listed streams.  A tile is VIEW_TY = 6 rows (the interior rows of one line of the
 *      compact now form, dvo_palette.h) by VIEW_TX = 64 columns: lanes walk the columns of the tile downwards -- the direction in which
 *      the compact form, the 16-byte texels and the frame store's grey image are all contiguous --, put the two grey values of a pixel
 *      into LDS, and the tile's rows then leave as whole dwords of the row-major BGR8 images (byte stores only for the at most three
 *      bytes at either end of a row segment that share a dword with a neighbouring tile).  Tile 0 of a stream also zeroes its record.
 *   2. tracker_views_points_kernel: point chunks x listed streams, one point per lane and trip.  project_point of dvo_device_math.h on
 *      the compact list (the floats of the alignment), the look-up of d = DT(py, px), two 3-byte marks, and hist[(int)eps + 1] in a
 *      260-entry LDS histogram (integer LDS atomics) whose non-zero bins go to the record with integer atomicAdd: integer sums have no
 *      order, the record does not depend on the grid.  A mark's colour depends on its pixel alone, so points that share a pixel store
 *      the same bytes and need no order either.
 * Both take the `switched` filter of tracker_information_kernel; entries at or beyond n_aligned are streams on their first frame: plain
 * backgrounds, the zero record with level -1.
 *
 * One deviation from the reference: cordList_2_mask (:472) accepts u == cols and v == rows and then writes outside its mask; here a
 * point marks a pixel exactly when the engine counts it visible (the half-open rule of project_point).  A bin index is clamped to the
 * 260 counters (the engine's distance transforms are normalised to [0, 255], so nothing is clamped in practice).
 *
 * Plain on purpose: no teams, no exchange between workgroups, no waiting.  The alignment kernels' sources stay as they are: the offset
 * arithmetic of the compact form (p4_line_offset of dvo_palette.h, in plain form) is restated below, as dvo_tracker_info.hip does.
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_kernel_common.h"
#include "dvo_palette.h"

#include <algorithm>

namespace dvo {

namespace {

constexpr int VIEW_TX = 64, VIEW_TY = DVO_P4_ROWS;      /* pixels of a background tile */
constexpr int VIEW_BG_BLOCK = 128;
constexpr int VIEW_PT_BLOCK = 256;
constexpr int VIEW_PT_TRIPS = 2;                        /* points per lane before the LDS histogram is flushed (more workgroups than that need: a grid stride) */
constexpr int VIEW_PT_GRID_MAX = 256;
constexpr int VIEW_ROW_DWORDS = (VIEW_TX * 3 + 3) / 4 + 1;      /* dwords that cover 192 bytes at any alignment */

/* the plain form of p4_line_offset (dvo_palette.h) + 128, as dvo_fused.hip once had it: byte offset of the rank word ABOVE pixel (yy, xx) in the compact image; the pixel's own
 * word is the next one.  yy / 6 by multiplication (exact for yy < 98 000) */
DVO_DEV unsigned view_p4_byte_offset(int yy, int xx, unsigned p4_col_bytes /* p4_tiles_per_col * 128 */) {
    static_assert(DVO_P4_ROWS == 6, "written for 6 interior rows per line");
    const unsigned ty = __umul24((unsigned)yy, 43691u) >> 18;
    return __umul24((unsigned)(xx >> 2), p4_col_bytes) + 128u /* the sentinel line */ + (((unsigned)xx & 3u) << 5) + ((unsigned)yy << 2) + __umul24(ty, 104u);
}

/* where a stream's now level is read from: its compact form where that is complete, otherwise its 16-byte texels (the branch of
 * tracker_information_kernel) */
struct ViewNow {
    const char *p4;             /* NULL: texels */
    const float2 *pal;
    const float4 *tex;
    unsigned col_bytes;
    int tiles_per_col;
};
DVO_DEV ViewNow view_now(const LevelSlab &L, int p, int use_p4) {
    ViewNow n;
    const int pal_n_raw = (use_p4 && L.pal_n) ? __builtin_amdgcn_readfirstlane(L.pal_n[p]) : 0;
    const bool p4 = pal_count(pal_n_raw) > 0 && !pal_partial(pal_n_raw);
    n.p4 = p4 ? reinterpret_cast<const char *>(L.p4 + (size_t)p * L.p4_stride) : nullptr;
    n.pal = p4 ? L.pal + (size_t)p * DVO_PAL_MAX : nullptr;
    n.tex = p4 ? nullptr : L.tex + (size_t)p * L.tex_stride;
    n.col_bytes = (unsigned)p4_tiles_per_col(L.rows) * 128u;
    n.tiles_per_col = texel_tiles_per_col(L.rows);
    return n;
}
/* DT(yy, xx): the float the alignment looks up */
DVO_DEV float view_dt(const ViewNow &n, int yy, int xx) {
    if (n.p4) {
        const unsigned w = *reinterpret_cast<const unsigned *>(n.p4 + view_p4_byte_offset(yy, xx, n.col_bytes) + 4u);
        return n.pal[(w >> 3) & 0x1fffu].x;
    }
    return n.tex[texel_index(yy, xx, n.tiles_per_col)].x;
}

DVO_DEV unsigned view_u8(float d) {                     /* convertTo(CV_8UC1): round half to even, saturate (NaN -> 0) */
    return (unsigned)fminf(fmaxf(rintf(d), 0.0f), 255.0f);
}

/* entry i of the list belongs to this launch */
DVO_DEV bool view_listed(const TrackerOut *__restrict__ out, int i, int n_aligned, int switched) {
    return i < n_aligned ? ((out[i].event >= 2) == (switched != 0)) : (switched == 0);
}

/* the jet map of FColorMap, entry j of 64, from its closed form */
DVO_DEV int jet_ramp(int j) { return j <= 0 ? 0 : min(255, 16 * j - 1); }
DVO_DEV void jet_bgr(int i, unsigned &b, unsigned &g, unsigned &r) {
    b = (unsigned)min(jet_ramp(i + 9), jet_ramp(39 - i));
    g = (unsigned)min(jet_ramp(i - 7), jet_ramp(55 - i));
    r = (unsigned)min(jet_ramp(i - 23), jet_ramp(71 - i));
}

}  // namespace

__global__ void __launch_bounds__(VIEW_BG_BLOCK)
tracker_views_background_kernel(const TrackerEntry *__restrict__ list, const TrackerOut *__restrict__ out, const int *__restrict__ slots,
                                int n_aligned, int switched, LevelSlab L, int level, int use_p4, const unsigned char *__restrict__ grey,
                                size_t grey_npx, int tiles_x, unsigned char *__restrict__ views, size_t view_stride, size_t view_plane,
                                TrackerViewRecord *__restrict__ rec) {
    __shared__ unsigned char g_dt[VIEW_TY][VIEW_TX], g_grey[VIEW_TY][VIEW_TX];
    const int i = blockIdx.y;
    if (!view_listed(out, i, n_aligned, switched)) return;
    const int p = list[i].stream;
    const int rows = L.rows, cols = L.cols;
    if (blockIdx.x == 0) {                              /* the stream's record: counters to zero, what the point kernel adds to */
        TrackerViewRecord &o = rec[i];
        for (int k = threadIdx.x; k < DVO_VIEW_HIST_BINS; k += VIEW_BG_BLOCK) o.hist[k] = 0u;
        if (threadIdx.x == 0) {
            o.n_points = i < n_aligned ? L.N[p] : 0;
            o.level = i < n_aligned ? level : -1;
        }
    }
    const int y0 = ((int)blockIdx.x / tiles_x) * VIEW_TY, x0 = ((int)blockIdx.x % tiles_x) * VIEW_TX;
    const int th = min(VIEW_TY, rows - y0), tw = min(VIEW_TX, cols - x0);
    const ViewNow now = view_now(L, p, use_p4);
    const unsigned char *__restrict__ gsrc = grey + (size_t)slots[i] * grey_npx;          /* column-major */
    for (int k = threadIdx.x; k < VIEW_TX * VIEW_TY; k += VIEW_BG_BLOCK) {
        const int ly = k % VIEW_TY, lx = k / VIEW_TY;
        if (ly < th && lx < tw) {
            const int yy = y0 + ly, xx = x0 + lx;
            g_dt[ly][lx] = (unsigned char)view_u8(view_dt(now, yy, xx));
            g_grey[ly][lx] = gsrc[(size_t)xx * rows + yy];
        }
    }
    __syncthreads();
    unsigned char *__restrict__ v0 = views + (size_t)p * view_stride, *__restrict__ v1 = v0 + view_plane;
    const int len = 3 * tw;
    for (int k = threadIdx.x; k < VIEW_TY * VIEW_ROW_DWORDS; k += VIEW_BG_BLOCK) {
        const int ly = k / VIEW_ROW_DWORDS, j = k % VIEW_ROW_DWORDS;
        if (ly >= th) break;
        const size_t a = ((size_t)(y0 + ly) * cols + x0) * 3;          /* first byte of the row segment; the images start on 256-byte boundaries */
        const size_t A = (a & ~(size_t)3) + 4u * (size_t)j;
        const int off = (int)((long long)A - (long long)a);            /* of the dword's first byte inside the segment: -3 .. len + 2 */
        if (off >= len) continue;
        unsigned w0 = 0u, w1 = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int o = min(max(off + b, 0), len - 1) / 3;
            w0 |= (unsigned)g_dt[ly][o] << (8 * b);
            w1 |= (unsigned)g_grey[ly][o] << (8 * b);
        }
        if (off >= 0 && off + 4 <= len) {
            *reinterpret_cast<unsigned *>(v0 + A) = w0;
            *reinterpret_cast<unsigned *>(v1 + A) = w1;
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (off + b >= 0 && off + b < len) {
                    v0[A + b] = (unsigned char)(w0 >> (8 * b));
                    v1[A + b] = (unsigned char)(w1 >> (8 * b));
                }
        }
    }
}

__global__ void __launch_bounds__(VIEW_PT_BLOCK)
tracker_views_points_kernel(const TrackerEntry *__restrict__ list, const TrackerOut *__restrict__ out, int n_aligned, int switched,
                            const double *__restrict__ poses, LevelSlab L, int level, Intrinsics K, int use_p4,
                            unsigned char *__restrict__ views, size_t view_stride, size_t view_plane, TrackerViewRecord *__restrict__ rec) {
    __shared__ unsigned hist[DVO_VIEW_HIST_BINS];
    const int i = blockIdx.y;
    if (i >= n_aligned || !view_listed(out, i, n_aligned, switched)) return;
    const int p = list[i].stream;
    const int N = __builtin_amdgcn_readfirstlane(L.N[p]);
    const int chunk = VIEW_PT_BLOCK * VIEW_PT_TRIPS;
    if ((int)blockIdx.x * chunk >= N) return;
    const uint2 *__restrict__ pts = L.cpts + (size_t)p * L.pt_cap;

    IterConst c;
    level_consts(c, pair_intrinsics(K, p), level, L.rows, L.cols);
    const double *P = poses + (size_t)p * 12;
    c.r[0] = uniform_f((float)P[0]); c.r[1] = uniform_f((float)P[1]); c.r[2] = uniform_f((float)P[2]);      /* cR.cast<float>() :673 */
    c.r[3] = uniform_f((float)P[3]); c.r[4] = uniform_f((float)P[4]); c.r[5] = uniform_f((float)P[5]);
    c.r[6] = uniform_f((float)P[6]); c.r[7] = uniform_f((float)P[7]); c.r[8] = uniform_f((float)P[8]);
    c.t[0] = uniform_f((float)P[9]); c.t[1] = uniform_f((float)P[10]); c.t[2] = uniform_f((float)P[11]);    /* :674 */
    const ViewNow now = view_now(L, p, use_p4);
    unsigned char *__restrict__ v0 = views + (size_t)p * view_stride, *__restrict__ v1 = v0 + view_plane;

    for (int k = threadIdx.x; k < DVO_VIEW_HIST_BINS; k += VIEW_PT_BLOCK) hist[k] = 0u;
    __syncthreads();
    for (int base = (int)blockIdx.x * chunk; base < N; base += (int)gridDim.x * chunk) {
#pragma unroll
        for (int u = 0; u < VIEW_PT_TRIPS; u++) {
            const int k = base + u * VIEW_PT_BLOCK + (int)threadIdx.x;
            const bool valid = k < N;
            const uint2 v = pts[valid ? k : (N - 1)];
            float X, Y, Z, xn, yn, zn, uu, vv;
            expand_compact(c, v.x, __uint_as_float(v.y), X, Y, Z);
            const bool vis = project_point(c, X, Y, Z, xn, yn, zn, uu, vv) && valid;
            float eps = 0.0f;                           /* getReprojectedEpsilons leaves an invisible point's residual at 0 (:429-441) */
            if (vis) {
                const int px = (int)uu, py = (int)vv;   /* :376-377 == floor for u, v >= 0; inside the level by the visibility rule */
                eps = view_dt(now, py, px);
                const size_t o = ((size_t)py * L.cols + px) * 3;
                v0[o] = 0; v0[o + 1] = 255; v0[o + 2] = 0;
                unsigned b, g, r;
                jet_bgr(eps > 60.0f ? 63 : min(max((int)eps, 0), 63), b, g, r);
                v1[o] = (unsigned char)b; v1[o + 1] = (unsigned char)g; v1[o + 2] = (unsigned char)r;
            }
            if (valid) atomicAdd(&hist[min(max((int)eps + 1, 0), DVO_VIEW_HIST_BINS - 1)], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < DVO_VIEW_HIST_BINS; k += VIEW_PT_BLOCK)
        if (hist[k]) atomicAdd(&rec[i].hist[k], hist[k]);
}

hipError_t launch_tracker_views(const TrackerEntry *list, const TrackerOut *out, const int *slots, int n_aligned, int count, int switched,
                                const double *poses, const LevelSlab &L, int level, const Intrinsics &K, bool use_p4,
                                const unsigned char *grey, size_t grey_npx, unsigned char *views, size_t view_stride, size_t view_plane,
                                TrackerViewRecord *rec, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int tiles_x = (L.cols + VIEW_TX - 1) / VIEW_TX, tiles_y = (L.rows + VIEW_TY - 1) / VIEW_TY;
    hipLaunchKernelGGL(tracker_views_background_kernel, dim3(tiles_x * tiles_y, count), dim3(VIEW_BG_BLOCK), 0, s, list, out, slots,
                       n_aligned, switched, L, level, use_p4 ? 1 : 0, grey, grey_npx, tiles_x, views, view_stride, view_plane, rec);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int chunk = VIEW_PT_BLOCK * VIEW_PT_TRIPS;
    const int gx = std::min(std::max((L.pt_cap + chunk - 1) / chunk, 1), VIEW_PT_GRID_MAX);
    hipLaunchKernelGGL(tracker_views_points_kernel, dim3(gx, count), dim3(VIEW_PT_BLOCK), 0, s, list, out, n_aligned, switched, poses, L,
                       level, K, use_p4 ? 1 : 0, views, view_stride, view_plane, rec);
    return hipGetLastError();
}

}  // namespace dvo
