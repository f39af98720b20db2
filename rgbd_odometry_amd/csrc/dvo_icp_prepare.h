/*
 * dvo_icp_prepare.h -- the front end of the frame-to-model alignment (include/dvo_amd.h, "preparing a depth frame"): a bilateral filter
 * of the depth image and the normals of the now frame, the definition in plain C++.  It follows the rules of dvo_icp.h, which it
 * includes: no device, no context, IEEE double in the order written, nothing fused (-ffp-contract=off), no transcendental function in
 * anything the device also runs; division and sqrt in double only.  dvo_icp_prepare_host is prepare() below; the kernels
 * (dvo_icp_prepare.hip) call filter_taps() and normal_pixel() as they are.  The gate that uses the normals is part of term() in dvo_icp.h.
 *
 * The weights are DATA: two tables in dvo_icp_prepare_params.  Host and device agree in bytes given the tables, and the definition never
 * depends on anyone's exp().  params_gaussian() fills them from two sigmas on the host (it alone calls exp).
 *
 * Filter.  The input is rows x cols, DVO_DEPTH_U16 or DVO_DEPTH_F32 under the hole rules of dvo_tsdf::metres_u16 / metres_f32; the
 * output is float metres, 0.0f = a hole.  Per output pixel (u, v):
 *   Dc = metres of the centre; a hole stays a hole;  num = 0.0, den = 0u (32 unsigned bits: 169 * 255 * 65535 < 2^32);
 *   the taps: dy from -radius to radius and, inside that, dx from -radius to radius, the centre an ordinary tap;
 *   a tap outside the image or on a hole is skipped;  D = its metres;  k = fabs(D - Dc) * range_scale;  skipped unless k < 256.0;
 *   w = (unsigned)spatial[(dy + radius) * (2 radius + 1) + (dx + radius)] * (unsigned)range[(int)k];
 *   num = num + (double)w * D;  den = den + w;
 *   the output is (float)(num / (double)den).
 * Normals, from the filtered float image F, in the axes of the NOW CAMERA (the gate rotates them by the estimate); three floats per
 * pixel, (0, 0, 0) = none.  None unless 1 <= u <= cols - 2 and 1 <= v <= rows - 2, F is no hole at the pixel and at its four
 * neighbours, and every neighbour has fabs(D_nb - D_c) <= edge_max (in double).  Otherwise
 *   V(u, v) = (((double)u - cx) / fx * D, ((double)v - cy) / fy * D, D): the alignment's own back-projection;
 *   a = V(u + 1, v) - V(u - 1, v);  b = V(u, v + 1) - V(u, v - 1);  G = b x a = (b1 a2 - b2 a1, b2 a0 - b0 a2, b0 a1 - b1 a0);
 *   gg = (G0 G0 + G1 G1) + G2 G2; none unless gg > 0;  n_k = (float)(G_k / sqrt(gg)).
 * On a fronto-parallel plane G points along -z: to the viewer's side, as the ray caster's normals do.
 */
#ifndef DVO_ICP_PREPARE_H_
#define DVO_ICP_PREPARE_H_

#include "dvo_icp.h"

/* the public struct as include/dvo_amd.h declares it (the same text under the same guard) */
#ifndef DVO_ICP_PREPARE_TYPES_DEFINED_
#define DVO_ICP_PREPARE_TYPES_DEFINED_
#define DVO_ICP_PREPARE_MAX_RADIUS 6
#define DVO_ICP_PREPARE_RANGE_BINS 256
typedef struct dvo_icp_prepare_params {
    int            radius;              /* [0, 6]: the window is (2 radius + 1)^2 */
    int            reserved;            /* 0 */
    double         range_scale;         /* bins per metre of depth difference: finite, > 0 */
    double         edge_max;            /* metres, finite, > 0: no normal across a larger depth step */
    unsigned short range[256];          /* range weight of bin k; range[0] >= 1 */
    unsigned char  spatial[13 * 13];    /* weight of tap (dy, dx) at (dy + radius) * (2 radius + 1) + (dx + radius);
                                           the centre's >= 1; entries past (2 radius + 1)^2 play no part */
} dvo_icp_prepare_params;
#endif

namespace dvo_icp {

constexpr int kPrepareMaxRadius = DVO_ICP_PREPARE_MAX_RADIUS;
constexpr int kRangeBins = DVO_ICP_PREPARE_RANGE_BINS;

inline bool prepare_params_ok(const dvo_icp_prepare_params *fp) {
    if (!fp || fp->radius < 0 || fp->radius > kPrepareMaxRadius || fp->reserved != 0) return false;
    if (!finite(fp->range_scale) || !finite(fp->edge_max) || !(fp->range_scale > 0.0) || !(fp->edge_max > 0.0)) return false;
    const int side = 2 * fp->radius + 1;
    return fp->range[0] >= 1 && fp->spatial[fp->radius * side + fp->radius] >= 1;
}

/* ---- the per-pixel functions, shared with the device ---- */

/* the taps of one output pixel whose centre is no hole.  tap(dy, dx, &D): the metres of the tap; false: outside the image or a hole
 * (a tap source may instead hand back +infinity for either: k is then no bin, and the tap is skipped all the same).  spatial: the
 * table as bytes or widened to words (the device reads it with scalar loads, which have no byte form); a tap's weight is read before
 * anything can skip the tap, where every lane of a wave still runs */
template <class Tap, class Weight>
DVO_TSDF_HD float filter_taps(int radius, double range_scale, const Weight *spatial, const unsigned short *range, double Dc, Tap tap) {
    double num = 0.0;
    unsigned den = 0u;
    const int side = 2 * radius + 1;
    for (int dy = -radius; dy <= radius; dy++)
        for (int dx = -radius; dx <= radius; dx++) {
            const unsigned ws = (unsigned)spatial[(dy + radius) * side + (dx + radius)];
            double D;
            if (!tap(dy, dx, &D)) continue;
            const double k = fabs(D - Dc) * range_scale;
            if (!(k < 256.0)) continue;
            const unsigned w = ws * (unsigned)range[(int)k];
            num = num + (double)w * D;
            den = den + w;
        }
    return (float)(num / (double)den);
}

/* the taps of the image itself */
struct ImageTap {
    const void *image;
    int format, rows, cols, u, v;
    DVO_TSDF_HD bool operator()(int dy, int dx, double *D) const {
        const int y = v + dy, x = u + dx;
        if (y < 0 || y >= rows || x < 0 || x >= cols) return false;
        return metres(image, format, (size_t)y * (size_t)cols + (size_t)x, D);
    }
};

DVO_TSDF_HD float filter_pixel(const dvo_icp_prepare_params &fp, const void *image, int format, int rows, int cols, int u, int v) {
    double Dc;
    if (!metres(image, format, (size_t)v * (size_t)cols + (size_t)u, &Dc)) return 0.0f;
    const ImageTap tap = {image, format, rows, cols, u, v};
    return filter_taps(fp.radius, fp.range_scale, fp.spatial, fp.range, Dc, tap);
}

/* the normal of pixel (u, v) of the filtered image F into n[3]; false: none, n = (0, 0, 0) */
DVO_TSDF_HD bool normal_pixel(const float *F, int rows, int cols, const double *K, double edge_max, int u, int v, float *n) {
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    if (u < 1 || u > cols - 2 || v < 1 || v > rows - 2) return false;
    const size_t px = (size_t)v * (size_t)cols + (size_t)u;
    double Dc, Dl, Dr, Du, Dd;
    if (!dvo_tsdf::metres_f32(F[px], &Dc) || !dvo_tsdf::metres_f32(F[px - 1], &Dl) || !dvo_tsdf::metres_f32(F[px + 1], &Dr) ||
        !dvo_tsdf::metres_f32(F[px - (size_t)cols], &Du) || !dvo_tsdf::metres_f32(F[px + (size_t)cols], &Dd))
        return false;
    if (!(fabs(Dl - Dc) <= edge_max && fabs(Dr - Dc) <= edge_max && fabs(Du - Dc) <= edge_max && fabs(Dd - Dc) <= edge_max)) return false;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const double Vr[3] = {((double)(u + 1) - cx) / fx * Dr, ((double)v - cy) / fy * Dr, Dr};
    const double Vl[3] = {((double)(u - 1) - cx) / fx * Dl, ((double)v - cy) / fy * Dl, Dl};
    const double Vd[3] = {((double)u - cx) / fx * Dd, ((double)(v + 1) - cy) / fy * Dd, Dd};
    const double Vu[3] = {((double)u - cx) / fx * Du, ((double)(v - 1) - cy) / fy * Du, Du};
    const double a[3] = {Vr[0] - Vl[0], Vr[1] - Vl[1], Vr[2] - Vl[2]};
    const double b[3] = {Vd[0] - Vu[0], Vd[1] - Vu[1], Vd[2] - Vu[2]};
    const double G[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};
    const double gg = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2];
    if (!(gg > 0.0)) return false;
    const double len = sqrt(gg);
    n[0] = (float)(G[0] / len); n[1] = (float)(G[1] / len); n[2] = (float)(G[2] / len);
    return true;
}

/* ---- the host ---- */

/* The tables of a Gaussian pair, host only (the one place that calls exp): spatial = rint(255 exp(-(dx^2 + dy^2) / (2 sigma_s^2))),
 * range_scale = 256 / (3 sigma_r) -- the table ends at three sigmas --, range[k] = rint(65535 exp(-((k + 0.5) / range_scale)^2 /
 * (2 sigma_r^2))): the weight at the middle of bin k.  False: refused, nothing written */
inline bool prepare_params_gaussian(int radius, double sigma_s_px, double sigma_r_m, double edge_max, dvo_icp_prepare_params *fp) {
    if (!fp || radius < 0 || radius > kPrepareMaxRadius || !finite(sigma_s_px) || !finite(sigma_r_m) || !finite(edge_max) || !(sigma_s_px > 0.0) ||
        !(sigma_r_m > 0.0) || !(edge_max > 0.0))
        return false;
    const double scale = 256.0 / (3.0 * sigma_r_m);
    if (!finite(scale) || !(scale > 0.0)) return false;
    fp->radius = radius; fp->reserved = 0; fp->range_scale = scale; fp->edge_max = edge_max;
    for (int k = 0; k < kRangeBins; k++) {
        const double d = ((double)k + 0.5) / scale;
        fp->range[k] = (unsigned short)rint(65535.0 * exp(-(d * d) / (2.0 * sigma_r_m * sigma_r_m)));
    }
    for (int k = 0; k < 13 * 13; k++) fp->spatial[k] = 0;
    const int side = 2 * radius + 1;
    for (int dy = -radius; dy <= radius; dy++)
        for (int dx = -radius; dx <= radius; dx++)
            fp->spatial[(dy + radius) * side + (dx + radius)] =
                (unsigned char)rint(255.0 * exp(-((double)(dx * dx + dy * dy)) / (2.0 * sigma_s_px * sigma_s_px)));
    return true;
}
/* radius 3, sigma_s 2 pixels, sigma_r 0.03 m, edge_max 0.05 m: a design choice for a metre-range sensor with millimetre noise */
inline void prepare_params_default(dvo_icp_prepare_params *fp) { (void)prepare_params_gaussian(3, 2.0, 0.03, 0.05, fp); }

/* what every public call refuses in its lists; K4: 4 doubles per image */
inline bool prepare_lists_ok(int count, const double *K4, const void *const *depth, float *const *depth_out, float *const *normals_out) {
    if (count < 1 || !K4 || !depth || !depth_out) return false;
    const double identity[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < count; i++)
        if (!depth[i] || !depth_out[i] || (normals_out && !normals_out[i]) || !frame_ok(K4 + 4 * (size_t)i, identity)) return false;
    return true;
}

/* images 0 .. count - 1, independently: depth_out[i] rows x cols floats, normals_out[i] (the list may be NULL) 3 rows x cols floats.
 * False: refused, nothing written */
inline bool prepare(const dvo_icp_prepare_params *fp, int count, int depth_format, int rows, int cols, const double *K4, const void *const *depth,
                    float *const *depth_out, float *const *normals_out) {
    if (!prepare_params_ok(fp) || !format_ok(depth_format) || !shape_ok(rows, cols) || !prepare_lists_ok(count, K4, depth, depth_out, normals_out))
        return false;
    for (int i = 0; i < count; i++) {
        for (int v = 0; v < rows; v++)
            for (int u = 0; u < cols; u++) depth_out[i][(size_t)v * (size_t)cols + (size_t)u] = filter_pixel(*fp, depth[i], depth_format, rows, cols, u, v);
        if (!normals_out) continue;
        for (int v = 0; v < rows; v++)
            for (int u = 0; u < cols; u++)
                (void)normal_pixel(depth_out[i], rows, cols, K4 + 4 * (size_t)i, fp->edge_max, u, v, normals_out[i] + 3 * ((size_t)v * (size_t)cols + (size_t)u));
    }
    return true;
}

}  // namespace dvo_icp
#endif
