/*
 * dvo_depth_register.h -- registration of a raw depth image to the colour camera (include/dvo_amd.h, "depth registration"): the
 * definition, in plain C++.  No device, no context, no other header of the library: dvo_depth_register_host is build() below, the
 * device kernel (dvo_depth_register.hip) shares splat() -- the whole per-pixel function -- with it, and a stand-alone program can
 * include the file as it is.
 *
 * Input: the depth camera's image (depth_rows x depth_cols, row-major, 16-bit millimetres or float metres; a pinhole camera taken as
 * undistorted).  Output: rows x cols 16-bit millimetres in the pixel grid of the colour image AS IT IS UPLOADED (before the stream's
 * cv::undistort, which is why the colour camera's distortion is applied forward, in closed form), 0 = hole.  Every valid depth pixel
 * is unprojected, moved into the colour camera (X_colour = R X_depth + t), and its two corners (u -+ 0.5, v -+ 0.5, at the pixel's own
 * depth) span the footprint it covers in the colour grid; a colour pixel keeps the smallest depth that covered it (z-buffer).
 *
 * All arithmetic is IEEE double in the order written, nothing fused (-ffp-contract=off), no transcendental function: host, device and
 * a numpy restatement agree bit for bit, and min is order-independent, so the device result is byte-equal under any schedule.
 */
#ifndef DVO_DEPTH_REGISTER_H_
#define DVO_DEPTH_REGISTER_H_

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define DVO_DEPTH_HD __host__ __device__ inline
#else
#define DVO_DEPTH_HD inline
#endif

/* the rig as include/dvo_amd.h declares it (the same text under the same guard: whichever header comes first defines it) */
#ifndef DVO_DEPTH_RIG_DEFINED_
#define DVO_DEPTH_RIG_DEFINED_
#define DVO_DEPTH_SPLAT_MAX 8
typedef struct dvo_depth_rig {
    int    depth_rows, depth_cols;   /* geometry of the raw depth image */
    double Kd4[4];                   /* depth camera fx, fy, cx, cy: pinhole, taken as undistorted */
    double R[9];                     /* column-major like every R of this header */
    double t[3];                     /* metres: X_colour = R X_depth + t */
    double Kc4[4];                   /* colour camera fx, fy, cx, cy of the colour image AS IT IS UPLOADED */
    int    has_Dc5;                  /* 1: Dc5 = k1, k2, p1, p2, k3 of the colour camera, applied FORWARD */
    double Dc5[5];
} dvo_depth_rig;
#endif

namespace dvo_depth {

constexpr int kFormatF32 = 0, kFormatU16 = 1;      /* == DVO_DEPTH_F32, DVO_DEPTH_U16 */
constexpr int kSplatMax = DVO_DEPTH_SPLAT_MAX;
constexpr double kCoordLimit = 1073741824.0;       /* 2^30: a corner at or beyond it (or not finite) drops the pixel */

/* finite: neither NaN nor an infinity (x - x is NaN for both) */
DVO_DEPTH_HD bool finite(double x) { return x - x == 0.0; }

/* what every entry point refuses: a size < 1, a focal length that is not positive, a number of the rig that is not finite (Dc5
 * included, whatever has_Dc5 says), has_Dc5 other than 0 or 1.  R is taken as given (not checked for orthogonality) */
inline bool rig_ok(const dvo_depth_rig *g) {
    if (!g || g->depth_rows < 1 || g->depth_cols < 1 || (g->has_Dc5 != 0 && g->has_Dc5 != 1)) return false;
    for (int k = 0; k < 4; k++) if (!finite(g->Kd4[k]) || !finite(g->Kc4[k])) return false;
    for (int k = 0; k < 9; k++) if (!finite(g->R[k])) return false;
    for (int k = 0; k < 3; k++) if (!finite(g->t[k])) return false;
    for (int k = 0; k < 5; k++) if (!finite(g->Dc5[k])) return false;
    return g->Kd4[0] > 0.0 && g->Kd4[1] > 0.0 && g->Kc4[0] > 0.0 && g->Kc4[1] > 0.0;
}

/* metres of a raw value; false: no measurement */
DVO_DEPTH_HD bool metres_u16(unsigned short r, double *Z) {
    if (r == 0) return false;
    *Z = (double)r / 1000.0;
    return true;
}
DVO_DEPTH_HD bool metres_f32(float r, double *Z) {
    const double z = (double)r;
    if (!finite(z) || !(z > 0.0)) return false;
    *Z = z;
    return true;
}

/* the point (a, b) of the depth image at depth Z -> colour pixel coordinates (uc, vc) and colour depth Zc; false: behind the camera */
DVO_DEPTH_HD bool project(const dvo_depth_rig &g, double a, double b, double Z, double *uc, double *vc, double *Zc) {
    const double X = ((a - g.Kd4[2]) * Z) / g.Kd4[0];
    const double Y = ((b - g.Kd4[3]) * Z) / g.Kd4[1];
    const double Xc = g.R[0] * X + g.R[3] * Y + g.R[6] * Z + g.t[0];
    const double Yc = g.R[1] * X + g.R[4] * Y + g.R[7] * Z + g.t[1];
    const double Zc_ = g.R[2] * X + g.R[5] * Y + g.R[8] * Z + g.t[2];
    if (!(Zc_ > 0.0)) return false;
    double x = Xc / Zc_, y = Yc / Zc_;
    if (g.has_Dc5) {
        const double k1 = g.Dc5[0], k2 = g.Dc5[1], p1 = g.Dc5[2], p2 = g.Dc5[3], k3 = g.Dc5[4];
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
        const double xd = x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x));
        const double yd = y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y);
        x = xd; y = yd;
    }
    *uc = g.Kc4[0] * x + g.Kc4[2];
    *vc = g.Kc4[1] * y + g.Kc4[3];
    *Zc = Zc_;
    return true;
}

/* what one depth pixel writes: q millimetres over the colour pixels x0 <= x < x1, y0 <= y < y1 (clipped to the image; may be empty) */
struct Splat { int x0, x1, y0, y1; unsigned q; };

/* ceil(lo) .. min(ceil(hi), ceil(lo) + kSplatMax), clipped to [0, n); |lo|, |hi| < 2^30 */
DVO_DEPTH_HD void cover(double a, double b, int n, int *i0, int *i1) {
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    int s = (int)ceil(lo), e = (int)ceil(hi);
    if (e > s + kSplatMax) e = s + kSplatMax;
    if (s < 0) s = 0;
    if (e > n) e = n;
    *i0 = s; *i1 = e;
}

/* depth pixel (v, u) at Z metres under rig g, into a rows x cols colour image; false: the pixel writes nothing */
DVO_DEPTH_HD bool splat(const dvo_depth_rig &g, int v, int u, double Z, int rows, int cols, Splat *out) {
    double uc, vc, Zc, ua, va, za, ub, vb, zb;
    if (!project(g, (double)u, (double)v, Z, &uc, &vc, &Zc)) return false;
    if (!project(g, (double)u - 0.5, (double)v - 0.5, Z, &ua, &va, &za)) return false;
    if (!project(g, (double)u + 0.5, (double)v + 0.5, Z, &ub, &vb, &zb)) return false;
    if (!finite(ua) || !finite(va) || !finite(ub) || !finite(vb)) return false;
    if (fabs(ua) >= kCoordLimit || fabs(va) >= kCoordLimit || fabs(ub) >= kCoordLimit || fabs(vb) >= kCoordLimit) return false;
    const double q = rint(Zc * 1000.0);                 /* round half to even */
    if (!(q >= 1.0 && q <= 65535.0)) return false;
    out->q = (unsigned)q;
    cover(ua, ub, cols, &out->x0, &out->x1);
    cover(va, vb, rows, &out->y0, &out->y1);
    return true;
}

/* out: rows * cols, row-major, 0 = hole.  False: refused, nothing written */
inline bool build(const dvo_depth_rig *g, const void *depth, int depth_format, int rows, int cols, unsigned short *out) {
    if (!rig_ok(g) || !depth || !out || rows < 1 || cols < 1 || (depth_format != kFormatF32 && depth_format != kFormatU16)) return false;
    const size_t npx = (size_t)rows * cols;
    for (size_t i = 0; i < npx; i++) out[i] = 0;
    for (int v = 0; v < g->depth_rows; v++)
        for (int u = 0; u < g->depth_cols; u++) {
            const size_t i = (size_t)v * g->depth_cols + u;
            double Z;
            if (depth_format == kFormatU16 ? !metres_u16(static_cast<const unsigned short *>(depth)[i], &Z)
                                           : !metres_f32(static_cast<const float *>(depth)[i], &Z))
                continue;
            Splat s;
            if (!splat(*g, v, u, Z, rows, cols, &s)) continue;
            for (int y = s.y0; y < s.y1; y++)
                for (int x = s.x0; x < s.x1; x++) {
                    unsigned short &o = out[(size_t)y * cols + x];
                    if (o == 0 || s.q < o) o = (unsigned short)s.q;       /* q >= 1: 0 is "nothing yet" */
                }
        }
    return true;
}

}  // namespace dvo_depth
#endif
