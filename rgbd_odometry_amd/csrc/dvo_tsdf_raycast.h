/*
 * dvo_tsdf_raycast.h -- ray casting of a fused volume into depth and normal maps (include/dvo_amd.h, "from the map back to depth"):
 * the definition, in plain C++.  It follows the rules of dvo_tsdf_map.h, which it includes: no device, no context, IEEE double in the
 * order written, nothing fused (-ffp-contract=off), no transcendental function.  sqrt and division in double are used; both are
 * correctly rounded on the host and on the device (dvo_device_math.h relies on the same sqrt).  Every position comes from a direct
 * formula of an integer index -- a sample's depth from its index k, never from adding steps up.  dvo_raycast_host is raycast() below;
 * the kernel (dvo_tsdf_raycast.hip) calls pixel(), the whole per-ray function, as it is.
 *
 * A view is a volume, K4 = fx, fy, cx, cy and a pose {R column-major, t}, camera to world; rows x cols are shared by a call.
 * Ray of pixel (u, v): xn = ((double)u - cx) / fx, yn = ((double)v - cy) / fy; the point at camera depth Z is Pc = (xn Z, yn Z, Z),
 *   in the world Pw = R Pc + t (per row ((R0 x + R3 y) + R6 z) + t0), in voxels g = (Pw - origin) inv_vs with inv_vs = 1.0 / voxel_size.
 * Sample S(g): i = floor(g), f = g - i per axis; valid iff on every axis 0 <= i and i + 1 <= n - 1 (compared in double: a NaN fails)
 *   and all eight corner words have w >= min_weight; its value is the trilinear interpolation of the eight q as doubles, along x, then
 *   y, then z, each step a + f (b - a).  A volume with a dimension of 1 has no valid sample.
 * March: step = step_trunc * trunc; sample k sits at Z_k = z_near + step (double)k, k = 0, 1, ... while Z_k <= z_far.  The ray ends at
 *   the first valid sample with S <= 0: a hit iff sample k - 1 exists and was valid with S_prev > 0, else a hole (the ray started inside
 *   or behind a surface).  Hit: Z* = Z_{k-1} + step (S_prev / (S_prev - S_cur)).  A ray that passes z_far without ending is a hole.
 * Depth: DVO_DEPTH_F32 (float)Z*, a hole 0.0f; DVO_DEPTH_U16 m = rint(Z* 1000.0), a hole 0, and m outside [1, 65535] is a hole.
 * Normal (optional, three floats per pixel, world axes): g* = the voxel coordinates of the point at Z*; G = (S(g* + ex) - S(g* - ex),
 *   S(g* + ey) - S(g* - ey), S(g* + ez) - S(g* - ez)); the normal is (float)(G_k / sqrt(G.G)) with G.G = (Gx Gx + Gy Gy) + Gz Gz; it is
 *   (0, 0, 0) for a hole, when one of the six samples is invalid, or when G.G is not > 0.  q is positive in front of a surface, so the
 *   normal points to the viewer's side.
 *
 * step_trunc.  With step_trunc <= 0.5 both samples that bracket the surface lie inside the unsaturated band |sdf| < trunc for ordinary
 * fields of view (a ray at angle a to the surface normal moves step cos a towards it per sample), where the field is linear and the
 * interpolation of Z* exact up to quantisation.  At 1.0 the bracket reaches clamped values (q = +-32767) and Z* is biased: on a fused
 * plane, a numpy prototype of this definition measured a worst error of 6e-7 m at 0.5 and 1.9e-4 m at 1.0.
 *
 * What an implementation may skip (the kernel does both): a sample whose first corner word fails min_weight is invalid whatever the
 * other seven say -- sample() below reads it first --, and samples outside the volume's box are invalid, so a march clipped to a range of k that
 * contains every sample inside the box (clip() below: conservative, widened by a voxel, a rounding allowance and two samples) gives
 * the same result: an invalid sample before the range leaves "no valid previous sample", as starting there does.
 */
#ifndef DVO_TSDF_RAYCAST_H_
#define DVO_TSDF_RAYCAST_H_

#include "dvo_tsdf_map.h"

/* the public struct as include/dvo_amd.h declares it (the same text under the same guard) */
#ifndef DVO_RAYCAST_TYPES_DEFINED_
#define DVO_RAYCAST_TYPES_DEFINED_
#define DVO_RAYCAST_MAX_STEPS 65536      /* samples of one view's march */
typedef struct dvo_raycast_params {
    double z_near, z_far;                /* metres: the first sample's camera depth, and the depth no sample lies beyond */
    double step_trunc;                   /* the march's step in units of the volume's trunc: (0, 1] */
    int    min_weight;                   /* a sample needs this many observations in all eight corners: [1, 65535] */
} dvo_raycast_params;
#endif

namespace dvo_tsdf {

constexpr int kRaycastMaxSteps = DVO_RAYCAST_MAX_STEPS;

inline void raycast_params_default(dvo_raycast_params *p) { p->z_near = 0.1; p->z_far = 8.0; p->step_trunc = 0.5; p->min_weight = 1; }

inline bool raycast_params_ok(const dvo_raycast_params *p) {
    return p && finite(p->z_near) && finite(p->z_far) && finite(p->step_trunc) && p->z_near > 0.0 && p->z_near < p->z_far &&
           p->step_trunc > 0.0 && p->step_trunc <= 1.0 && p->min_weight >= 1 && p->min_weight <= 65535;
}

/* the depth of sample k: the direct formula */
DVO_TSDF_HD double sample_depth(double z_near, double step, int k) { return z_near + step * (double)k; }

/* how many samples the march of a volume has: the k with Z_k <= z_far (Z_k does not decrease with k); -1: more than
 * DVO_RAYCAST_MAX_STEPS, or a step that is not positive */
inline int march_samples(const dvo_raycast_params &p, double trunc) {
    const double step = p.step_trunc * trunc;
    if (!(step > 0.0)) return -1;
    const double est = (p.z_far - p.z_near) / step;
    if (!(est < (double)kRaycastMaxSteps + 2.0)) return -1;
    int n = (int)floor(est);
    while (n > 0 && !(sample_depth(p.z_near, step, n - 1) <= p.z_far)) n--;
    while (n <= kRaycastMaxSteps && sample_depth(p.z_near, step, n) <= p.z_far) n++;
    return n <= kRaycastMaxSteps ? n : -1;
}

/* ---- the per-ray functions, shared with the device ---- */

/* what a volume contributes to every sample; inv_vs = 1.0 / voxel_size, computed once per volume */
struct RayVolume {
    int nx, ny, nz, pad_;
    double origin[3], inv_vs;
};
DVO_TSDF_HD RayVolume ray_volume(const dvo_tsdf_volume &v) {
    RayVolume r;
    r.nx = v.nx; r.ny = v.ny; r.nz = v.nz; r.pad_ = 0;
    r.origin[0] = v.origin[0]; r.origin[1] = v.origin[1]; r.origin[2] = v.origin[2];
    r.inv_vs = 1.0 / v.voxel_size;
    return r;
}
/* one view: pose {R column-major, t} camera to world, K = fx, fy, cx, cy, step = step_trunc * trunc of its volume */
struct RayCamera {
    double R[9], t[3], K[4], step;
};
struct RayConst { int depth_format, rows, cols, min_weight; double z_near, z_far; };

/* the voxel coordinates of the point at camera depth Z on the ray (xn, yn) */
DVO_TSDF_HD void ray_point(const RayVolume &rv, const RayCamera &c, double xn, double yn, double Z, double *g) {
    const double X = xn * Z, Y = yn * Z;
    g[0] = ((((c.R[0] * X + c.R[3] * Y) + c.R[6] * Z) + c.t[0]) - rv.origin[0]) * rv.inv_vs;
    g[1] = ((((c.R[1] * X + c.R[4] * Y) + c.R[7] * Z) + c.t[1]) - rv.origin[1]) * rv.inv_vs;
    g[2] = ((((c.R[2] * X + c.R[5] * Y) + c.R[8] * Z) + c.t[2]) - rv.origin[2]) * rv.inv_vs;
}

/* S(g); false: not valid.  The first corner's weight is looked at before the other seven are read */
DVO_TSDF_HD bool sample(const unsigned *words, const RayVolume &rv, int min_weight, double gx, double gy, double gz, double *S) {
    const double ix = floor(gx), iy = floor(gy), iz = floor(gz);
    if (!(ix >= 0.0 && ix + 1.0 <= (double)(rv.nx - 1) && iy >= 0.0 && iy + 1.0 <= (double)(rv.ny - 1) && iz >= 0.0 &&
          iz + 1.0 <= (double)(rv.nz - 1)))
        return false;                                                                                  /* NaN falls out here */
    const double fx = gx - ix, fy = gy - iy, fz = gz - iz;
    const size_t sy = (size_t)rv.nx, sz = (size_t)rv.nx * (size_t)rv.ny;
    const unsigned *w = words + ((size_t)(int)ix + sy * ((size_t)(int)iy + (size_t)rv.ny * (size_t)(int)iz));
    const unsigned w000 = w[0];
    if (word_w(w000) < min_weight) return false;
    const unsigned w100 = w[1], w010 = w[sy], w110 = w[sy + 1], w001 = w[sz], w101 = w[sz + 1], w011 = w[sz + sy], w111 = w[sz + sy + 1];
    if (word_w(w100) < min_weight || word_w(w010) < min_weight || word_w(w110) < min_weight || word_w(w001) < min_weight ||
        word_w(w101) < min_weight || word_w(w011) < min_weight || word_w(w111) < min_weight)
        return false;
    const double q000 = (double)word_q(w000), q100 = (double)word_q(w100), q010 = (double)word_q(w010), q110 = (double)word_q(w110),
                 q001 = (double)word_q(w001), q101 = (double)word_q(w101), q011 = (double)word_q(w011), q111 = (double)word_q(w111);
    const double c00 = q000 + fx * (q100 - q000), c10 = q010 + fx * (q110 - q010), c01 = q001 + fx * (q101 - q001),
                 c11 = q011 + fx * (q111 - q011);
    const double c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    *S = c0 + fz * (c1 - c0);
    return true;
}

/* the march of one ray over samples k_first .. k_last (the definition: 0 .. DVO_RAYCAST_MAX_STEPS, it ends at z_far by itself).
 * true: a hit at camera depth *Zs */
DVO_TSDF_HD bool march(const unsigned *words, const RayVolume &rv, const RayCamera &c, const RayConst &rc, double xn, double yn, int k_first,
                       int k_last, double *Zs) {
    bool prev_valid = false;
    double S_prev = 0.0;
    for (int k = k_first; k <= k_last; k++) {
        const double Z = sample_depth(rc.z_near, c.step, k);
        if (!(Z <= rc.z_far)) return false;
        double g[3], S = 0.0;
        ray_point(rv, c, xn, yn, Z, g);
        const bool valid = sample(words, rv, rc.min_weight, g[0], g[1], g[2], &S);
        if (valid && S <= 0.0) {
            if (!(k > 0 && prev_valid && S_prev > 0.0)) return false;
            *Zs = sample_depth(rc.z_near, c.step, k - 1) + c.step * (S_prev / (S_prev - S));
            return true;
        }
        prev_valid = valid;
        S_prev = S;
    }
    return false;
}

/* the normal at camera depth Zs of the ray; false: (0, 0, 0) */
DVO_TSDF_HD bool normal(const unsigned *words, const RayVolume &rv, const RayCamera &c, const RayConst &rc, double xn, double yn, double Zs,
                        float *n3) {
    double g[3], a, b, G[3];
    ray_point(rv, c, xn, yn, Zs, g);
    if (!sample(words, rv, rc.min_weight, g[0] + 1.0, g[1], g[2], &a) || !sample(words, rv, rc.min_weight, g[0] - 1.0, g[1], g[2], &b)) return false;
    G[0] = a - b;
    if (!sample(words, rv, rc.min_weight, g[0], g[1] + 1.0, g[2], &a) || !sample(words, rv, rc.min_weight, g[0], g[1] - 1.0, g[2], &b)) return false;
    G[1] = a - b;
    if (!sample(words, rv, rc.min_weight, g[0], g[1], g[2] + 1.0, &a) || !sample(words, rv, rc.min_weight, g[0], g[1], g[2] - 1.0, &b)) return false;
    G[2] = a - b;
    const double GG = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2];
    if (!(GG > 0.0)) return false;
    const double len = sqrt(GG);
    n3[0] = (float)(G[0] / len); n3[1] = (float)(G[1] / len); n3[2] = (float)(G[2] / len);
    return true;
}

/* A range of k outside which no sample of the ray (xn, yn) lies inside the volume's box, so that march(k_first .. k_last) is the
 * whole march.  A sample is inside on an axis only if 0 <= g <= n - 1.  g is, up to rounding, the line a Z + b with
 * a = (R_row . (xn, yn, 1)) inv_vs and b = (t - origin) inv_vs; every one of the few roundings in ray_point, in a and in b is relative
 * to a magnitude below M = (|R0 xn| + |R3 yn| + |R6|) z_far + |t| + |origin|, times inv_vs: 1e-9 M is millions of them.  The slab
 * [-1 - 1e-9 M, n + 1e-9 M] is cut in Z, and the k range of that interval is widened by two samples on either side.  Anything not
 * finite, or an empty cut (first > last: the ray misses the box and march() returns a hole at once), is handled by the caller's loop;
 * a line that cannot be cut safely keeps the whole range */
DVO_TSDF_HD void clip(const RayVolume &rv, const RayCamera &c, const RayConst &rc, double xn, double yn, int *k_first, int *k_last) {
    int first = 0, last = kRaycastMaxSteps;
    double lo = rc.z_near, hi = rc.z_far;
    const int dim[3] = {rv.nx, rv.ny, rv.nz};
    bool ok = true;
    for (int a = 0; a < 3; a++) {
        const double d = (c.R[a] * xn + c.R[3 + a] * yn) + c.R[6 + a];
        const double M = ((fabs(c.R[a] * xn) + fabs(c.R[3 + a] * yn) + fabs(c.R[6 + a])) * rc.z_far + fabs(c.t[a]) + fabs(rv.origin[a])) * rv.inv_vs;
        const double slope = d * rv.inv_vs, at0 = (c.t[a] - rv.origin[a]) * rv.inv_vs, pad = 1.0 + 1e-9 * M;
        const double g_lo = -pad, g_hi = (double)dim[a] + pad;
        if (!finite(slope) || !finite(at0) || !finite(pad)) { ok = false; break; }
        if (fabs(slope) * rc.z_far <= 1e-9 * M + 1e-300) {                /* as good as parallel to the slab: inside for all Z or for none */
            if (at0 < g_lo - pad || at0 > g_hi + pad) { lo = 1.0; hi = 0.0; break; }
            continue;
        }
        double z0 = (g_lo - at0) / slope, z1 = (g_hi - at0) / slope;
        if (z0 > z1) { const double s = z0; z0 = z1; z1 = s; }
        if (z0 > lo) lo = z0;
        if (z1 < hi) hi = z1;
    }
    if (ok && finite(lo) && finite(hi)) {
        if (lo > hi) { first = 1; last = 0; }
        else {
            const double kf = floor((lo - rc.z_near) / c.step) - 2.0, kl = floor((hi - rc.z_near) / c.step) + 3.0;
            if (kf > 0.0) first = kf < (double)kRaycastMaxSteps ? (int)kf : kRaycastMaxSteps;
            if (kl < (double)kRaycastMaxSteps) last = kl > 0.0 ? (int)kl : 0;
        }
    }
    *k_first = first; *k_last = last;
}

/* the raw depth value of a ray: hit and Z* -> what goes into the image */
DVO_TSDF_HD float depth_f32(bool hit, double Zs) { return hit ? (float)Zs : 0.0f; }
DVO_TSDF_HD unsigned short depth_u16(bool hit, double Zs) {
    if (!hit) return 0;
    const double m = rint(Zs * 1000.0);
    if (!(m >= 1.0 && m <= 65535.0)) return 0;
    return (unsigned short)(int)m;
}

/* pixel (u, v) of one view: its depth into depth_out and, unless NULL, its normal into normals_out.  clipped: march the range of
 * clip() instead of every k (the same result).  true: a hit (after the u16 rule) on the ray ray2 = (xn, yn) at camera depth *Zs_out --
 * what the colour of the pixel (dvo_tsdf_colour.h) starts from */
DVO_TSDF_HD bool pixel_hit(const unsigned *words, const RayVolume &rv, const RayCamera &c, const RayConst &rc, int u, int v, bool clipped,
                           void *depth_out, float *normals_out, double *ray2, double *Zs_out) {
    const double xn = ((double)u - c.K[2]) / c.K[0], yn = ((double)v - c.K[3]) / c.K[1];
    int k_first = 0, k_last = kRaycastMaxSteps;
    if (clipped) clip(rv, c, rc, xn, yn, &k_first, &k_last);
    double Zs = 0.0;
    bool hit = march(words, rv, c, rc, xn, yn, k_first, k_last, &Zs);
    const size_t px = (size_t)v * (size_t)rc.cols + (size_t)u;
    if (rc.depth_format == kFormatU16) {
        const unsigned short m = depth_u16(hit, Zs);
        static_cast<unsigned short *>(depth_out)[px] = m;
        hit = m != 0;
    } else {
        static_cast<float *>(depth_out)[px] = depth_f32(hit, Zs);
    }
    if (normals_out) {
        float n3[3];
        if (!hit || !normal(words, rv, c, rc, xn, yn, Zs, n3)) n3[0] = n3[1] = n3[2] = 0.0f;
        normals_out[3 * px] = n3[0]; normals_out[3 * px + 1] = n3[1]; normals_out[3 * px + 2] = n3[2];
    }
    ray2[0] = xn; ray2[1] = yn; *Zs_out = Zs;
    return hit;
}
DVO_TSDF_HD void pixel(const unsigned *words, const RayVolume &rv, const RayCamera &c, const RayConst &rc, int u, int v, bool clipped,
                       void *depth_out, float *normals_out) {
    double ray2[2], Zs;
    (void)pixel_hit(words, rv, c, rc, u, v, clipped, depth_out, normals_out, ray2, &Zs);
}

inline RayCamera ray_camera(const double *K4, const double *pose12, double step) {
    RayCamera c;
    for (int k = 0; k < 9; k++) c.R[k] = pose12[k];
    for (int k = 0; k < 3; k++) c.t[k] = pose12[9 + k];
    for (int k = 0; k < 4; k++) c.K[k] = K4[k];
    c.step = step;
    return c;
}

/* ---- the entry point ---- */

/* views 0 .. count - 1 of one volume: depth_out[i] rows x cols of depth_format; normals_out NULL, or normals_out[i] 3 rows x cols
 * floats.  clipped: see pixel().  False: refused, nothing written */
inline bool raycast(const dvo_tsdf_volume *vol, const unsigned *voxels, const dvo_raycast_params *p, int count, int depth_format, int rows, int cols,
                    const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out, bool clipped = false) {
    if (!volume_ok(vol) || !voxels || !raycast_params_ok(p) || count < 1 || !format_ok(depth_format) || rows < 1 || cols < 1 || !K4 || !poses12 ||
        !depth_out)
        return false;
    if (march_samples(*p, vol->trunc) < 0) return false;
    for (int i = 0; i < count; i++)
        if (!depth_out[i] || (normals_out && !normals_out[i]) || !frame_ok(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i)) return false;
    const RayVolume rv = ray_volume(*vol);
    RayConst rc;
    rc.depth_format = depth_format; rc.rows = rows; rc.cols = cols; rc.min_weight = p->min_weight; rc.z_near = p->z_near; rc.z_far = p->z_far;
    for (int i = 0; i < count; i++) {
        const RayCamera c = ray_camera(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i, p->step_trunc * vol->trunc);
        for (int v = 0; v < rows; v++)
            for (int u = 0; u < cols; u++) pixel(voxels, rv, c, rc, u, v, clipped, depth_out[i], normals_out ? normals_out[i] : nullptr);
    }
    return true;
}

}  // namespace dvo_tsdf
#endif
