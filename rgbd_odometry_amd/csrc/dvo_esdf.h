/*
 * dvo_esdf.h -- Euclidean signed distance fields of fused volumes (include/dvo_amd.h, "distance fields"): the definition, in plain C++.
 * No device, no context: dvo_esdf_host is esdf() below, dvo_esdf_distances_host is esdf_distances(), dvo_esdf_query_host is
 * esdf_query(); the device kernels (dvo_esdf.hip) share esdf_flags(), esdf_metres() and esdf_query_point() -- the whole per-voxel and
 * per-point functions -- with them, and a stand-alone program can include the file as it is.  The rules of dvo_tsdf_map.h hold:
 * -ffp-contract=off, no transcendental function, sqrt and division only in double (both correctly rounded).
 *
 * Per voxel a of one volume, with q, w from its TSDF word (word_q, word_w of dvo_tsdf_map.h):
 *   observed(a) = w >= min_weight; inside(a) = observed(a) && q < 0 (the sign test of a crossing of extract());
 *   a is a SURFACE SITE when it is observed and one of its up to six axis neighbours b (+-1 along x, y, z, inside the volume) is observed
 *   with (qa < 0) != (qb < 0): both sides of a crossing are sites.  With sites == DVO_ESDF_SITES_SURFACE_AND_UNKNOWN every voxel that is
 *   not observed is a site too (unknown space is an obstacle);
 *   d2(a) = the minimum over all sites s of (ax - sx)^2 + (ay - sy)^2 + (az - sz)^2, an integer of at most 3 * 1023^2 = 3 139 587;
 *   DVO_ESDF_NO_SITE = 0xFFFFFF when the volume has no site.
 * The ESDF word, 32 bits, one per voxel at the voxel's index: bits 0..23 d2, bit 30 inside, bit 31 !observed, every other bit 0.  The
 * word is the contract: an integer with no order of summation and no ties.
 *
 * What the number means.  esdf_metres() is voxel_size * sqrt(d2), negative inside: the distance to the CENTRE of the nearest site voxel,
 * not to the surface.  Every surface site lies within one voxel_size of the surface, so the value is within one voxel_size of the
 * distance to the surface, and within trunc of the surface the TSDF itself is the better value.
 *
 * esdf() computes d2 by three separable passes of the exact min-plus transform out[i] = min_j (f[j] + (i - j)^2): along x from the site
 * flags, then along y, then along z.  Each output scans j = i -+ k outwards and stops when k^2 >= the best value so far -- no j further
 * out can improve it -- which is exact and needs no stack.  A volume without any site costs a full column per voxel that way; esdf()
 * skips the passes for it.
 */
#ifndef DVO_ESDF_H_
#define DVO_ESDF_H_

#include "dvo_tsdf_map.h"

#include <new>
#include <vector>

/* the public structs as include/dvo_amd.h declares them (the same text under the same guard: whichever header comes first defines them) */
#ifndef DVO_ESDF_TYPES_DEFINED_
#define DVO_ESDF_TYPES_DEFINED_
#define DVO_ESDF_SITES_SURFACE 0                 /* sites: the voxels on either side of a sign change between observed neighbours */
#define DVO_ESDF_SITES_SURFACE_AND_UNKNOWN 1     /* and every voxel that is not observed */
#define DVO_ESDF_NO_SITE 0xFFFFFFu               /* d2 of every voxel of a volume without a site */
#define DVO_ESDF_INSIDE 0x40000000u              /* bit 30 of an ESDF word: observed with q < 0 */
#define DVO_ESDF_UNKNOWN 0x80000000u             /* bit 31: not observed (w < min_weight) */
#define DVO_ESDF_FOUND 0                         /* dvo_esdf_sample.status: distance and gradient are set */
#define DVO_ESDF_OUTSIDE 1                       /* the point's cell is not inside the lattice (or the point is not finite) */
#define DVO_ESDF_NO_DISTANCE 2                   /* a corner of the cell has d2 == DVO_ESDF_NO_SITE */
typedef struct dvo_esdf_params {
    int min_weight;                      /* a voxel is observed with this many observations: >= 1 */
    int sites;                           /* DVO_ESDF_SITES_SURFACE or DVO_ESDF_SITES_SURFACE_AND_UNKNOWN */
} dvo_esdf_params;
typedef struct dvo_esdf_sample {
    int    status;                       /* DVO_ESDF_FOUND, DVO_ESDF_OUTSIDE or DVO_ESDF_NO_DISTANCE */
    int    unknown;                      /* corners of the cell that are not observed (bit 31): 0 when OUTSIDE */
    double distance;                     /* metres, negative inside; 0 unless FOUND */
    double gradient[3];                  /* d distance / d P, world axes; 0 unless FOUND */
} dvo_esdf_sample;
#endif

namespace dvo_tsdf {

constexpr unsigned kEsdfNoSite = DVO_ESDF_NO_SITE, kEsdfInside = DVO_ESDF_INSIDE, kEsdfUnknown = DVO_ESDF_UNKNOWN;
constexpr unsigned kEsdfD2Mask = 0xFFFFFFu;

inline void esdf_params_default(dvo_esdf_params *p) { p->min_weight = 1; p->sites = DVO_ESDF_SITES_SURFACE; }
inline bool esdf_params_ok(const dvo_esdf_params *p) {
    return p && p->min_weight >= 1 && (p->sites == DVO_ESDF_SITES_SURFACE || p->sites == DVO_ESDF_SITES_SURFACE_AND_UNKNOWN);
}

/* ---- the per-voxel functions, shared with the device ---- */

DVO_TSDF_HD bool esdf_observed(unsigned word, int min_weight) { return word_w(word) >= min_weight; }
/* the flag bits of voxel (x, y, z) -- kEsdfInside, kEsdfUnknown -- and whether it is a site.  words: the volume's TSDF words */
DVO_TSDF_HD unsigned esdf_flags(const unsigned *words, int nx, int ny, int nz, int x, int y, int z, int min_weight, int sites, bool *site) {
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny, a = (size_t)x + sy * (size_t)y + sz * (size_t)z;
    const unsigned wa = words[a];
    if (!esdf_observed(wa, min_weight)) {
        *site = sites == DVO_ESDF_SITES_SURFACE_AND_UNKNOWN;
        return kEsdfUnknown;
    }
    const bool neg = word_q(wa) < 0;
    bool s = false;
    if (x > 0)      { const unsigned wb = words[a - 1];  s = s || (esdf_observed(wb, min_weight) && (word_q(wb) < 0) != neg); }
    if (x + 1 < nx) { const unsigned wb = words[a + 1];  s = s || (esdf_observed(wb, min_weight) && (word_q(wb) < 0) != neg); }
    if (y > 0)      { const unsigned wb = words[a - sy]; s = s || (esdf_observed(wb, min_weight) && (word_q(wb) < 0) != neg); }
    if (y + 1 < ny) { const unsigned wb = words[a + sy]; s = s || (esdf_observed(wb, min_weight) && (word_q(wb) < 0) != neg); }
    if (z > 0)      { const unsigned wb = words[a - sz]; s = s || (esdf_observed(wb, min_weight) && (word_q(wb) < 0) != neg); }
    if (z + 1 < nz) { const unsigned wb = words[a + sz]; s = s || (esdf_observed(wb, min_weight) && (word_q(wb) < 0) != neg); }
    *site = s;
    return neg ? kEsdfInside : 0u;
}

/* One output of the min-plus transform along a line: min over j in [0, n) of d2(line[j * stride]) + (i - j)^2, the entries with
 * d2 == kEsdfNoSite left out; kEsdfNoSite when there is none.  The scan goes outwards from i and stops at the first k with k^2 >= the
 * best so far, or when both i - k and i + k have left the line.  line: ESDF words (only their d2 is read) */
DVO_TSDF_HD unsigned esdf_scan(const unsigned *line, size_t stride, int n, int i) {
    unsigned best = line[(size_t)i * stride] & kEsdfD2Mask;
    for (int k = 1; k < n; k++) {
        const unsigned kk = (unsigned)k * (unsigned)k;
        if (kk >= best) break;
        const int lo = i - k, hi = i + k;
        if (lo < 0 && hi >= n) break;
        if (lo >= 0) {
            const unsigned f = line[(size_t)lo * stride] & kEsdfD2Mask;
            if (f != kEsdfNoSite && f + kk < best) best = f + kk;
        }
        if (hi < n) {
            const unsigned f = line[(size_t)hi * stride] & kEsdfD2Mask;
            if (f != kEsdfNoSite && f + kk < best) best = f + kk;
        }
    }
    return best;
}

/* the signed distance of a word in metres, as a double: voxel_size * sqrt(d2), negated inside; d2 != kEsdfNoSite */
DVO_TSDF_HD double esdf_signed(unsigned word, double voxel_size) {
    const double d = voxel_size * sqrt((double)(word & kEsdfD2Mask));
    return (word & kEsdfInside) ? -d : d;
}
/* metres from a word: the distance to the centre of the nearest site voxel, negative inside; +-INFINITY for kEsdfNoSite */
DVO_TSDF_HD float esdf_metres(unsigned word, double voxel_size) {
    if ((word & kEsdfD2Mask) == kEsdfNoSite) return (word & kEsdfInside) ? -INFINITY : INFINITY;
    return (float)esdf_signed(word, voxel_size);
}

/* The point query.  For a world point P, per axis k: g_k = (P_k - origin_k) / voxel_size, i_k = floor(g_k); OUTSIDE unless 0 <= i_k and
 * i_k + 1 <= n_k - 1 on all three axes, compared in double (a NaN falls out; so does an infinity).  The eight corners
 * v[dz][dy][dx] = esdf_signed(word at (i_x + dx, i_y + dy, i_z + dz)); `unknown` counts the corners with bit 31; NO_DISTANCE when a
 * corner has d2 == kEsdfNoSite.  Otherwise, with f_k = g_k - i_k, trilinear along x, then y, then z, every step a + f * (b - a):
 *   c00 = v000 + fx * (v001 - v000)   c10 = v010 + fx * (v011 - v010)   c01 = v100 + fx * (v101 - v100)   c11 = v110 + fx * (v111 - v110)
 *   c0 = c00 + fy * (c10 - c00)       c1 = c01 + fy * (c11 - c01)       distance = c0 + fz * (c1 - c0)
 * and the gradient is the analytic derivative of that form, divided by voxel_size:
 *   x00 = v001 - v000, x10 = v011 - v010, x01 = v101 - v100, x11 = v111 - v110; x0 = x00 + fy * (x10 - x00), x1 = x01 + fy * (x11 - x01);
 *   gradient[0] = (x0 + fz * (x1 - x0)) / voxel_size
 *   y0 = c10 - c00, y1 = c11 - c01; gradient[1] = (y0 + fz * (y1 - y0)) / voxel_size
 *   gradient[2] = (c1 - c0) / voxel_size
 * (the index digits of v are dz dy dx).  words: the volume's ESDF words */
DVO_TSDF_HD dvo_esdf_sample esdf_query_point(const VolumeConst &vc, const unsigned *words, double px, double py, double pz) {
    dvo_esdf_sample r;
    r.status = DVO_ESDF_OUTSIDE; r.unknown = 0; r.distance = 0.0; r.gradient[0] = 0.0; r.gradient[1] = 0.0; r.gradient[2] = 0.0;
    const double gx = (px - vc.origin[0]) / vc.voxel_size, gy = (py - vc.origin[1]) / vc.voxel_size, gz = (pz - vc.origin[2]) / vc.voxel_size;
    const double ix = floor(gx), iy = floor(gy), iz = floor(gz);
    if (!(ix >= 0.0 && ix + 1.0 <= (double)(vc.nx - 1) && iy >= 0.0 && iy + 1.0 <= (double)(vc.ny - 1) && iz >= 0.0 && iz + 1.0 <= (double)(vc.nz - 1)))
        return r;
    const double fx = gx - ix, fy = gy - iy, fz = gz - iz;
    const size_t sy = (size_t)vc.nx, sz = (size_t)vc.nx * (size_t)vc.ny, a = (size_t)(int)ix + sy * (size_t)(int)iy + sz * (size_t)(int)iz;
    unsigned w[8];
    bool none = false;
    for (int c = 0; c < 8; c++) {
        w[c] = words[a + (size_t)(c & 1) + sy * (size_t)((c >> 1) & 1) + sz * (size_t)(c >> 2)];
        if (w[c] & kEsdfUnknown) r.unknown++;
        if ((w[c] & kEsdfD2Mask) == kEsdfNoSite) none = true;
    }
    if (none) { r.status = DVO_ESDF_NO_DISTANCE; return r; }
    double v[8];
    for (int c = 0; c < 8; c++) v[c] = esdf_signed(w[c], vc.voxel_size);
    const double c00 = v[0] + fx * (v[1] - v[0]), c10 = v[2] + fx * (v[3] - v[2]), c01 = v[4] + fx * (v[5] - v[4]), c11 = v[6] + fx * (v[7] - v[6]);
    const double c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    const double x00 = v[1] - v[0], x10 = v[3] - v[2], x01 = v[5] - v[4], x11 = v[7] - v[6];
    const double x0 = x00 + fy * (x10 - x00), x1 = x01 + fy * (x11 - x01);
    const double y0 = c10 - c00, y1 = c11 - c01;
    r.status = DVO_ESDF_FOUND;
    r.distance = c0 + fz * (c1 - c0);
    r.gradient[0] = (x0 + fz * (x1 - x0)) / vc.voxel_size;
    r.gradient[1] = (y0 + fz * (y1 - y0)) / vc.voxel_size;
    r.gradient[2] = (c1 - c0) / vc.voxel_size;
    return r;
}

/* ---- the entry points ---- */

/* the ESDF words of one volume from its TSDF words.  False: refused, nothing written.  Throws std::bad_alloc when the one scratch copy
 * of the words (4 bytes per voxel) cannot be had */
inline bool esdf(const dvo_tsdf_volume *vol, const unsigned *voxels, const dvo_esdf_params *p, unsigned *words_out) {
    if (!volume_ok(vol) || !voxels || !esdf_params_ok(p) || !words_out) return false;
    const int nx = vol->nx, ny = vol->ny, nz = vol->nz;
    const size_t n = voxels_of(*vol), sy = (size_t)nx, sz = (size_t)nx * (size_t)ny;
    std::vector<unsigned> tmp(n);
    unsigned *const A = words_out, *const B = tmp.data();
    /* pass x, fused with the classification: the nearest site of the row on either side, by two sweeps */
    bool any = false;
    size_t a = 0;
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++) {
            unsigned *row = A + a;
            int last = -1;
            for (int x = 0; x < nx; x++, a++) {
                bool site;
                const unsigned flags = esdf_flags(voxels, nx, ny, nz, x, y, z, p->min_weight, p->sites, &site);
                if (site) { last = x; any = true; }
                row[x] = flags | (last < 0 ? kEsdfNoSite : (unsigned)((x - last) * (x - last)));
            }
            if (last < 0) continue;
            int next = -1;
            for (int x = nx - 1; x >= 0; x--) {
                if ((row[x] & kEsdfD2Mask) == 0u) next = x;
                if (next >= 0 && (unsigned)((next - x) * (next - x)) < (row[x] & kEsdfD2Mask))
                    row[x] = (row[x] & ~kEsdfD2Mask) | (unsigned)((next - x) * (next - x));
            }
        }
    if (!any) return true;                         /* every d2 is kEsdfNoSite already */
    /* pass y: A -> B; pass z: B -> A.  A pass's outputs are other outputs' inputs, so none runs in place */
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                const size_t i = (size_t)x + sy * (size_t)y + sz * (size_t)z;
                B[i] = (A[i] & ~kEsdfD2Mask) | esdf_scan(A + (size_t)x + sz * (size_t)z, sy, ny, y);
            }
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                const size_t i = (size_t)x + sy * (size_t)y + sz * (size_t)z;
                A[i] = (B[i] & ~kEsdfD2Mask) | esdf_scan(B + (size_t)x + sy * (size_t)y, sz, nz, z);
            }
    return true;
}

/* esdf_metres() of every word of a volume.  False: refused, nothing written */
inline bool esdf_distances(const dvo_tsdf_volume *vol, const unsigned *words, float *out) {
    if (!volume_ok(vol) || !words || !out) return false;
    const size_t n = voxels_of(*vol);
    for (size_t i = 0; i < n; i++) out[i] = esdf_metres(words[i], vol->voxel_size);
    return true;
}

/* esdf_query_point() of `count` points (xyz: 3 doubles each).  False: refused -- a point that is not finite included -- nothing written */
inline bool esdf_query(const dvo_tsdf_volume *vol, const unsigned *words, int count, const double *xyz, dvo_esdf_sample *records) {
    if (!volume_ok(vol) || !words || count < 1 || !xyz || !records) return false;
    for (size_t i = 0; i < 3 * (size_t)count; i++)
        if (!finite(xyz[i])) return false;
    const VolumeConst vc = volume_const(*vol);
    for (size_t i = 0; i < (size_t)count; i++) records[i] = esdf_query_point(vc, words, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return true;
}

}  // namespace dvo_tsdf
#endif
