/*
 * dvo_tsdf_map.h -- depth fusion into truncated-signed-distance volumes (include/dvo_amd.h, "depth fusion"): the definition, in plain
 * C++.  No device, no context, no other header of the library: dvo_tsdf_integrate_host is integrate() below, dvo_tsdf_extract_host is
 * extract(), the device kernels (dvo_tsdf_map.hip) share update() and crossing() -- the whole per-voxel functions -- with them, and a
 * stand-alone program can include the file as it is.  update() is project() followed by blend(): the colour path (dvo_tsdf_colour.h)
 * runs the same two parts with its own blend between them.
 *
 * A volume is nx * ny * nz voxels, voxel (ix, iy, iz) at index ix + nx * (iy + ny * iz), its centre at origin + voxel_size * (ix, iy,
 * iz) in the world.  One voxel is one 32-bit word: low 16 bits q (int16: the truncated distance in units of trunc / 32767), high 16
 * bits w (uint16: observations).  Word 0 = never seen.  A frame is a depth image (rows x cols, row-major, 16-bit millimetres or float
 * metres; a pinhole camera taken as undistorted and registered), K4 = fx, fy, cx, cy and a pose {R column-major, t}, camera to world.
 *
 * All arithmetic is IEEE double in the order written, nothing fused (-ffp-contract=off), no transcendental function, no float: host,
 * device and a numpy restatement agree bit for bit.  Every voxel position comes from the direct formula origin + voxel_size * i, never
 * from stepping along an axis.  A voxel's new word depends on its old word and the frame alone, and a frame list is applied in list
 * order, so the device result is byte-equal under any schedule and any batch.
 */
#ifndef DVO_TSDF_MAP_H_
#define DVO_TSDF_MAP_H_

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define DVO_TSDF_HD __host__ __device__ inline
#else
#define DVO_TSDF_HD inline
#endif

/* the public structs as include/dvo_amd.h declares them (the same text under the same guard: whichever header comes first defines them) */
#ifndef DVO_TSDF_TYPES_DEFINED_
#define DVO_TSDF_TYPES_DEFINED_
#define DVO_TSDF_MAX_DIM 1024            /* voxels along one axis */
typedef struct dvo_tsdf_volume {
    int    nx, ny, nz;                   /* each in [1, DVO_TSDF_MAX_DIM]; voxel (ix, iy, iz) at index ix + nx * (iy + ny * iz) */
    double voxel_size;                   /* metres, > 0 */
    double origin[3];                    /* world position of the centre of voxel (0, 0, 0) */
    double trunc;                        /* truncation distance, metres, > 0 */
} dvo_tsdf_volume;
typedef struct dvo_tsdf_params {
    double z_near, z_far;                /* metres: a voxel at camera depth <= z_near, a measurement beyond z_far are skipped */
    int    max_weight;                   /* the observation count saturates here: [1, 65535] */
} dvo_tsdf_params;
#endif

namespace dvo_tsdf {

constexpr int kFormatF32 = 0, kFormatU16 = 1;      /* == DVO_DEPTH_F32, DVO_DEPTH_U16 */
constexpr int kMaxDim = DVO_TSDF_MAX_DIM;
constexpr double kQMax = 32767.0;

/* finite: neither NaN nor an infinity (x - x is NaN for both) */
DVO_TSDF_HD bool finite(double x) { return x - x == 0.0; }

inline void params_default(dvo_tsdf_params *p) { p->z_near = 0.1; p->z_far = 8.0; p->max_weight = 128; }

/* ---- what every public call refuses ---- */
inline bool volume_ok(const dvo_tsdf_volume *v) {
    if (!v || v->nx < 1 || v->ny < 1 || v->nz < 1 || v->nx > kMaxDim || v->ny > kMaxDim || v->nz > kMaxDim) return false;
    if (!finite(v->voxel_size) || !(v->voxel_size > 0.0) || !finite(v->trunc) || !(v->trunc > 0.0)) return false;
    return finite(v->origin[0]) && finite(v->origin[1]) && finite(v->origin[2]);
}
inline bool params_ok(const dvo_tsdf_params *p) {
    return p && finite(p->z_near) && finite(p->z_far) && p->z_near > 0.0 && p->z_near < p->z_far && p->max_weight >= 1 && p->max_weight <= 65535;
}
inline bool format_ok(int depth_format) { return depth_format == kFormatF32 || depth_format == kFormatU16; }
/* one frame's camera and pose: every number finite, fx and fy positive.  R is taken as given (not checked for orthogonality) */
inline bool frame_ok(const double *K4, const double *pose12) {
    if (!K4 || !pose12) return false;
    for (int k = 0; k < 4; k++) if (!finite(K4[k])) return false;
    for (int k = 0; k < 12; k++) if (!finite(pose12[k])) return false;
    return K4[0] > 0.0 && K4[1] > 0.0;
}
inline size_t voxels_of(const dvo_tsdf_volume &v) { return (size_t)v.nx * (size_t)v.ny * (size_t)v.nz; }
inline size_t depth_pixel_bytes(int depth_format) { return depth_format == kFormatU16 ? 2 : 4; }

/* ---- the per-voxel functions, shared with the device ---- */

/* what a volume contributes to every voxel's update; inv_trunc = 1.0 / trunc, computed once per volume */
struct VolumeConst {
    int nx, ny, nz, pad_;
    double voxel_size, origin[3], trunc, inv_trunc;
};
DVO_TSDF_HD VolumeConst volume_const(const dvo_tsdf_volume &v) {
    VolumeConst c;
    c.nx = v.nx; c.ny = v.ny; c.nz = v.nz; c.pad_ = 0;
    c.voxel_size = v.voxel_size;
    c.origin[0] = v.origin[0]; c.origin[1] = v.origin[1]; c.origin[2] = v.origin[2];
    c.trunc = v.trunc;
    c.inv_trunc = 1.0 / v.trunc;
    return c;
}
/* one frame: pose {R column-major, t} camera to world, K = fx, fy, cx, cy, and where its image is */
struct Frame {
    double R[9], t[3], K[4];
    const void *depth;
    long long pad_;
};
struct FrameConst { int depth_format, rows, cols, max_weight; double z_near, z_far; };

/* the centre of voxel index i along one axis: the direct formula */
DVO_TSDF_HD double centre(double origin, double voxel_size, int i) { return origin + voxel_size * (double)i; }

/* metres of a raw value; false: a hole */
DVO_TSDF_HD bool metres_u16(unsigned short r, double *D) {
    if (r == 0) return false;
    *D = (double)r / 1000.0;
    return true;
}
DVO_TSDF_HD bool metres_f32(float r, double *D) {
    const double d = (double)r;
    if (!finite(d) || !(d > 0.0)) return false;
    *D = d;
    return true;
}

DVO_TSDF_HD int word_q(unsigned word) { return (int)(short)(unsigned short)(word & 0xFFFFu); }
DVO_TSDF_HD int word_w(unsigned word) { return (int)(word >> 16); }
DVO_TSDF_HD unsigned make_word(int q, int w) { return ((unsigned)w << 16) | ((unsigned)q & 0xFFFFu); }

/* update() in two parts, shared with the colour path (dvo_tsdf_colour.h).  project(): the voxel whose centre is (wx, wy, wz) seen from
 * frame f; false: skipped.  *px: the pixel its depth was read from (row-major index); *sdf: measured depth - the voxel's, >= -trunc */
DVO_TSDF_HD bool project(double wx, double wy, double wz, const VolumeConst &vc, const Frame &f, const FrameConst &fc, size_t *px_out, double *sdf_out) {
    const double dx = wx - f.t[0], dy = wy - f.t[1], dz = wz - f.t[2];
    const double X = f.R[0] * dx + f.R[1] * dy + f.R[2] * dz;
    const double Y = f.R[3] * dx + f.R[4] * dy + f.R[5] * dz;
    const double Z = f.R[6] * dx + f.R[7] * dy + f.R[8] * dz;
    if (!(Z > fc.z_near)) return false;
    const double iz = 1.0 / Z;
    const double u = f.K[0] * (X * iz) + f.K[2];
    const double v = f.K[1] * (Y * iz) + f.K[3];
    const double ui = floor(u + 0.5), vi = floor(v + 0.5);
    if (!(ui >= 0.0 && ui < (double)fc.cols && vi >= 0.0 && vi < (double)fc.rows)) return false;      /* NaN falls out here */
    const size_t px = (size_t)(int)vi * (size_t)fc.cols + (size_t)(int)ui;
    double D;
    if (fc.depth_format == kFormatU16 ? !metres_u16(static_cast<const unsigned short *>(f.depth)[px], &D)
                                      : !metres_f32(static_cast<const float *>(f.depth)[px], &D))
        return false;
    if (D > fc.z_far) return false;
    const double sdf = D - Z;
    if (sdf < -vc.trunc) return false;
    *px_out = px; *sdf_out = sdf;
    return true;
}
/* blend(): the word after a measurement of signed distance sdf */
DVO_TSDF_HD unsigned blend(unsigned word, double sdf, const VolumeConst &vc, const FrameConst &fc) {
    double fr = sdf * vc.inv_trunc;
    if (fr > 1.0) fr = 1.0;
    const double F = fr * kQMax;
    const int q = word_q(word), w = word_w(word);
    const int qn = (int)rint(((double)q * (double)w + F) / ((double)w + 1.0));      /* round half to even */
    const int wn = w + 1 < fc.max_weight ? w + 1 : fc.max_weight;
    return make_word(qn, wn);
}
/* the word of the voxel whose centre is (wx, wy, wz) after frame f; a skipped voxel keeps its word */
DVO_TSDF_HD unsigned update(unsigned word, double wx, double wy, double wz, const VolumeConst &vc, const Frame &f, const FrameConst &fc) {
    size_t px;
    double sdf;
    if (!project(wx, wy, wz, vc, f, fc, &px, &sdf)) return word;
    return blend(word, sdf, vc, fc);
}

/* the surface point between voxel a (index ia along `axis`, word wa) and its neighbour b (ia + 1, word wb); false: no crossing.
 * cx, cy, cz: the centre of a */
DVO_TSDF_HD bool crossing(unsigned wa, unsigned wb, int min_weight, int axis, double cx, double cy, double cz, double voxel_size, float *xyz) {
    if (word_w(wa) < min_weight || word_w(wb) < min_weight) return false;
    const int qa = word_q(wa), qb = word_q(wb);
    if ((qa < 0) == (qb < 0)) return false;
    const double lambda = (double)qa / (double)(qa - qb);
    const double move = lambda * voxel_size;
    xyz[0] = (float)(axis == 0 ? cx + move : cx);
    xyz[1] = (float)(axis == 1 ? cy + move : cy);
    xyz[2] = (float)(axis == 2 ? cz + move : cz);
    return true;
}
/* the word offset from a voxel to its neighbour along `axis` */
DVO_TSDF_HD size_t axis_step(const VolumeConst &vc, int axis) { return axis == 0 ? 1 : axis == 1 ? (size_t)vc.nx : (size_t)vc.nx * (size_t)vc.ny; }

/* ---- the entry points ---- */

/* frames 0 .. count - 1, in this order, into the words of one volume.  depth[i]: rows x cols of depth_format; K4: 4 doubles per frame;
 * poses12: 12 per frame.  False: refused, nothing written */
inline bool integrate(const dvo_tsdf_volume *vol, unsigned *voxels, const dvo_tsdf_params *p, int count, const void *const *depth,
                      int depth_format, int rows, int cols, const double *K4, const double *poses12) {
    if (!volume_ok(vol) || !voxels || !params_ok(p) || count < 1 || !depth || !format_ok(depth_format) || rows < 1 || cols < 1 || !K4 || !poses12)
        return false;
    for (int i = 0; i < count; i++)
        if (!depth[i] || !frame_ok(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i)) return false;
    const VolumeConst vc = volume_const(*vol);
    FrameConst fc;
    fc.depth_format = depth_format; fc.rows = rows; fc.cols = cols; fc.max_weight = p->max_weight; fc.z_near = p->z_near; fc.z_far = p->z_far;
    for (int i = 0; i < count; i++) {
        Frame f;
        for (int k = 0; k < 9; k++) f.R[k] = poses12[12 * (size_t)i + k];
        for (int k = 0; k < 3; k++) f.t[k] = poses12[12 * (size_t)i + 9 + k];
        for (int k = 0; k < 4; k++) f.K[k] = K4[4 * (size_t)i + k];
        f.depth = depth[i]; f.pad_ = 0;
        size_t a = 0;
        for (int z = 0; z < vc.nz; z++) {
            const double wz = centre(vc.origin[2], vc.voxel_size, z);
            for (int y = 0; y < vc.ny; y++) {
                const double wy = centre(vc.origin[1], vc.voxel_size, y);
                for (int x = 0; x < vc.nx; x++, a++) voxels[a] = update(voxels[a], centre(vc.origin[0], vc.voxel_size, x), wy, wz, vc, f, fc);
            }
        }
    }
    return true;
}

/* the surface points of a volume in the definition's order: voxels in index order, per voxel the axes x, y, z.  *n_points: how many
 * there are; the first `capacity` go to xyz (3 floats each; may be NULL with capacity 0).  False: refused, nothing written */
inline bool extract(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long capacity, long long *n_points) {
    if (!volume_ok(vol) || !voxels || min_weight < 1 || capacity < 0 || (capacity > 0 && !xyz) || !n_points) return false;
    const VolumeConst vc = volume_const(*vol);
    long long n = 0;
    size_t a = 0;
    for (int z = 0; z < vc.nz; z++)
        for (int y = 0; y < vc.ny; y++)
            for (int x = 0; x < vc.nx; x++, a++) {
                const int at[3] = {x, y, z}, dim[3] = {vc.nx, vc.ny, vc.nz};
                const double cx = centre(vc.origin[0], vc.voxel_size, x), cy = centre(vc.origin[1], vc.voxel_size, y),
                             cz = centre(vc.origin[2], vc.voxel_size, z);
                for (int axis = 0; axis < 3; axis++) {
                    if (at[axis] + 1 >= dim[axis]) continue;
                    float pt[3];
                    if (!crossing(voxels[a], voxels[a + axis_step(vc, axis)], min_weight, axis, cx, cy, cz, vc.voxel_size, pt)) continue;
                    if (n < capacity) { xyz[3 * n] = pt[0]; xyz[3 * n + 1] = pt[1]; xyz[3 * n + 2] = pt[2]; }
                    n++;
                }
            }
    *n_points = n;
    return true;
}

}  // namespace dvo_tsdf
#endif
