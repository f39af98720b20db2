/*
 * dvo_tsdf_colour.h -- colour in the fused volumes, the ray-cast views and the meshes (include/dvo_amd.h, "colour in the map"): the
 * definition, in plain C++.  It follows the rules of dvo_tsdf_map.h, dvo_tsdf_raycast.h and dvo_tsdf_mesh.h, which it includes: no
 * device, no context, IEEE double in the order written, nothing fused (-ffp-contract=off).  dvo_colour_integrate_host is
 * integrate_colour() below, dvo_colour_raycast_host raycast_colour(), dvo_colour_mesh_host mesh_colour(); the kernels call the
 * per-voxel, per-pixel and per-vertex functions -- update_colour, pixel_colour, mesh_vertex_colour -- as they are.
 *
 * Colour word.  One 64-bit word per voxel in a second pool laid out exactly like the voxel pool (same offsets, same index
 *   ix + nx (iy + ny iz)): bits 0-15 r, 16-31 g, 32-47 b, each the running mean of the channel in units of 1/256 of an 8-bit level
 *   (0 .. 65280); bits 48-63 wc, the colour observation count.  Word 0 = no colour yet, so clearing is a fill with zero.  Sixteen-bit
 *   channels on purpose: with 8-bit storage and max_weight 128 a running mean stops moving for changes below 65 levels.
 * Fusing a frame.  The depth frame of dvo_tsdf_map.h plus an image of the same rows x cols, registered to the depth, in one of the
 *   engine's formats (BGR8, RGB8: three bytes per pixel; MONO8: one byte g = (g, g, g)).  Per voxel the TSDF word is updated exactly as
 *   update() does; the colour word is updated iff the voxel was not skipped (update()'s tests all passed, up to and including
 *   sdf >= -trunc) and sdf <= trunc, compared in double (sdf == trunc is in): free space further than trunc in front of a surface takes
 *   no colour.  The pixel is the one at (vi, ui) the depth was read from, channels C = R, G, B as integers 0 .. 255.  Integer
 *   arithmetic only: c' = (c wc + 256 C + ((wc + 1) >> 1)) / (wc + 1) per channel, the division truncating (the mean rounds half up;
 *   everything fits in 32 unsigned bits: 65535 * 65535 + 65280 + 32768 < 2^32), wc' = min(wc + 1, max_weight).  A frame list is applied
 *   in list order.
 * A ray-cast pixel's colour.  On a hit (after the u16 rule that turns m outside [1, 65535] into a hole) g* = the voxel coordinates
 *   ray_point() gives at Z* (the point normal() uses); i = floor(g*), f = g* - i per axis with the bounds test of sample(); all eight
 *   corner colour words need wc >= 1 (TSDF weights are not consulted); each channel is the trilinear interpolation of the eight values
 *   as doubles, along x, then y, then z, each step a + f (b - a); the level is L = (int)floor(c / 256.0 + 0.5), clamped to [0, 255].
 *   A hole, an out-of-bounds cell or a corner without colour gives (0, 0, 0).  RGB8 writes (R, G, B), BGR8 (B, G, R), MONO8 the engine's
 *   grey (1868 B + 9617 G + 4899 R + 8192) >> 14.
 * A mesh vertex's colour.  The vertex lies on the owned edge between voxels a and b with the lambda of mesh_vertex().  Both ends have
 *   wc >= 1: each channel is ca + lambda (cb - ca) in double; exactly one end has: that end's values; neither: (0, 0, 0).  The level
 *   comes from the ray caster's formula.  Three bytes per vertex, always R, G, B, in vertex order.
 * Words, depth, normals, vertices, triangles and counts are byte-equal to those of the uncoloured calls.
 */
#ifndef DVO_TSDF_COLOUR_H_
#define DVO_TSDF_COLOUR_H_

#include "dvo_tsdf_map.h"
#include "dvo_tsdf_raycast.h"
#include "dvo_tsdf_mesh.h"

namespace dvo_tsdf {

constexpr int kImageBGR8 = 0, kImageRGB8 = 1, kImageMONO8 = 2;      /* == DVO_CAM_BGR8, DVO_CAM_RGB8, DVO_CAM_MONO8 */

DVO_TSDF_HD bool image_format_ok(int image_format) { return image_format == kImageBGR8 || image_format == kImageRGB8 || image_format == kImageMONO8; }
DVO_TSDF_HD size_t image_pixel_bytes(int image_format) { return image_format == kImageMONO8 ? 1 : 3; }

/* ---- the colour word ---- */
DVO_TSDF_HD unsigned colour_r(unsigned long long cw) { return (unsigned)(cw & 0xFFFFull); }
DVO_TSDF_HD unsigned colour_g(unsigned long long cw) { return (unsigned)((cw >> 16) & 0xFFFFull); }
DVO_TSDF_HD unsigned colour_b(unsigned long long cw) { return (unsigned)((cw >> 32) & 0xFFFFull); }
DVO_TSDF_HD unsigned colour_wc(unsigned long long cw) { return (unsigned)(cw >> 48); }
DVO_TSDF_HD unsigned long long make_colour(unsigned r, unsigned g, unsigned b, unsigned wc) {
    return (unsigned long long)r | ((unsigned long long)g << 16) | ((unsigned long long)b << 32) | ((unsigned long long)wc << 48);
}

/* ---- pixels ---- */
/* R, G, B of pixel px of an image */
DVO_TSDF_HD void image_rgb(const void *image, int image_format, size_t px, unsigned *rgb) {
    const unsigned char *p = static_cast<const unsigned char *>(image);
    if (image_format == kImageMONO8) { rgb[0] = rgb[1] = rgb[2] = p[px]; return; }
    const unsigned c0 = p[3 * px], c1 = p[3 * px + 1], c2 = p[3 * px + 2];
    rgb[1] = c1;
    if (image_format == kImageRGB8) { rgb[0] = c0; rgb[2] = c2; } else { rgb[0] = c2; rgb[2] = c0; }
}
/* levels R, G, B into pixel px of an image */
DVO_TSDF_HD void image_store(void *image, int image_format, size_t px, const int *rgb) {
    unsigned char *p = static_cast<unsigned char *>(image);
    if (image_format == kImageMONO8) {
        p[px] = (unsigned char)((1868u * (unsigned)rgb[2] + 9617u * (unsigned)rgb[1] + 4899u * (unsigned)rgb[0] + 8192u) >> 14);
        return;
    }
    p[3 * px + 1] = (unsigned char)rgb[1];
    if (image_format == kImageRGB8) { p[3 * px] = (unsigned char)rgb[0]; p[3 * px + 2] = (unsigned char)rgb[2]; }
    else { p[3 * px] = (unsigned char)rgb[2]; p[3 * px + 2] = (unsigned char)rgb[0]; }
}
/* the 8-bit level of a channel value in 1/256 levels */
DVO_TSDF_HD int colour_level(double c) {
    const int L = (int)floor(c / 256.0 + 0.5);
    return L < 0 ? 0 : L > 255 ? 255 : L;
}

/* ---- fusing ---- */
/* one channel's running mean after the observation C (0 .. 255) */
DVO_TSDF_HD unsigned colour_mean(unsigned c, unsigned wc, unsigned C) { return (c * wc + 256u * C + ((wc + 1u) >> 1)) / (wc + 1u); }
/* the colour word after the observation rgb */
DVO_TSDF_HD unsigned long long colour_blend(unsigned long long cw, const unsigned *rgb, int max_weight) {
    const unsigned wc = colour_wc(cw);
    return make_colour(colour_mean(colour_r(cw), wc, rgb[0]), colour_mean(colour_g(cw), wc, rgb[1]), colour_mean(colour_b(cw), wc, rgb[2]),
                       wc + 1u < (unsigned)max_weight ? wc + 1u : (unsigned)max_weight);
}
/* update() with colour: the word of the voxel whose centre is (wx, wy, wz) after frame f, and its colour word *cw after the frame's
 * image; a skipped voxel keeps both */
DVO_TSDF_HD unsigned update_colour(unsigned word, unsigned long long *cw, double wx, double wy, double wz, const VolumeConst &vc, const Frame &f,
                                   const void *image, int image_format, const FrameConst &fc) {
    size_t px;
    double sdf;
    if (!project(wx, wy, wz, vc, f, fc, &px, &sdf)) return word;
    if (sdf <= vc.trunc) {
        unsigned rgb[3];
        image_rgb(image, image_format, px, rgb);
        *cw = colour_blend(*cw, rgb, fc.max_weight);
    }
    return blend(word, sdf, vc, fc);
}

/* ---- a ray-cast pixel ---- */
/* the colour at voxel coordinates g; false: out of bounds or a corner without colour */
DVO_TSDF_HD bool colour_sample(const unsigned long long *colours, const RayVolume &rv, double gx, double gy, double gz, int *rgb) {
    const double ix = floor(gx), iy = floor(gy), iz = floor(gz);
    if (!(ix >= 0.0 && ix + 1.0 <= (double)(rv.nx - 1) && iy >= 0.0 && iy + 1.0 <= (double)(rv.ny - 1) && iz >= 0.0 &&
          iz + 1.0 <= (double)(rv.nz - 1)))
        return false;                                                                                  /* NaN falls out here */
    const double fx = gx - ix, fy = gy - iy, fz = gz - iz;
    const size_t sy = (size_t)rv.nx, sz = (size_t)rv.nx * (size_t)rv.ny;
    const unsigned long long *w = colours + ((size_t)(int)ix + sy * ((size_t)(int)iy + (size_t)rv.ny * (size_t)(int)iz));
    const unsigned long long c[8] = {w[0], w[1], w[sy], w[sy + 1], w[sz], w[sz + 1], w[sz + sy], w[sz + sy + 1]};
    for (int k = 0; k < 8; k++)
        if (colour_wc(c[k]) < 1u) return false;
    for (int ch = 0; ch < 3; ch++) {
        double q[8];
        for (int k = 0; k < 8; k++) q[k] = (double)(unsigned)((c[k] >> (16 * ch)) & 0xFFFFull);
        const double c00 = q[0] + fx * (q[1] - q[0]), c10 = q[2] + fx * (q[3] - q[2]), c01 = q[4] + fx * (q[5] - q[4]), c11 = q[6] + fx * (q[7] - q[6]);
        const double c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
        rgb[ch] = colour_level(c0 + fz * (c1 - c0));
    }
    return true;
}
/* pixel (u, v) of one view with colour: pixel() of dvo_tsdf_raycast.h, then the pixel's colour into image_out */
DVO_TSDF_HD void pixel_colour(const unsigned *words, const unsigned long long *colours, const RayVolume &rv, const RayCamera &c, const RayConst &rc,
                              int u, int v, bool clipped, void *depth_out, float *normals_out, void *image_out, int image_format) {
    double ray2[2], Zs;
    const bool hit = pixel_hit(words, rv, c, rc, u, v, clipped, depth_out, normals_out, ray2, &Zs);
    int rgb[3] = {0, 0, 0};
    if (hit) {
        double g[3];
        ray_point(rv, c, ray2[0], ray2[1], Zs, g);
        if (!colour_sample(colours, rv, g[0], g[1], g[2], rgb)) rgb[0] = rgb[1] = rgb[2] = 0;
    }
    image_store(image_out, image_format, (size_t)v * (size_t)rc.cols + (size_t)u, rgb);
}

/* ---- a mesh vertex ---- */
/* R, G, B of the vertex on the edge between a (word wa, colour ca) and b (wb, cb); the edge carries a vertex */
DVO_TSDF_HD void mesh_vertex_colour(unsigned wa, unsigned wb, unsigned long long ca, unsigned long long cb, unsigned char *rgb) {
    const bool has_a = colour_wc(ca) >= 1u, has_b = colour_wc(cb) >= 1u;
    if (!has_a && !has_b) { rgb[0] = rgb[1] = rgb[2] = 0; return; }
    const int qa = word_q(wa), qb = word_q(wb);
    const double lambda = (double)qa / (double)(qa - qb);
    for (int ch = 0; ch < 3; ch++) {
        const double va = (double)(unsigned)((ca >> (16 * ch)) & 0xFFFFull), vb = (double)(unsigned)((cb >> (16 * ch)) & 0xFFFFull);
        rgb[ch] = (unsigned char)colour_level(has_a && has_b ? va + lambda * (vb - va) : has_a ? va : vb);
    }
}

/* ---- the entry points ---- */

/* integrate() of dvo_tsdf_map.h with an image per frame: image[i] rows x cols of image_format.  False: refused, nothing written */
inline bool integrate_colour(const dvo_tsdf_volume *vol, unsigned *voxels, unsigned long long *colours, const dvo_tsdf_params *p, int count,
                             const void *const *depth, int depth_format, const void *const *image, int image_format, int rows, int cols,
                             const double *K4, const double *poses12) {
    if (!volume_ok(vol) || !voxels || !colours || !params_ok(p) || count < 1 || !depth || !format_ok(depth_format) || !image ||
        !image_format_ok(image_format) || rows < 1 || cols < 1 || !K4 || !poses12)
        return false;
    for (int i = 0; i < count; i++)
        if (!depth[i] || !image[i] || !frame_ok(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i)) return false;
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
                for (int x = 0; x < vc.nx; x++, a++)
                    voxels[a] = update_colour(voxels[a], colours + a, centre(vc.origin[0], vc.voxel_size, x), wy, wz, vc, f, image[i], image_format, fc);
            }
        }
    }
    return true;
}

/* raycast() of dvo_tsdf_raycast.h with an image per view: image_out[i] rows x cols of image_format.  False: refused, nothing written */
inline bool raycast_colour(const dvo_tsdf_volume *vol, const unsigned *voxels, const unsigned long long *colours, const dvo_raycast_params *p,
                           int count, int depth_format, int rows, int cols, const double *K4, const double *poses12, void *const *depth_out,
                           float *const *normals_out, void *const *image_out, int image_format, bool clipped = false) {
    if (!volume_ok(vol) || !voxels || !colours || !raycast_params_ok(p) || count < 1 || !format_ok(depth_format) || rows < 1 || cols < 1 || !K4 ||
        !poses12 || !depth_out || !image_out || !image_format_ok(image_format))
        return false;
    if (march_samples(*p, vol->trunc) < 0) return false;
    for (int i = 0; i < count; i++)
        if (!depth_out[i] || (normals_out && !normals_out[i]) || !image_out[i] || !frame_ok(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i)) return false;
    const RayVolume rv = ray_volume(*vol);
    RayConst rc;
    rc.depth_format = depth_format; rc.rows = rows; rc.cols = cols; rc.min_weight = p->min_weight; rc.z_near = p->z_near; rc.z_far = p->z_far;
    for (int i = 0; i < count; i++) {
        const RayCamera c = ray_camera(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i, p->step_trunc * vol->trunc);
        for (int v = 0; v < rows; v++)
            for (int u = 0; u < cols; u++)
                pixel_colour(voxels, colours, rv, c, rc, u, v, clipped, depth_out[i], normals_out ? normals_out[i] : nullptr, image_out[i], image_format);
    }
    return true;
}

/* mesh() of dvo_tsdf_mesh.h with three bytes R, G, B per vertex: the first vertex_capacity vertices' go to rgb (may be NULL with
 * capacity 0).  False: refused as mesh() refuses */
inline bool mesh_colour(const dvo_tsdf_volume *vol, const unsigned *voxels, const unsigned long long *colours, int min_weight, float *xyz,
                        unsigned char *rgb, long long vertex_capacity, int *tri, long long triangle_capacity, long long *n_vertices,
                        long long *n_triangles) {
    if (!colours || (vertex_capacity > 0 && !rgb)) return false;
    return mesh_walk(vol, voxels, min_weight, xyz, vertex_capacity, tri, triangle_capacity, n_vertices, n_triangles,
                     [&](long long o, size_t a, size_t b, int) { mesh_vertex_colour(voxels[a], voxels[b], colours[a], colours[b], rgb + 3 * o); });
}

}  // namespace dvo_tsdf
#endif
