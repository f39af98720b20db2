/*
 * dvo_capi_tsdf.cpp -- depth fusion (include/dvo_amd.h, "depth fusion"): the host definition's entry points (dvo_tsdf_map.h is the
 * definition), the stand-alone batch handle, its one-launch integration and its three-launch extraction (dvo_tsdf_map.hip), and the
 * ray cast of volumes into depth and normal maps (dvo_tsdf_raycast.h is its definition, dvo_tsdf_raycast.hip its one launch) and the
 * triangle mesh of a volume (dvo_tsdf_mesh.h is its definition, dvo_tsdf_mesh.hip its four launches), and the colour variants of all
 * three (dvo_tsdf_colour.h is their definition; the same launches with a colour kernel in them), and the Euclidean distance fields of
 * volumes (dvo_esdf.h is their definition, dvo_esdf.hip their kernels, dvo_esdf_launch.h the shape of their launches).  The handle
 * touches no dvo_ctx and no tracker.  Host side only; no CPU compute path behind the handle's entry points.
 */
#include "../../include/dvo_amd.h"
#include "dvo_handle.h"
#include "dvo_launch.h"
#include "dvo_tsdf_launch.h"
#include "dvo_esdf_launch.h"

#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace dvo_host;
using namespace dvo_tsdf;

/* The pool holds the set volumes back to back in the order they were set.  A volume set again keeps its place when its voxel count is
 * the same; the volume placed last may also change its count.  Nothing is in flight between two calls: every call that touches the
 * device ends in a synchronisation of the handle's stream. */
struct dvo_tsdf_batch : Handle {
    int max_volumes = 0;
    long long max_voxels = 0, used = 0;
    int last_placed = -1;
    struct Vol {
        bool set = false;
        dvo_tsdf_volume v = {};
        long long off = 0, n = 0;
        bool esdf_current = false;                 /* the volume's distance field is that of its words: set by dvo_esdf_update alone */
    };
    std::vector<Vol> vol;
    DevBuf<unsigned> pool;
    DevBuf<unsigned long long> colours;            /* the colour pool, laid out like `pool`; empty until dvo_colour_enable */
    Staging upload, out;                           /* descriptors + staged images of a call; count + points of an extraction: grow on demand */
    DevBuf<unsigned long long> d_counts;
    DevBuf<unsigned char> d_mesh;                  /* the per-voxel scratch of a mesh call (dvo_tsdf_launch.h: MeshScratch): grows on demand */
    DevBuf<unsigned> esdf;                         /* the distance-field pool, laid out like `pool`; empty until dvo_esdf_enable */
    DevBuf<unsigned> esdf_scratch;                 /* where an update's pass y writes and its pass z reads: grows on demand */
};

namespace {
thread_local std::string g_tsdf_create_error;      /* of the calling thread's last failed creation */

int tfail(dvo_tsdf_batch *b, int code, const std::string &msg) {
    (b ? b->err : g_tsdf_create_error) = msg;
    return code;
}
#define THIP(b, expr) DVO_HIP_CHECK(tfail, b, expr, #expr)

size_t pad16(size_t b) { return (b + 15) / 16 * 16; }

/* volume index -> its record; DVO_OK, or the code with the handle's message set */
int volume_of(dvo_tsdf_batch *b, int volume, dvo_tsdf_batch::Vol **out) {
    if (volume < 0 || volume >= b->max_volumes) return tfail(b, DVO_ERR_INVALID, "volume outside [0, max_volumes)");
    if (!b->vol[(size_t)volume].set) return tfail(b, DVO_ERR_STATE, "volume " + std::to_string(volume) + " was never set (dvo_tsdf_set_volume)");
    *out = &b->vol[(size_t)volume];
    return DVO_OK;
}

/* What dvo_tsdf_integrate (what = "frame") and dvo_raycast_views ("view") and their colour variants refuse in their lists: `images` is
 * the call's list of depth images and, in a `colour` call, `colour_images` its second list, of colour images of image_format;
 * image_ok(i) says that entry i has what it needs and `no_image` what to say if not.  DVO_OK, or the code with the
 * handle's message set */
template <class ImageOk>
int listed_ok(dvo_tsdf_batch *b, const char *what, int count, const int *volumes, const void *images, bool colour, const void *colour_images,
              int image_format, ImageOk image_ok, const char *no_image, int depth_format, int rows, int cols, const double *K4, const double *poses12, int flags) {
    if (count < 1 || !volumes || !images || (colour && !colour_images) || !K4 || !poses12) return tfail(b, DVO_ERR_INVALID, "count < 1 or a NULL argument");
    if (rows < 1 || cols < 1 || !format_ok(depth_format)) return tfail(b, DVO_ERR_INVALID, "rows or cols < 1, or an unknown depth format");
    if (colour && !image_format_ok(image_format)) return tfail(b, DVO_ERR_INVALID, "an unknown image format (DVO_CAM_BGR8, DVO_CAM_RGB8 or DVO_CAM_MONO8)");
    if (flags != 0 && flags != DVO_UPLOAD_DEVICE) return tfail(b, DVO_ERR_INVALID, "unknown flags (0 or DVO_UPLOAD_DEVICE)");
    for (int i = 0; i < count; i++) {
        if (volumes[i] < 0 || volumes[i] >= b->max_volumes) return tfail(b, DVO_ERR_INVALID, "a listed volume is outside [0, max_volumes)");
        if (!image_ok(i)) return tfail(b, DVO_ERR_INVALID, no_image);
        if (!frame_ok(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i))
            return tfail(b, DVO_ERR_INVALID, std::string(what) + " " + std::to_string(i) + ": a K4 or pose that is not finite, or fx / fy not positive");
    }
    dvo_tsdf_batch::Vol *V = nullptr;
    for (int i = 0; i < count; i++)
        if (const int rc = volume_of(b, volumes[i], &V)) return rc;
    return DVO_OK;
}

/* the first min(total, capacity) entries of 12 bytes of a result go to the caller */
void copy_entries(void *dst, const unsigned char *src, unsigned long long total, long long capacity, size_t entry_bytes = 12) {
    const long long keep = (long long)total < capacity ? (long long)total : capacity;
    if (keep > 0) std::memcpy(dst, src, entry_bytes * (size_t)keep);
}

/* every colour call on a handle without a colour pool */
int colour_enabled(dvo_tsdf_batch *b) {
    return b->colours.size() ? DVO_OK : tfail(b, DVO_ERR_STATE, "the handle has no colour pool (dvo_colour_enable)");
}

/* the zero fill of a volume's words, and of its colour words where the handle has them */
int zero_volume(dvo_tsdf_batch *b, long long off, long long n) {
    THIP(b, hipMemsetAsync(b->pool + off, 0, 4 * (size_t)n, b->stream));
    if (b->colours.size()) THIP(b, hipMemsetAsync(b->colours + off, 0, 8 * (size_t)n, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    return DVO_OK;
}

/* dvo_tsdf_integrate and, with `colour`, dvo_colour_integrate */
int integrate_on_device(dvo_tsdf_batch *b, const dvo_tsdf_params *p, int count, const int *volumes, const void *const *depth, int depth_format,
                        bool colour, const void *const *image, int image_format, int rows, int cols, const double *K4, const double *poses12,
                        int flags) {
    /* refusals first: a refused call changes nothing */
    if (!params_ok(p)) return tfail(b, DVO_ERR_INVALID, "bad parameters (NULL, 0 < z_near < z_far, both finite, max_weight in [1, 65535])");
    if (const int rc = listed_ok(b, "frame", count, volumes, depth, colour, image, image_format,
                                 [&](int i) { return depth[i] != nullptr && (!colour || image[i] != nullptr); },
                                 colour ? "a NULL depth image or a NULL image" : "a NULL depth image", depth_format, rows, cols, K4, poses12, flags))
        return rc;
    /* the frames grouped per volume, list order kept inside a volume; the volumes in the order they first appear */
    std::vector<int> slot((size_t)b->max_volumes, -1), listed, frames_of;
    for (int i = 0; i < count; i++)
        if (slot[(size_t)volumes[i]] < 0) { slot[(size_t)volumes[i]] = (int)listed.size(); listed.push_back(volumes[i]); }
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    const size_t pixels = (size_t)rows * (size_t)cols, depth_raw = pixels * depth_pixel_bytes(depth_format);
    const size_t colour_raw = colour ? pixels * image_pixel_bytes(image_format) : 0;
    const size_t nv = listed.size(), image_bytes = pad16(depth_raw), colour_bytes = pad16(colour_raw);
    /* the upload: volume records, frame records, [the frames' image pointers], [depth images, then colour images] */
    const size_t frames_at = pad16(sizeof(DeviceVolume) * nv), pointers_at = frames_at + pad16(sizeof(Frame) * (size_t)count);
    const size_t images_at = pointers_at + (colour ? pad16(sizeof(void *) * (size_t)count) : 0);
    const size_t colours_at = images_at + (staged ? image_bytes * (size_t)count : 0);
    const size_t up_total = colours_at + (staged ? colour_bytes * (size_t)count : 0);
    OnDevice guard(b->device);
    THIP(b, b->upload.reserve(up_total));
    DeviceVolume *dv = reinterpret_cast<DeviceVolume *>(b->upload.host.get());
    Frame *fr = reinterpret_cast<Frame *>(b->upload.host.get() + frames_at);
    const void **im = reinterpret_cast<const void **>(b->upload.host.get() + pointers_at);
    long long blocks = 0;
    int at = 0;
    for (size_t s = 0; s < nv; s++) {
        const dvo_tsdf_batch::Vol &V = b->vol[(size_t)listed[s]];
        DeviceVolume &D = dv[s];
        std::memset(&D, 0, sizeof(D));
        D.off = V.off; D.n = V.n; D.vc = volume_const(V.v);
        D.frame_first = at;
        for (int i = 0; i < count; i++) {
            if (volumes[i] != listed[s]) continue;
            Frame &f = fr[at];
            std::memcpy(f.R, poses12 + 12 * (size_t)i, 72);
            std::memcpy(f.t, poses12 + 12 * (size_t)i + 9, 24);
            std::memcpy(f.K, K4 + 4 * (size_t)i, 32);
            f.pad_ = 0;
            if (!staged) {
                f.depth = depth[i];
                if (colour) im[at] = image[i];
            } else {
                const size_t o = images_at + image_bytes * (size_t)at;
                std::memcpy(b->upload.host + o, depth[i], depth_raw);
                f.depth = b->upload.dev + o;
                if (colour) {
                    const size_t oc = colours_at + colour_bytes * (size_t)at;
                    std::memcpy(b->upload.host + oc, image[i], colour_raw);
                    im[at] = b->upload.dev + oc;
                }
            }
            at++;
        }
        D.frame_count = at - D.frame_first;
        D.block_first = (unsigned)blocks;
        D.nblocks = integrate_blocks(V.off, V.n);
        blocks += D.nblocks;
    }
    if (blocks > 0x7FFFFFFFll) return tfail(b, DVO_ERR_STATE, "internal: more workgroups than one launch holds");
    for (size_t s = 0; s < nv; s++) b->vol[(size_t)listed[s]].esdf_current = false;      /* host state only: the words are about to change */
    FrameConst fc;
    fc.depth_format = depth_format; fc.rows = rows; fc.cols = cols; fc.max_weight = p->max_weight; fc.z_near = p->z_near; fc.z_far = p->z_far;
    const DeviceVolume *d_vols = reinterpret_cast<const DeviceVolume *>(b->upload.dev.get());
    const Frame *d_frames = reinterpret_cast<const Frame *>(b->upload.dev.get() + frames_at);
    CallStats stats(*b, dvo::g_kernel_launches);
    THIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up_total, hipMemcpyHostToDevice, b->stream));
    if (colour)
        THIP(b, (hipError_t)launch_tsdf_integrate_colour(b->pool, b->colours, d_vols, (int)nv, d_frames,
                                                         reinterpret_cast<const void *const *>(b->upload.dev.get() + pointers_at), image_format, fc,
                                                         (unsigned)blocks, b->stream));
    else
        THIP(b, (hipError_t)launch_tsdf_integrate(b->pool, d_vols, (int)nv, d_frames, fc, (unsigned)blocks, b->stream));
    stats.launched();
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    return DVO_OK;
}

/* dvo_raycast_views and, with `colour`, dvo_colour_raycast_views */
int raycast_on_device(dvo_tsdf_batch *b, const dvo_raycast_params *p, int count, const int *volumes, int depth_format, int rows, int cols,
                      const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out, bool colour, void *const *image_out,
                      int image_format, int flags) {
    /* refusals first: a refused call writes nothing */
    if (!raycast_params_ok(p))
        return tfail(b, DVO_ERR_INVALID, "bad parameters (NULL, 0 < z_near < z_far, step_trunc in (0, 1], all finite, min_weight in [1, 65535])");
    if (const int rc = listed_ok(b, "view", count, volumes, depth_out, colour, image_out, image_format,
                                 [&](int i) { return depth_out[i] && (!normals_out || normals_out[i]) && (!colour || image_out[i]); },
                                 "a NULL output image", depth_format, rows, cols, K4, poses12, flags))
        return rc;
    for (int i = 0; i < count; i++)
        if (march_samples(*p, b->vol[(size_t)volumes[i]].v.trunc) < 0)
            return tfail(b, DVO_ERR_INVALID, "view " + std::to_string(i) + ": its march would have more than DVO_RAYCAST_MAX_STEPS samples");
    const size_t pixels = (size_t)rows * (size_t)cols, depth_bytes = pad16(pixels * depth_pixel_bytes(depth_format));
    const size_t normal_bytes = normals_out ? pad16(12 * pixels) : 0;
    const size_t colour_raw = colour ? pixels * image_pixel_bytes(image_format) : 0, colour_bytes = pad16(colour_raw);
    const size_t up_total = pad16(sizeof(DeviceView) * (size_t)count);
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    /* the results: depth images, then normals, then colour images */
    const size_t colours_at = (depth_bytes + normal_bytes) * (size_t)count;
    const size_t out_total = staged ? colours_at + colour_bytes * (size_t)count : 0;
    if ((unsigned long long)raycast_tiles(rows, cols) * (unsigned long long)count > 0x7FFFFFFFull)
        return tfail(b, DVO_ERR_INVALID, "more pixel tiles than one launch holds");
    OnDevice guard(b->device);
    THIP(b, b->upload.reserve(up_total));
    THIP(b, b->out.reserve(out_total));
    DeviceView *dv = reinterpret_cast<DeviceView *>(b->upload.host.get());
    for (int i = 0; i < count; i++) {
        const dvo_tsdf_batch::Vol &V = b->vol[(size_t)volumes[i]];
        DeviceView &D = dv[i];
        std::memset(&D, 0, sizeof(D));
        D.cam = ray_camera(K4 + 4 * (size_t)i, poses12 + 12 * (size_t)i, p->step_trunc * V.v.trunc);
        D.rv = ray_volume(V.v);
        D.off = V.off;
        if (staged) {
            D.depth = b->out.dev + depth_bytes * (size_t)i;
            D.normals = normals_out ? reinterpret_cast<float *>(b->out.dev + depth_bytes * (size_t)count + normal_bytes * (size_t)i) : nullptr;
            D.image = colour ? b->out.dev + colours_at + colour_bytes * (size_t)i : nullptr;
        } else {
            D.depth = depth_out[i];
            D.normals = normals_out ? normals_out[i] : nullptr;
            D.image = colour ? image_out[i] : nullptr;
        }
    }
    RayConst rc;
    rc.depth_format = depth_format; rc.rows = rows; rc.cols = cols; rc.min_weight = p->min_weight; rc.z_near = p->z_near; rc.z_far = p->z_far;
    CallStats stats(*b, dvo::g_kernel_launches);
    THIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up_total, hipMemcpyHostToDevice, b->stream));
    if (colour)
        THIP(b, (hipError_t)launch_tsdf_raycast_colour(b->pool, b->colours, reinterpret_cast<const DeviceView *>(b->upload.dev.get()), count, rc,
                                                       image_format, b->stream));
    else
        THIP(b, (hipError_t)launch_tsdf_raycast(b->pool, reinterpret_cast<const DeviceView *>(b->upload.dev.get()), count, rc, b->stream));
    stats.launched();
    if (staged) THIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    if (staged)
        for (int i = 0; i < count; i++) {
            std::memcpy(depth_out[i], b->out.host + depth_bytes * (size_t)i, pixels * depth_pixel_bytes(depth_format));
            if (normals_out) std::memcpy(normals_out[i], b->out.host + depth_bytes * (size_t)count + normal_bytes * (size_t)i, 12 * pixels);
            if (colour) std::memcpy(image_out[i], b->out.host + colours_at + colour_bytes * (size_t)i, colour_raw);
        }
    return DVO_OK;
}

/* dvo_mesh_extract and, with `colour`, dvo_colour_mesh_extract */
int mesh_on_device(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, bool colour, unsigned char *rgb, long long vertex_capacity, int *tri,
                   long long triangle_capacity, long long *n_vertices, long long *n_triangles, int flags) {
    /* refusals first: a refused call writes nothing */
    if (min_weight < 1 || vertex_capacity < 0 || (vertex_capacity > 0 && (!xyz || (colour && !rgb))) || triangle_capacity < 0 || (triangle_capacity > 0 && !tri) ||
        !n_vertices || !n_triangles)
        return tfail(b, DVO_ERR_INVALID, "min_weight < 1, a negative capacity, a NULL buffer with capacity > 0, or a NULL count");
    if (flags != 0 && flags != DVO_UPLOAD_DEVICE) return tfail(b, DVO_ERR_INVALID, "unknown flags (0 or DVO_UPLOAD_DEVICE)");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    /* a volume has at most seven vertices and twelve triangles per voxel: the device never needs room for more */
    const long long vcap = vertex_capacity < kMeshEdges * V->n ? vertex_capacity : kMeshEdges * V->n;
    const long long tcap = triangle_capacity < kMeshCellTriangles * V->n ? triangle_capacity : kMeshCellTriangles * V->n;
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    /* the results: 16 bytes of counts, xyz, [rgb], tri */
    const size_t rgb_at = 16 + pad16(12 * (size_t)vcap), tri_at = rgb_at + (colour ? pad16(3 * (size_t)vcap) : 0);
    const size_t out_total = staged ? tri_at + 12 * (size_t)tcap : 16;
    const size_t n_counts = 2 * ((size_t)extract_blocks(V->n) + 1), scratch_bytes = mesh_scratch_bytes(V->n);
    OnDevice guard(b->device);
    /* every block grows before anything is enqueued */
    if (n_counts > b->d_counts.size()) THIP(b, b->d_counts.alloc(n_counts));
    if (scratch_bytes > b->d_mesh.size()) THIP(b, b->d_mesh.alloc(scratch_bytes));
    THIP(b, b->out.reserve(out_total));
    float *d_xyz = staged ? reinterpret_cast<float *>(b->out.dev + 16) : xyz;
    int *d_tri = staged ? reinterpret_cast<int *>(b->out.dev + tri_at) : tri;
    unsigned char *d_rgb = staged ? b->out.dev + rgb_at : rgb;
    CallStats stats(*b, dvo::g_kernel_launches);
    if (colour)
        THIP(b, (hipError_t)launch_tsdf_mesh_colour(b->pool + V->off, b->colours + V->off, volume_const(V->v), min_weight, b->d_counts,
                                                    mesh_scratch_at(b->d_mesh, V->n), reinterpret_cast<unsigned long long *>(b->out.dev.get()),
                                                    vcap > 0 ? d_xyz : nullptr, vcap > 0 ? d_rgb : nullptr, vcap, tcap > 0 ? d_tri : nullptr, tcap,
                                                    b->stream));
    else
        THIP(b, (hipError_t)launch_tsdf_mesh(b->pool + V->off, volume_const(V->v), min_weight, b->d_counts, mesh_scratch_at(b->d_mesh, V->n),
                                             reinterpret_cast<unsigned long long *>(b->out.dev.get()), vcap > 0 ? d_xyz : nullptr, vcap,
                                             tcap > 0 ? d_tri : nullptr, tcap, b->stream));
    stats.launched();
    THIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    unsigned long long totals[2] = {0, 0};
    std::memcpy(totals, b->out.host.get(), 16);
    *n_vertices = (long long)totals[0];
    *n_triangles = (long long)totals[1];
    if ((long long)totals[0] > kMeshMaxVertices) return tfail(b, DVO_ERR_INVALID, "the mesh has more than 2^31 - 1 vertices: its indices are 32-bit");
    if (staged) {
        copy_entries(xyz, b->out.host + 16, totals[0], vcap);
        if (colour) copy_entries(rgb, b->out.host + rgb_at, totals[0], vcap, 3);
        copy_entries(tri, b->out.host + tri_at, totals[1], tcap);
    }
    return DVO_OK;
}
/* every reader of a distance field: the handle has its pool and the volume's field is that of its words */
int esdf_current(dvo_tsdf_batch *b, int volume, dvo_tsdf_batch::Vol **out) {
    if (!b->esdf.size()) return tfail(b, DVO_ERR_STATE, "the handle has no distance-field pool (dvo_esdf_enable)");
    if (const int rc = volume_of(b, volume, out)) return rc;
    if (!(*out)->esdf_current)
        return tfail(b, DVO_ERR_STATE, "the distance field of volume " + std::to_string(volume) + " is not current (dvo_esdf_update)");
    return DVO_OK;
}
}  // namespace

extern "C" {

int dvo_tsdf_params_default(dvo_tsdf_params *p) {
    if (!p) return DVO_ERR_INVALID;
    params_default(p);
    return DVO_OK;
}

int dvo_tsdf_integrate_host(const dvo_tsdf_volume *vol, unsigned *voxels, const dvo_tsdf_params *p, int count, const void *const *depth,
                            int depth_format, int rows, int cols, const double *K4, const double *poses12) {
    return integrate(vol, voxels, p, count, depth, depth_format, rows, cols, K4, poses12) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_tsdf_extract_host(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long capacity, long long *n_points) {
    return extract(vol, voxels, min_weight, xyz, capacity, n_points) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_tsdf_create(int max_volumes, long long max_voxels_total, dvo_tsdf_batch **out) {
    if (!out) return tfail(nullptr, DVO_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (max_volumes < 1 || max_voxels_total < 1 || (long long)max_volumes > max_voxels_total)
        return tfail(nullptr, DVO_ERR_INVALID, "bad capacities (max_volumes >= 1, max_voxels_total >= max_volumes)");
    std::string why;
    if (const int rc = device_check(&why)) return tfail(nullptr, rc, why);
    /* a volume is at most 2^30 words; the launch counts its workgroups in 31 bits */
    if (max_voxels_total > ((long long)1 << 38)) return tfail(nullptr, DVO_ERR_NOMEM, "a pool above 2^38 voxels is not supported");
    dvo_tsdf_batch *b = new dvo_tsdf_batch();
    b->max_volumes = max_volumes; b->max_voxels = max_voxels_total;
    b->vol.resize((size_t)max_volumes);
    hipError_t r = b->open();
    if (r == hipSuccess) r = b->pool.alloc((size_t)max_voxels_total);
    if (r != hipSuccess) {
        const std::string msg = std::string("depth-fusion pool: ") + hipGetErrorString(r);
        dvo_tsdf_destroy(b);
        return tfail(nullptr, hip_status(r), msg);
    }
    *out = b;
    return DVO_OK;
}

int dvo_tsdf_destroy(dvo_tsdf_batch *b) {
    if (!b) return DVO_ERR_INVALID;
    OnDevice guard(b->device);
    b->close();
    delete b;                                      /* the buffers go here, on the handle's device */
    return DVO_OK;
}

const char *dvo_tsdf_last_error(const dvo_tsdf_batch *b) { return b ? b->err.c_str() : g_tsdf_create_error.c_str(); }

int dvo_tsdf_set_volume(dvo_tsdf_batch *b, int volume, const dvo_tsdf_volume *vol) {
    if (!b) return DVO_ERR_INVALID;
    if (volume < 0 || volume >= b->max_volumes) return tfail(b, DVO_ERR_INVALID, "volume outside [0, max_volumes)");
    if (!volume_ok(vol))
        return tfail(b, DVO_ERR_INVALID, "bad volume (NULL, a dimension outside [1, DVO_TSDF_MAX_DIM], voxel_size or trunc not positive, a number "
                                         "that is not finite)");
    dvo_tsdf_batch::Vol &V = b->vol[(size_t)volume];
    const long long n = (long long)voxels_of(*vol);
    long long off = b->used, used_after = b->used + n;
    if (V.set && V.n == n) { off = V.off; used_after = b->used; }
    else if (V.set && volume == b->last_placed) { off = V.off; used_after = V.off + n; }
    else if (V.set) return tfail(b, DVO_ERR_INVALID, "a set volume keeps its voxel count unless it is the one placed last");
    if (used_after > b->max_voxels) return tfail(b, DVO_ERR_INVALID, "the set volumes would hold more voxels than the handle was created for");
    OnDevice guard(b->device);
    V.esdf_current = false;
    if (const int rc = zero_volume(b, off, n)) return rc;
    if (!V.set || V.n != n) b->last_placed = volume;
    V.set = true; V.v = *vol; V.off = off; V.n = n;
    b->used = used_after;
    return DVO_OK;
}

int dvo_tsdf_clear(dvo_tsdf_batch *b, int volume) {
    if (!b) return DVO_ERR_INVALID;
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    OnDevice guard(b->device);
    V->esdf_current = false;
    return zero_volume(b, V->off, V->n);
}

int dvo_tsdf_integrate(dvo_tsdf_batch *b, const dvo_tsdf_params *p, int count, const int *volumes, const void *const *depth, int depth_format,
                       int rows, int cols, const double *K4, const double *poses12, int flags) {
    if (!b) return DVO_ERR_INVALID;
    return integrate_on_device(b, p, count, volumes, depth, depth_format, false, nullptr, 0, rows, cols, K4, poses12, flags);
}

int dvo_colour_integrate_host(const dvo_tsdf_volume *vol, unsigned *voxels, unsigned long long *colours, const dvo_tsdf_params *p, int count,
                                   const void *const *depth, int depth_format, const void *const *image, int image_format, int rows, int cols,
                                   const double *K4, const double *poses12) {
    return integrate_colour(vol, voxels, colours, p, count, depth, depth_format, image, image_format, rows, cols, K4, poses12) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_colour_enable(dvo_tsdf_batch *b) {
    if (!b) return DVO_ERR_INVALID;
    if (b->colours.size()) return DVO_OK;
    OnDevice guard(b->device);
    DevBuf<unsigned long long> fresh;
    hipError_t r = fresh.alloc((size_t)b->max_voxels);
    if (r == hipSuccess) r = hipMemsetAsync(fresh, 0, 8 * (size_t)b->max_voxels, b->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(b->stream);
    if (r != hipSuccess) return tfail(b, hip_status(r), std::string("colour pool: ") + hipGetErrorString(r));
    b->colours = std::move(fresh);
    return DVO_OK;
}

int dvo_colour_integrate(dvo_tsdf_batch *b, const dvo_tsdf_params *p, int count, const int *volumes, const void *const *depth, int depth_format,
                              const void *const *image, int image_format, int rows, int cols, const double *K4, const double *poses12, int flags) {
    if (!b) return DVO_ERR_INVALID;
    if (const int rc = colour_enabled(b)) return rc;
    return integrate_on_device(b, p, count, volumes, depth, depth_format, true, image, image_format, rows, cols, K4, poses12, flags);
}

int dvo_colour_get_words(dvo_tsdf_batch *b, int volume, unsigned long long *out) {
    if (!b) return DVO_ERR_INVALID;
    if (const int rc = colour_enabled(b)) return rc;
    if (!out) return tfail(b, DVO_ERR_INVALID, "a NULL buffer");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    OnDevice guard(b->device);
    THIP(b, hipMemcpyAsync(out, b->colours + V->off, 8 * (size_t)V->n, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    return DVO_OK;
}

int dvo_colour_set_words(dvo_tsdf_batch *b, int volume, const unsigned long long *in) {
    if (!b) return DVO_ERR_INVALID;
    if (const int rc = colour_enabled(b)) return rc;
    if (!in) return tfail(b, DVO_ERR_INVALID, "a NULL buffer");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    OnDevice guard(b->device);
    THIP(b, hipMemcpyAsync(b->colours + V->off, in, 8 * (size_t)V->n, hipMemcpyHostToDevice, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    return DVO_OK;
}

int dvo_tsdf_extract_points(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, long long capacity, long long *n_points) {
    if (!b) return DVO_ERR_INVALID;
    if (min_weight < 1 || capacity < 0 || (capacity > 0 && !xyz) || !n_points)
        return tfail(b, DVO_ERR_INVALID, "min_weight < 1, a negative capacity, a NULL buffer with capacity > 0, or a NULL n_points");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    /* a volume has at most three points per voxel: the device never needs room for more */
    const long long cap = capacity < 3 * V->n ? capacity : 3 * V->n;
    const size_t out_total = 16 + 12 * (size_t)cap, n_counts = (size_t)extract_blocks(V->n) + 1;
    OnDevice guard(b->device);
    if (n_counts > b->d_counts.size()) THIP(b, b->d_counts.alloc(n_counts));
    THIP(b, b->out.reserve(out_total));
    CallStats stats(*b, dvo::g_kernel_launches);
    THIP(b, (hipError_t)launch_tsdf_extract(b->pool + V->off, volume_const(V->v), min_weight, b->d_counts, b->out.dev, cap, b->stream));
    stats.launched();
    THIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    unsigned long long total = 0;
    std::memcpy(&total, b->out.host.get(), 8);
    copy_entries(xyz, b->out.host + 16, total, cap);
    *n_points = (long long)total;
    return DVO_OK;
}

int dvo_tsdf_get_voxels(dvo_tsdf_batch *b, int volume, unsigned *out) {
    if (!b) return DVO_ERR_INVALID;
    if (!out) return tfail(b, DVO_ERR_INVALID, "a NULL buffer");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    OnDevice guard(b->device);
    THIP(b, hipMemcpyAsync(out, b->pool + V->off, 4 * (size_t)V->n, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    return DVO_OK;
}

int dvo_tsdf_set_voxels(dvo_tsdf_batch *b, int volume, const unsigned *in) {
    if (!b) return DVO_ERR_INVALID;
    if (!in) return tfail(b, DVO_ERR_INVALID, "a NULL buffer");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = volume_of(b, volume, &V)) return rc;
    OnDevice guard(b->device);
    V->esdf_current = false;
    THIP(b, hipMemcpyAsync(b->pool + V->off, in, 4 * (size_t)V->n, hipMemcpyHostToDevice, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    return DVO_OK;
}

int dvo_raycast_params_default(dvo_raycast_params *p) {
    if (!p) return DVO_ERR_INVALID;
    raycast_params_default(p);
    return DVO_OK;
}

int dvo_raycast_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const dvo_raycast_params *p, int count, int depth_format, int rows, int cols,
                     const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out) {
    return raycast(vol, voxels, p, count, depth_format, rows, cols, K4, poses12, depth_out, normals_out) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_raycast_views(dvo_tsdf_batch *b, const dvo_raycast_params *p, int count, const int *volumes, int depth_format, int rows, int cols,
                      const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out, int flags) {
    if (!b) return DVO_ERR_INVALID;
    return raycast_on_device(b, p, count, volumes, depth_format, rows, cols, K4, poses12, depth_out, normals_out, false, nullptr, 0, flags);
}

int dvo_colour_raycast_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const unsigned long long *colours, const dvo_raycast_params *p, int count,
                            int depth_format, int rows, int cols, const double *K4, const double *poses12, void *const *depth_out,
                            float *const *normals_out, void *const *image_out, int image_format) {
    return raycast_colour(vol, voxels, colours, p, count, depth_format, rows, cols, K4, poses12, depth_out, normals_out, image_out, image_format)
               ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_colour_raycast_views(dvo_tsdf_batch *b, const dvo_raycast_params *p, int count, const int *volumes, int depth_format, int rows, int cols,
                             const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out, void *const *image_out,
                             int image_format, int flags) {
    if (!b) return DVO_ERR_INVALID;
    if (const int rc = colour_enabled(b)) return rc;
    return raycast_on_device(b, p, count, volumes, depth_format, rows, cols, K4, poses12, depth_out, normals_out, true, image_out, image_format, flags);
}

int dvo_mesh_host(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long vertex_capacity, int *tri,
                  long long triangle_capacity, long long *n_vertices, long long *n_triangles) {
    try {
        return mesh(vol, voxels, min_weight, xyz, vertex_capacity, tri, triangle_capacity, n_vertices, n_triangles) ? DVO_OK : DVO_ERR_INVALID;
    } catch (const std::bad_alloc &) {
        return DVO_ERR_NOMEM;
    }
}

int dvo_colour_mesh_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const unsigned long long *colours, int min_weight, float *xyz,
                         unsigned char *rgb, long long vertex_capacity, int *tri, long long triangle_capacity, long long *n_vertices,
                         long long *n_triangles) {
    try {
        return mesh_colour(vol, voxels, colours, min_weight, xyz, rgb, vertex_capacity, tri, triangle_capacity, n_vertices, n_triangles) ? DVO_OK
                                                                                                                                         : DVO_ERR_INVALID;
    } catch (const std::bad_alloc &) {
        return DVO_ERR_NOMEM;
    }
}

int dvo_mesh_extract(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, long long vertex_capacity, int *tri, long long triangle_capacity,
                     long long *n_vertices, long long *n_triangles, int flags) {
    if (!b) return DVO_ERR_INVALID;
    return mesh_on_device(b, volume, min_weight, xyz, false, nullptr, vertex_capacity, tri, triangle_capacity, n_vertices, n_triangles, flags);
}

int dvo_colour_mesh_extract(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, unsigned char *rgb, long long vertex_capacity, int *tri,
                            long long triangle_capacity, long long *n_vertices, long long *n_triangles, int flags) {
    if (!b) return DVO_ERR_INVALID;
    if (const int rc = colour_enabled(b)) return rc;
    return mesh_on_device(b, volume, min_weight, xyz, true, rgb, vertex_capacity, tri, triangle_capacity, n_vertices, n_triangles, flags);
}

int dvo_esdf_params_default(dvo_esdf_params *p) {
    if (!p) return DVO_ERR_INVALID;
    esdf_params_default(p);
    return DVO_OK;
}

int dvo_esdf_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const dvo_esdf_params *p, unsigned *words_out) {
    try {
        return esdf(vol, voxels, p, words_out) ? DVO_OK : DVO_ERR_INVALID;
    } catch (const std::bad_alloc &) {
        return DVO_ERR_NOMEM;
    }
}

int dvo_esdf_distances_host(const dvo_tsdf_volume *vol, const unsigned *words, float *out) {
    return esdf_distances(vol, words, out) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_esdf_query_host(const dvo_tsdf_volume *vol, const unsigned *words, int count, const double *xyz, dvo_esdf_sample *records) {
    return esdf_query(vol, words, count, xyz, records) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_esdf_enable(dvo_tsdf_batch *b) {
    if (!b) return DVO_ERR_INVALID;
    if (b->esdf.size()) return DVO_OK;
    OnDevice guard(b->device);
    DevBuf<unsigned> fresh;
    hipError_t r = fresh.alloc((size_t)b->max_voxels);
    if (r == hipSuccess) r = hipMemsetAsync(fresh, 0, 4 * (size_t)b->max_voxels, b->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(b->stream);
    if (r != hipSuccess) return tfail(b, hip_status(r), std::string("distance-field pool: ") + hipGetErrorString(r));
    b->esdf = std::move(fresh);
    return DVO_OK;
}

int dvo_esdf_update(dvo_tsdf_batch *b, const dvo_esdf_params *p, int count, const int *volumes) {
    if (!b) return DVO_ERR_INVALID;
    /* refusals first: a refused call changes nothing */
    if (!b->esdf.size()) return tfail(b, DVO_ERR_STATE, "the handle has no distance-field pool (dvo_esdf_enable)");
    if (!esdf_params_ok(p)) return tfail(b, DVO_ERR_INVALID, "bad parameters (NULL, min_weight < 1 or an unknown sites)");
    if (count < 1 || count > b->max_volumes || !volumes) return tfail(b, DVO_ERR_INVALID, "count outside [1, max_volumes] or a NULL list");
    std::vector<char> seen((size_t)b->max_volumes, 0);
    for (int i = 0; i < count; i++) {
        if (volumes[i] < 0 || volumes[i] >= b->max_volumes) return tfail(b, DVO_ERR_INVALID, "a listed volume is outside [0, max_volumes)");
        if (seen[(size_t)volumes[i]]) return tfail(b, DVO_ERR_INVALID, "volume " + std::to_string(volumes[i]) + " is listed twice");
        seen[(size_t)volumes[i]] = 1;
    }
    dvo_tsdf_batch::Vol *V = nullptr;
    for (int i = 0; i < count; i++)
        if (const int rc = volume_of(b, volumes[i], &V)) return rc;
    /* the upload: one record per listed volume; the scratch holds the listed volumes back to back, since every launch covers them all */
    const size_t up_total = pad16(sizeof(EsdfVolume) * (size_t)count);
    long long blocks[3] = {0, 0, 0}, scratch = 0;
    OnDevice guard(b->device);
    THIP(b, b->upload.reserve(up_total));
    EsdfVolume *ev = reinterpret_cast<EsdfVolume *>(b->upload.host.get());
    for (int i = 0; i < count; i++) {
        const dvo_tsdf_batch::Vol &L = b->vol[(size_t)volumes[i]];
        EsdfVolume &E = ev[i];
        std::memset(&E, 0, sizeof(E));
        E.off = L.off; E.scratch_off = scratch;
        E.nx = L.v.nx; E.ny = L.v.ny; E.nz = L.v.nz;
        for (int k = 0; k < 3; k++) {
            E.first[k] = (unsigned)blocks[k];
            blocks[k] += esdf_blocks(k, E.nx, E.ny, E.nz);
            if (blocks[k] > 0x7FFFFFFFll) return tfail(b, DVO_ERR_INVALID, "more workgroups than one launch holds: list fewer volumes per call");
        }
        scratch += L.n;
    }
    if ((size_t)scratch > b->esdf_scratch.size()) THIP(b, b->esdf_scratch.alloc((size_t)scratch));
    const unsigned nb[3] = {(unsigned)blocks[0], (unsigned)blocks[1], (unsigned)blocks[2]};
    for (int i = 0; i < count; i++) b->vol[(size_t)volumes[i]].esdf_current = false;
    CallStats stats(*b, dvo::g_kernel_launches);
    THIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up_total, hipMemcpyHostToDevice, b->stream));
    THIP(b, (hipError_t)launch_esdf_update(b->pool, b->esdf, b->esdf_scratch, reinterpret_cast<const EsdfVolume *>(b->upload.dev.get()), count,
                                           p->min_weight, p->sites, nb, b->stream));
    stats.launched();
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    for (int i = 0; i < count; i++) b->vol[(size_t)volumes[i]].esdf_current = true;
    return DVO_OK;
}

int dvo_esdf_get_words(dvo_tsdf_batch *b, int volume, unsigned *out) {
    if (!b) return DVO_ERR_INVALID;
    if (!out) return tfail(b, DVO_ERR_INVALID, "a NULL buffer");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = esdf_current(b, volume, &V)) return rc;
    OnDevice guard(b->device);
    THIP(b, hipMemcpyAsync(out, b->esdf + V->off, 4 * (size_t)V->n, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    return DVO_OK;
}

int dvo_esdf_get_distances(dvo_tsdf_batch *b, int volume, int iz0, int nz, float *out, int flags) {
    if (!b) return DVO_ERR_INVALID;
    if (!out) return tfail(b, DVO_ERR_INVALID, "a NULL buffer");
    if (flags != 0 && flags != DVO_UPLOAD_DEVICE) return tfail(b, DVO_ERR_INVALID, "unknown flags (0 or DVO_UPLOAD_DEVICE)");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = esdf_current(b, volume, &V)) return rc;
    if (iz0 < 0 || nz < 1 || iz0 > V->v.nz - nz) return tfail(b, DVO_ERR_INVALID, "planes outside the volume (0 <= iz0, nz >= 1, iz0 + nz <= its nz)");
    const long long plane = (long long)V->v.nx * V->v.ny, count = plane * nz;
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    OnDevice guard(b->device);
    if (staged) THIP(b, b->out.reserve(4 * (size_t)count));
    float *d_out = staged ? reinterpret_cast<float *>(b->out.dev.get()) : out;
    CallStats stats(*b, dvo::g_kernel_launches);
    THIP(b, (hipError_t)launch_esdf_distances(b->esdf + V->off + plane * iz0, count, V->v.voxel_size, d_out, b->stream));
    stats.launched();
    if (staged) THIP(b, hipMemcpyAsync(b->out.host, b->out.dev, 4 * (size_t)count, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    if (staged) std::memcpy(out, b->out.host.get(), 4 * (size_t)count);
    return DVO_OK;
}

int dvo_esdf_query(dvo_tsdf_batch *b, int volume, int count, const double *xyz, dvo_esdf_sample *out, int flags) {
    if (!b) return DVO_ERR_INVALID;
    if (count < 1 || !xyz || !out) return tfail(b, DVO_ERR_INVALID, "count < 1 or a NULL argument");
    if (flags != 0 && flags != DVO_UPLOAD_DEVICE) return tfail(b, DVO_ERR_INVALID, "unknown flags (0 or DVO_UPLOAD_DEVICE)");
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    if (staged)
        for (size_t i = 0; i < 3 * (size_t)count; i++)
            if (!dvo_tsdf::finite(xyz[i])) return tfail(b, DVO_ERR_INVALID, "point " + std::to_string(i / 3) + " is not finite");
    dvo_tsdf_batch::Vol *V = nullptr;
    if (const int rc = esdf_current(b, volume, &V)) return rc;
    const size_t up_total = 24 * (size_t)count, out_total = sizeof(dvo_esdf_sample) * (size_t)count;
    OnDevice guard(b->device);
    if (staged) {
        THIP(b, b->upload.reserve(up_total));
        THIP(b, b->out.reserve(out_total));
        std::memcpy(b->upload.host.get(), xyz, up_total);
    }
    const double *d_xyz = staged ? reinterpret_cast<const double *>(b->upload.dev.get()) : xyz;
    dvo_esdf_sample *d_out = staged ? reinterpret_cast<dvo_esdf_sample *>(b->out.dev.get()) : out;
    CallStats stats(*b, dvo::g_kernel_launches);
    if (staged) THIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up_total, hipMemcpyHostToDevice, b->stream));
    THIP(b, (hipError_t)launch_esdf_query(b->esdf + V->off, volume_const(V->v), count, d_xyz, d_out, b->stream));
    stats.launched();
    if (staged) THIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    THIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    if (staged) std::memcpy(out, b->out.host.get(), out_total);
    return DVO_OK;
}

int dvo_tsdf_stats(dvo_tsdf_batch *b, int *last_launches, int *last_syncs) {
    return b ? b->stats(last_launches, last_syncs) : DVO_ERR_INVALID;
}

}  // extern "C"
