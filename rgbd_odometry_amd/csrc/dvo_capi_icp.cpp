/*
 * dvo_capi_icp.cpp -- frame-to-model alignment (include/dvo_amd.h, "frame-to-model alignment"): the host definition's entry point
 * (dvo_icp.h is the definition), the stand-alone batch handle and its two launches per sweep (dvo_icp.hip), and the front end of a depth
 * frame -- bilateral filter and now-frame normals (dvo_icp_prepare.h is the definition, dvo_icp_prepare.hip the kernels).  The handle touches no
 * dvo_ctx, no tracker and no dvo_tsdf_batch.  Host side only; no CPU compute path behind the handle's entry points.
 */
#include "../../include/dvo_amd.h"
#include "dvo_handle.h"
#include "dvo_launch.h"
#include "dvo_icp_launch.h"
#include "dvo_icp_prepare_launch.h"

#include <cstring>
#include <string>

using namespace dvo_host;
using namespace dvo_icp;

/* Nothing is in flight between two calls: every call that touches the device ends in a synchronisation of the handle's stream. */
struct dvo_icp_batch : Handle {
    int max_views = 0;
    Staging upload, out;                           /* the views (and the staged images) of a call; its poses and records: grow on demand */
    DevBuf<double> partials;                       /* kSlots rows per view, one entry per sweep workgroup: grows on demand */
};

namespace {
thread_local std::string g_icp_create_error;       /* of the calling thread's last failed creation */

int ifail(dvo_icp_batch *b, int code, const std::string &msg) {
    (b ? b->err : g_icp_create_error) = msg;
    return code;
}
#define IHIP(b, expr) DVO_HIP_CHECK(ifail, b, expr, #expr)

size_t pad16(size_t n) { return (n + 15) / 16 * 16; }
}  // namespace

extern "C" {

int dvo_icp_params_default(dvo_icp_params *p) {
    if (!p) return DVO_ERR_INVALID;
    params_default(p);
    return DVO_OK;
}

int dvo_icp_align_gated_host(const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                             const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                             const double *model_poses12, const double *start_poses12, const float *const *now_normals, double normal_cos_min,
                             double *poses12_out, dvo_icp_record *records) {
    return align_gated(p, count, now_format, model_format, rows, cols, K4, now_depth, model_depth, model_normals, model_poses12, start_poses12, now_normals,
                       normal_cos_min, poses12_out, records)
               ? DVO_OK
               : DVO_ERR_INVALID;
}

int dvo_icp_align_host(const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                       const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                       const double *model_poses12, const double *start_poses12, double *poses12_out, dvo_icp_record *records) {
    return dvo_icp_align_gated_host(p, count, now_format, model_format, rows, cols, K4, now_depth, model_depth, model_normals, model_poses12, start_poses12,
                                    nullptr, 0.0, poses12_out, records);
}

int dvo_icp_prepare_params_default(dvo_icp_prepare_params *fp) {
    if (!fp) return DVO_ERR_INVALID;
    prepare_params_default(fp);
    return DVO_OK;
}

int dvo_icp_prepare_params_gaussian(int radius, double sigma_s_px, double sigma_r_m, double edge_max, dvo_icp_prepare_params *fp) {
    return prepare_params_gaussian(radius, sigma_s_px, sigma_r_m, edge_max, fp) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_icp_prepare_host(const dvo_icp_prepare_params *fp, int count, int depth_format, int rows, int cols, const double *K4, const void *const *depth,
                         float *const *depth_out, float *const *normals_out) {
    return prepare(fp, count, depth_format, rows, cols, K4, depth, depth_out, normals_out) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_icp_create(int max_views, dvo_icp_batch **out) {
    if (!out) return ifail(nullptr, DVO_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (max_views < 1) return ifail(nullptr, DVO_ERR_INVALID, "max_views < 1");
    std::string why;
    if (const int rc = device_check(&why)) return ifail(nullptr, rc, why);
    dvo_icp_batch *b = new dvo_icp_batch();
    b->max_views = max_views;
    const hipError_t r = b->open();
    if (r != hipSuccess) {
        const std::string msg = std::string("alignment handle: ") + hipGetErrorString(r);
        dvo_icp_destroy(b);
        return ifail(nullptr, hip_status(r), msg);
    }
    *out = b;
    return DVO_OK;
}

int dvo_icp_destroy(dvo_icp_batch *b) {
    if (!b) return DVO_ERR_INVALID;
    OnDevice guard(b->device);
    b->close();
    delete b;                                      /* the buffers go here, on the handle's device */
    return DVO_OK;
}

const char *dvo_icp_last_error(const dvo_icp_batch *b) { return b ? b->err.c_str() : g_icp_create_error.c_str(); }

int dvo_icp_prepare(dvo_icp_batch *b, const dvo_icp_prepare_params *fp, int count, int depth_format, int rows, int cols, const double *K4,
                    const void *const *depth, float *const *depth_out, float *const *normals_out, int flags) {
    if (!b) return DVO_ERR_INVALID;
    dvo_icp_prepare_params P;
    if (fp) P = *fp; else prepare_params_default(&P);
    /* refusals first: a refused call writes nothing */
    if (!prepare_params_ok(&P))
        return ifail(b, DVO_ERR_INVALID, "bad parameters (radius in [0, DVO_ICP_PREPARE_MAX_RADIUS], reserved 0, range_scale and edge_max finite and > 0, "
                                         "range[0] and the centre's spatial weight >= 1)");
    if (count < 1 || !K4 || !depth || !depth_out) return ifail(b, DVO_ERR_INVALID, "count < 1 or a NULL argument");
    if (count > b->max_views) return ifail(b, DVO_ERR_INVALID, "count above max_views");
    if (!shape_ok(rows, cols) || !format_ok(depth_format))
        return ifail(b, DVO_ERR_INVALID, "rows or cols < 1, rows * cols > DVO_ICP_MAX_PIXELS, or an unknown depth format");
    if (flags != 0 && flags != DVO_UPLOAD_DEVICE) return ifail(b, DVO_ERR_INVALID, "unknown flags (0 or DVO_UPLOAD_DEVICE)");
    const double identity[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    for (int i = 0; i < count; i++) {
        if (!depth[i] || !depth_out[i] || (normals_out && !normals_out[i])) return ifail(b, DVO_ERR_INVALID, "a NULL image");
        if (!frame_ok(K4 + 4 * (size_t)i, identity))
            return ifail(b, DVO_ERR_INVALID, "image " + std::to_string(i) + ": a K4 that is not finite, or fx / fy not positive");
        if (!staged && static_cast<const void *>(depth_out[i]) == depth[i])
            return ifail(b, DVO_ERR_INVALID, "image " + std::to_string(i) + ": depth_out is its depth (the filter reads a halo: it cannot run in place)");
    }
    const size_t pixels = (size_t)rows * (size_t)cols;
    const size_t in_raw = pixels * dvo_tsdf::depth_pixel_bytes(depth_format), in_bytes = pad16(in_raw);
    const size_t f_raw = 4 * pixels, f_bytes = pad16(f_raw), n_raw = 12 * pixels, n_bytes = normals_out ? pad16(n_raw) : 0;
    /* the upload: the image records, [the images]; the outputs of a staged call: per image [filtered, normals] */
    const size_t images_at = pad16(sizeof(PrepareImage) * (size_t)count);
    const size_t up_total = images_at + (staged ? in_bytes * (size_t)count : 0);
    const size_t out_per = f_bytes + n_bytes, out_total = staged ? out_per * (size_t)count : 0;
    if ((unsigned long long)filter_tiles(rows, cols) * (unsigned long long)count > 0x7FFFFFFFull ||
        (unsigned long long)normals_blocks(rows, cols) * (unsigned long long)count > 0x7FFFFFFFull)
        return ifail(b, DVO_ERR_INVALID, "more workgroups than one launch holds");
    OnDevice guard(b->device);
    /* every block grows before anything is enqueued */
    IHIP(b, b->upload.reserve(up_total));
    if (staged) IHIP(b, b->out.reserve(out_total));
    PrepareImage *im = reinterpret_cast<PrepareImage *>(b->upload.host.get());
    for (int i = 0; i < count; i++) {
        std::memset(&im[i], 0, sizeof(PrepareImage));
        if (staged) {
            std::memcpy(b->upload.host + images_at + in_bytes * (size_t)i, depth[i], in_raw);
            im[i].depth = b->upload.dev + images_at + in_bytes * (size_t)i;
            im[i].depth_out = reinterpret_cast<float *>(b->out.dev + out_per * (size_t)i);
            im[i].normals_out = normals_out ? reinterpret_cast<float *>(b->out.dev + out_per * (size_t)i + f_bytes) : nullptr;
        } else {
            im[i].depth = depth[i];
            im[i].depth_out = depth_out[i];
            im[i].normals_out = normals_out ? normals_out[i] : nullptr;
        }
        for (int k = 0; k < 4; k++) im[i].K[k] = K4[4 * (size_t)i + k];
    }
    CallStats stats(*b, dvo::g_kernel_launches);
    IHIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up_total, hipMemcpyHostToDevice, b->stream));
    IHIP(b, (hipError_t)launch_icp_prepare(reinterpret_cast<const PrepareImage *>(b->upload.dev.get()), P, count, depth_format, rows, cols,
                                           normals_out != nullptr, b->stream));
    stats.launched();
    if (staged) IHIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    IHIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    if (staged)
        for (int i = 0; i < count; i++) {
            std::memcpy(depth_out[i], b->out.host + out_per * (size_t)i, f_raw);
            if (normals_out) std::memcpy(normals_out[i], b->out.host + out_per * (size_t)i + f_bytes, n_raw);
        }
    return DVO_OK;
}

int dvo_icp_align(dvo_icp_batch *b, const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                  const void *const *now_depth, const void *const *model_depth, const float *const *model_normals, const double *model_poses12,
                  const double *start_poses12, double *poses12_out, dvo_icp_record *records, int flags) {
    return dvo_icp_align_gated(b, p, count, now_format, model_format, rows, cols, K4, now_depth, model_depth, model_normals, model_poses12, start_poses12,
                               nullptr, 0.0, poses12_out, records, flags);
}

int dvo_icp_align_gated(dvo_icp_batch *b, const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                        const void *const *now_depth, const void *const *model_depth, const float *const *model_normals, const double *model_poses12,
                        const double *start_poses12, const float *const *now_normals, double normal_cos_min, double *poses12_out,
                        dvo_icp_record *records, int flags) {
    if (!b) return DVO_ERR_INVALID;
    dvo_icp_params P;
    if (p) P = *p; else params_default(&P);
    /* refusals first: a refused call writes nothing */
    if (!params_ok(&P))
        return ifail(b, DVO_ERR_INVALID, "bad parameters (levels in [1, DVO_ICP_MAX_LEVELS], iterations in [0, DVO_ICP_MAX_ITERATIONS], 0 < z_near < z_far, "
                                         "dist_max > 0, huber and stop_norm >= 0, min_pivot_ratio inside (0, 1), all finite, min_count >= 1)");
    if (count < 1 || !K4 || !now_depth || !model_depth || !model_normals || !model_poses12 || !start_poses12 || !poses12_out || !records)
        return ifail(b, DVO_ERR_INVALID, "count < 1 or a NULL argument");
    if (count > b->max_views) return ifail(b, DVO_ERR_INVALID, "count above max_views");
    if (!shape_ok(rows, cols) || !format_ok(now_format) || !format_ok(model_format))
        return ifail(b, DVO_ERR_INVALID, "rows or cols < 1, rows * cols > DVO_ICP_MAX_PIXELS, or an unknown depth format");
    if (flags != 0 && flags != DVO_UPLOAD_DEVICE) return ifail(b, DVO_ERR_INVALID, "unknown flags (0 or DVO_UPLOAD_DEVICE)");
    const bool gated = now_normals != nullptr;
    if (gated && (!finite(normal_cos_min) || normal_cos_min < -1.0 || normal_cos_min > 1.0))
        return ifail(b, DVO_ERR_INVALID, "normal_cos_min not finite or outside [-1, 1]");
    for (int i = 0; i < count; i++) {
        if (!now_depth[i] || !model_depth[i] || !model_normals[i] || (gated && !now_normals[i])) return ifail(b, DVO_ERR_INVALID, "a NULL image");
        if (!frame_ok(K4 + 4 * (size_t)i, model_poses12 + 12 * (size_t)i) || !frame_ok(K4 + 4 * (size_t)i, start_poses12 + 12 * (size_t)i))
            return ifail(b, DVO_ERR_INVALID, "view " + std::to_string(i) + ": a K4 or pose that is not finite, or fx / fy not positive");
    }
    const bool staged = flags != DVO_UPLOAD_DEVICE;
    const size_t pixels = (size_t)rows * (size_t)cols;
    const size_t now_raw = pixels * dvo_tsdf::depth_pixel_bytes(now_format), model_raw = pixels * dvo_tsdf::depth_pixel_bytes(model_format);
    const size_t normals_raw = 12 * pixels;
    const size_t now_bytes = pad16(now_raw), model_bytes = pad16(model_raw), normals_bytes = pad16(normals_raw);
    /* the upload: the views with their states, [now images, model images, normals, now normals of a gated call] */
    const size_t images_at = pad16(sizeof(DeviceView) * (size_t)count), per_view = now_bytes + model_bytes + normals_bytes + (gated ? normals_bytes : 0);
    const size_t up_total = images_at + (staged ? per_view * (size_t)count : 0);
    const size_t out_total = sizeof(DeviceResult) * (size_t)count;
    const unsigned stride = sweep_blocks(level_entries(rows, cols, 0));
    const size_t n_partials = (size_t)count * kSlots * stride;
    if ((unsigned long long)stride * (unsigned long long)count > 0x7FFFFFFFull) return ifail(b, DVO_ERR_INVALID, "more workgroups than one launch holds");
    OnDevice guard(b->device);
    /* every block grows before anything is enqueued */
    IHIP(b, b->upload.reserve(up_total));
    IHIP(b, b->out.reserve(out_total));
    if (n_partials > b->partials.size()) IHIP(b, b->partials.alloc(n_partials));
    DeviceView *dv = reinterpret_cast<DeviceView *>(b->upload.host.get());
    for (int i = 0; i < count; i++) {
        const void *now = now_depth[i], *model = model_depth[i];
        const float *normals = model_normals[i], *gate = gated ? now_normals[i] : nullptr;
        if (staged) {
            const size_t o = images_at + per_view * (size_t)i;
            std::memcpy(b->upload.host + o, now_depth[i], now_raw);
            std::memcpy(b->upload.host + o + now_bytes, model_depth[i], model_raw);
            std::memcpy(b->upload.host + o + now_bytes + model_bytes, model_normals[i], normals_raw);
            now = b->upload.dev + o;
            model = b->upload.dev + o + now_bytes;
            normals = reinterpret_cast<const float *>(b->upload.dev + o + now_bytes + model_bytes);
            if (gated) {
                std::memcpy(b->upload.host + o + now_bytes + model_bytes + normals_bytes, now_normals[i], normals_raw);
                gate = reinterpret_cast<const float *>(b->upload.dev + o + now_bytes + model_bytes + normals_bytes);
            }
        }
        std::memset(&dv[i], 0, sizeof(DeviceView));
        dv[i].view = make_view(K4 + 4 * (size_t)i, model_poses12 + 12 * (size_t)i, now, model, normals, gate);
        state_start(dv[i].state, start_poses12 + 12 * (size_t)i);
    }
    CallArgs a;
    a.views = reinterpret_cast<DeviceView *>(b->upload.dev.get());
    a.partials = b->partials;
    a.results = reinterpret_cast<DeviceResult *>(b->out.dev.get());
    a.c = sweep_const(P, now_format, model_format, rows, cols, gated ? normal_cos_min : 0.0);
    a.gated = gated;
    a.p = P;
    a.count = count;
    a.stride = stride;
    CallStats stats(*b, dvo::g_kernel_launches);
    IHIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up_total, hipMemcpyHostToDevice, b->stream));
    for (int level = P.levels - 1; level >= 0; level--)
        for (int it = 0; it < P.iterations[level]; it++) IHIP(b, (hipError_t)launch_icp_sweep(a, level, false, b->stream));
    IHIP(b, (hipError_t)launch_icp_sweep(a, 0, true, b->stream));
    stats.launched();
    IHIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    IHIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    const DeviceResult *res = reinterpret_cast<const DeviceResult *>(b->out.host.get());
    for (int i = 0; i < count; i++) {
        std::memcpy(poses12_out + 12 * (size_t)i, res[i].pose12, 96);
        records[i] = res[i].record;
    }
    return DVO_OK;
}

int dvo_icp_stats(dvo_icp_batch *b, int *last_launches, int *last_syncs) {
    return b ? b->stats(last_launches, last_syncs) : DVO_ERR_INVALID;
}

}  // extern "C"
