/*
 * dvo_upload_plan.h -- the SHAPE of a frame upload, decided from a handful of integers: the pyramid's level sizes, the bytes per
 * pixel and the image strides of the landing buffer, which of the four routes the sources take, how many frames form a chunk, the
 * workgroups of a gather launch, whether a chunk's copies are submitted ahead of the previous chunk's kernels, and the refusals
 * that depend on the arguments alone.  dvo_capi_frames.cpp gathers the facts from the call and the context, asks here and carries
 * the answer out on the device; nothing in this file touches a context, the device or the environment.
 * Host only, no HIP header: tests/host/upload_plan_main.cpp walks it under a sanitizer.  Internal; not installed.
 */
#ifndef DVO_UPLOAD_PLAN_H_
#define DVO_UPLOAD_PLAN_H_

#include "../../include/dvo_amd.h"      /* DVO_UPLOAD_*, DVO_CAM_*, DVO_DEPTH_*, DVO_PIX_*, DVO_OK, DVO_ERR_* */

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace dvo_host {

/* a constant of a HIP header this file cannot include; dvo_capi_frames.cpp asserts they agree */
constexpr int PLAN_LEVELS = 8;                     /* DVO_LEVELS of dvo_launch.h */

constexpr size_t kUploadHalf = (size_t)32 << 20;   /* landing buffer per pipeline stage */
constexpr size_t kSmallImage = (size_t)256 << 10;  /* images up to this size are gathered on the host before they go up */
constexpr size_t kMappedHalf = (size_t)64 << 20;   /* ... when a kernel pulls them out of mapped host memory */
constexpr size_t kDeviceHalf = (size_t)512 << 20;  /* landing buffer per stage when the sources are device buffers: whole batches */
constexpr int kGatherImages = 32;                  /* images of one gather launch */

inline int round_half_even_pos(double v) {         /* cvRound for the non-negative sizes used here */
    const double f = std::floor(v);
    const double d = v - f;
    int i = (int)f;
    if (d > 0.5 || (d == 0.5 && (i & 1))) i++;
    return i;
}

/* slots of a store nobody reserved (dvo_frames_reserve) */
inline int frames_default_slots(int n_pairs) { return std::min(2 * n_pairs + 2, 64); }
inline bool slot_range_ok(int first_slot, int count, int n_slots, int n_pairs) {
    return first_slot >= 0 && first_slot + count <= (n_slots ? n_slots : frames_default_slots(n_pairs));
}
inline bool now_range_ok(int now_first_pair, int count, int n_pairs) {      /* < 0: the frames become nobody's now frames */
    return now_first_pair < 0 || (now_first_pair < n_pairs && now_first_pair + count <= n_pairs);
}
inline size_t pix_bytes(int dtype) { return dtype == DVO_PIX_U8 ? 1 : (dtype == DVO_PIX_U16 ? 2 : 4); }
inline size_t round16(size_t bytes) { return (bytes + 15) / 16 * 16; }
/* mapped host memory: ~32 workgroups per launch of up to 32 images keep the link busy (128 KB in flight) without taking
 * the wave slots the previous chunk's preprocessing needs; a single camera frame gets all 32 */
inline int mapped_gather_wgs(int images) { return std::max(1, kGatherImages / std::min(images, kGatherImages)); }

/* A refusal: the error code and its message.  `late`: the refusal comes after the caller's own (those that need the
 * context), which today precede it -- everything else in the plan is valid beside it, for those checks to read. */
struct UploadRefusal {
    int err = DVO_OK;
    const char *msg = nullptr;
    bool late = false;
};
template <class Plan>
Plan upload_refusal(Plan p, const char *msg, bool late = false) {
    p.err = DVO_ERR_INVALID; p.msg = msg; p.late = late;
    return p;
}

/* ---- dvo_frames_upload_cameras_fmt -------------------------------------------------------------------------------------------- */
enum UploadRoute {
    ROUTE_IN_PLACE,     /* device sources the level kernels read where they are, through a table of their addresses */
    ROUTE_GATHER,       /* device or mapped host sources, gathered into the landing buffer by a kernel */
    ROUTE_DMA,          /* DVO_UPLOAD_DIRECT: one copy per image out of the caller's memory */
    ROUTE_MIRROR        /* memcpy into the pinned mirror of the landing buffer, two copies per chunk */
};

struct CameraFacts {
    int first_slot = 0, count = 0, rows = 0, cols = 0, n_levels = 0, first_shift = 0;
    int image_format = DVO_CAM_BGR8, depth_format = DVO_DEPTH_F32;
    bool has_images = false;        /* the image pointer array is there */
    bool has_depth = false;
    bool null_image = false;        /* some image (or, with depth, some depth image) of the call is NULL */
    bool aligned = false;           /* every source meets the in-place alignment: 4 bytes the image, 4 * dpp bytes the depth image */
    int flags = 0;
    int now_first_pair = -1, n_pairs = 1;
    int n_slots = 0;                /* of the store; 0: not reserved yet */
};

struct CameraPlan : UploadRefusal {
    int rows[PLAN_LEVELS] = {0}, cols[PLAN_LEVELS] = {0};
    size_t bpp = 0, dpp = 0;        /* the sources' real bytes per pixel */
    size_t b_img = 0, d_img = 0;    /* image strides of the landing buffer, in bytes */
    size_t d_px = 0;                /* ... of the depth images, in pixels */
    UploadRoute route = ROUTE_MIRROR;
    bool device_sources = false;
    int chunk = 1;
    bool copies_ahead = false;      /* chunk k+1's copies are submitted before chunk k's kernels */
    bool mirror = false;            /* the landing buffers need their pinned mirrors */
    size_t landing_bytes = 0;       /* of each landing buffer; 0: none */
    int table_entries = 0;          /* of the in-place address table: `count` images, then `count` depth images */
    /* workgroups per image of the gather launch of a chunk of `images` */
    int gather_wgs(int images) const { return device_sources ? 64 : mapped_gather_wgs(images); }
};

inline CameraPlan plan_camera_upload(const CameraFacts &f) {
    CameraPlan p;
    if (f.image_format != DVO_CAM_BGR8 && f.image_format != DVO_CAM_RGB8 && f.image_format != DVO_CAM_MONO8)
        return upload_refusal(p, "unknown image format (DVO_CAM_BGR8 / DVO_CAM_RGB8 / DVO_CAM_MONO8)");
    if (f.depth_format != DVO_DEPTH_F32 && f.depth_format != DVO_DEPTH_U16)
        return upload_refusal(p, "unknown depth format (DVO_DEPTH_F32 / DVO_DEPTH_U16)");
    if (!f.has_images || f.count < 1 || f.rows < 1 || f.cols < 1 || f.n_levels < 1 || f.n_levels > PLAN_LEVELS || f.first_shift < 0 ||
        f.first_shift + f.n_levels > 16)
        return upload_refusal(p, "bad camera frame arguments");
    if (f.null_image) return upload_refusal(p, "NULL camera image");
    for (int l = 0; l < f.n_levels; l++) {          /* cv::resize(Size(), s, s): dsize = cvRound(size * s) */
        const double sc = std::ldexp(1.0, -(f.first_shift + l));
        p.rows[l] = round_half_even_pos(f.rows * sc); p.cols[l] = round_half_even_pos(f.cols * sc);
        if (p.rows[l] < 1 || p.cols[l] < 1) return upload_refusal(p, "pyramid level would be empty");
    }
    if (!now_range_ok(f.now_first_pair, f.count, f.n_pairs)) return upload_refusal(p, "now_first_pair range out of bounds");

    const size_t npx = (size_t)f.rows * f.cols;
    /* the sources' real bytes per pixel size the landing buffers, the copies and the read-in-place alignment */
    p.bpp = f.image_format == DVO_CAM_MONO8 ? 1 : 3; p.dpp = f.depth_format == DVO_DEPTH_U16 ? 2 : 4;
    p.b_img = round16(npx * p.bpp);
    p.d_img = !f.has_depth ? 0 : (p.dpp == 2 ? round16(npx * 2) : npx * 4);      /* 16-bit depth images: 16-byte aligned, like the colour images */
    p.d_px = p.d_img / p.dpp;                                                    /* ... their stride in pixels */
    p.device_sources = (f.flags & DVO_UPLOAD_DEVICE) != 0;                       /* no PCIe to overlap with: whole batches per stage */
    const bool pulled = p.device_sources || (f.flags & DVO_UPLOAD_MAPPED);       /* device-addressable sources: gathered by a kernel, no pinned mirror */
    /* Frames already in HBM are read where they are (round 6): their addresses go up as a table and the level kernels index it -- no
     * landing copy (per 256 VGA frames 236 MB each way, 71 us, and a stream hand-over: 1.60 -> 1.5 ms per `frames in HBM -> poses` step).
     * Needs the alignment of the widest load of the level kernels (4 bytes of the image; 16 of float depth, 8 of 16-bit depth); other
     * sources take the copy. */
    const bool in_place = p.device_sources && f.aligned;
    p.route = in_place ? ROUTE_IN_PLACE : (pulled ? ROUTE_GATHER : ((f.flags & DVO_UPLOAD_DIRECT) ? ROUTE_DMA : ROUTE_MIRROR));
    const size_t half = p.device_sources ? kDeviceHalf : ((f.flags & DVO_UPLOAD_MAPPED) ? kMappedHalf : kUploadHalf);
    p.chunk = in_place ? f.count : (int)std::min<size_t>(std::max<size_t>(half / (p.b_img + p.d_img), 1), (size_t)f.count);
    /* whole gather launches of 32 images: a short tail launch runs far below the link rate */
    if (p.route == ROUTE_GATHER && p.chunk > kGatherImages) p.chunk -= p.chunk % kGatherImages;
    /* pull kernels (few workgroups, latency-bound on the link) go in ahead of the chunk's preprocessing and run beside
     * it; DMA / blit copies submitted ahead would hold the preprocessing back instead (measured: 14.6 -> 22 ms per 256
     * frames with depth), so they keep their place behind it */
    p.copies_ahead = pulled;
    p.mirror = !pulled;
    p.landing_bytes = in_place ? 0 : (p.b_img + p.d_img) * (size_t)p.chunk;
    p.table_entries = in_place ? 2 * f.count : 0;
    if (!slot_range_ok(f.first_slot, f.count, f.n_slots, f.n_pairs))
        return upload_refusal(p, "frame slot range out of bounds (dvo_frames_reserve)", true);
    return p;
}

/* ---- dvo_frames_upload_pyramids ----------------------------------------------------------------------------------------------- */
struct PyramidFacts {
    int first_slot = 0, count = 0, n_levels = 0;
    bool has_grey = false, has_depth = false;
    /* of the first frame's images (the caller checks that every frame's agree, and refuses empty levels and foreign dtypes) */
    int rows[PLAN_LEVELS] = {0}, cols[PLAN_LEVELS] = {0};
    int grey_dtype[PLAN_LEVELS] = {0}, depth_dtype[PLAN_LEVELS] = {0};
    int flags = 0;
    int now_first_pair = -1, n_pairs = 1;
    int n_slots = 0;
};

struct PyramidPlan : UploadRefusal {
    /* landing layout: per level, `chunk` grey images then `chunk` depth images, every image 16-byte aligned */
    size_t g_img[PLAN_LEVELS] = {0}, d_img[PLAN_LEVELS] = {0}, g_off[PLAN_LEVELS] = {0}, d_off[PLAN_LEVELS] = {0};
    size_t frame_bytes = 0;
    int chunk = 1;
    bool mapped = false;            /* pinned host memory the GPU addresses: pulled by a kernel (dvo_amd.h) */
    bool mirror = false;
    size_t landing_bytes = 0;
    /* A sub-megabyte hipMemcpyAsync costs ~10 us of host time however small it is, and a pyramid is mostly small
     * images (the reference's 320x240 ... 40x30 levels: eight per frame): those are gathered into the pinned mirror
     * of the landing buffer with memcpy and go up in one copy per run of small levels; big images go up directly. */
    bool small[PLAN_LEVELS] = {false};
    int n_runs = 0;
    size_t run_lo[PLAN_LEVELS] = {0}, run_hi[PLAN_LEVELS] = {0};      /* [lo, hi) of the landing buffer: one copy per maximal run of small levels */
};

inline PyramidPlan plan_pyramid_upload(const PyramidFacts &f) {
    PyramidPlan p;
    if (!f.has_grey || f.count < 1 || f.n_levels < 1 || f.n_levels > PLAN_LEVELS) return upload_refusal(p, "bad frame arguments");
    size_t npx[PLAN_LEVELS];
    for (int l = 0; l < f.n_levels; l++) {
        npx[l] = (f.rows[l] > 0 && f.cols[l] > 0) ? (size_t)f.rows[l] * f.cols[l] : 0;      /* an empty level is the caller's to refuse */
        p.g_img[l] = round16(npx[l] * pix_bytes(f.grey_dtype[l]));
        p.d_img[l] = f.has_depth ? round16(npx[l] * pix_bytes(f.depth_dtype[l])) : 0;
        p.frame_bytes += p.g_img[l] + p.d_img[l];
    }
    p.mapped = (f.flags & DVO_UPLOAD_MAPPED) != 0;
    p.mirror = !p.mapped;
    p.chunk = (int)std::min<size_t>(std::max<size_t>((p.mapped ? kMappedHalf : kUploadHalf) / std::max<size_t>(p.frame_bytes, 1), 1), (size_t)f.count);
    p.landing_bytes = p.frame_bytes * (size_t)p.chunk;
    size_t o = 0;
    for (int l = 0; l < f.n_levels; l++) { p.g_off[l] = o; o += p.g_img[l] * p.chunk; p.d_off[l] = o; o += p.d_img[l] * p.chunk; }
    for (int l = 0; l < f.n_levels; l++) {
        const size_t gb = pix_bytes(f.grey_dtype[l]), db = f.has_depth ? pix_bytes(f.depth_dtype[l]) : 0;
        p.small[l] = !p.mapped && (!(f.flags & DVO_UPLOAD_DIRECT) || npx[l] * std::max(gb, db) <= kSmallImage);     /* default: through the pinned mirror */
    }
    for (int l = 0; l < f.n_levels;) {
        if (!p.small[l]) { l++; continue; }
        int e = l;
        while (e + 1 < f.n_levels && p.small[e + 1]) e++;
        p.run_lo[p.n_runs] = p.g_off[l];
        p.run_hi[p.n_runs] = (e + 1 < f.n_levels) ? p.g_off[e + 1] : p.landing_bytes;
        p.n_runs++;
        l = e + 1;
    }
    if (!slot_range_ok(f.first_slot, f.count, f.n_slots, f.n_pairs))
        return upload_refusal(p, "frame slot range out of bounds (dvo_frames_reserve)", true);
    if (!now_range_ok(f.now_first_pair, f.count, f.n_pairs)) return upload_refusal(p, "now_first_pair range out of bounds", true);
    return p;
}

}  // namespace dvo_host
#endif
