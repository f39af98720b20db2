/*
 * dvo_capi_frames.cpp -- the frame-store half of the C ABI (include/dvo_amd.h, "frames in"): SURVEY.md section 8f rows
 * f1 + f2.  Host side only: slabs, uploads (double-buffered landing buffers, two copy streams, pinned mirror for small
 * images), kernel launches of dvo_frames.hip.  No CPU compute path.
 */
#include "dvo_ctx.h"
#include "dvo_mask_levels.h"
#include <chrono>
#include <cstdio>

using namespace dvo;
using namespace dvo_host;

namespace {
/* the map pair p's frames are remapped with: the context's, none, or one of the shared per-pair maps */
void pair_umap_of(const dvo_ctx *c, int p, const short2 *&xy, const unsigned short *&frac) {
    const int m = c->pair_umap.empty() ? -1 : c->pair_umap[p];
    if (m < 0) { xy = c->d_umap_xy; frac = c->d_umap_frac; }
    else if (m == 0) { xy = nullptr; frac = nullptr; }
    else { xy = c->umaps[m - 1].xy; frac = c->umaps[m - 1].frac; }
}
}  // namespace

extern "C" {

/* ---- frame store: rows f1 + f2 ------------------------------------------------------------------------ */
namespace {

constexpr size_t kWorkBudget = (size_t)1 << 30;     /* scratch per chunk of a batched preprocessing call */

int round_half_even_pos(double v) {                 /* cvRound for the non-negative sizes used here */
    const double f = std::floor(v);
    const double d = v - f;
    int i = (int)f;
    if (d > 0.5 || (d == 0.5 && (i & 1))) i++;
    return i;
}

void canny_thresholds(const dvo_ctx *c, int *low, int *high) {
    double t1 = c->prm.canny_threshold1, t2 = c->prm.canny_threshold2;
    if (t1 == 0 && t2 == 0) { t1 = 150; t2 = 100; }               /* SolveDVO.cpp:1704, :1764 */
    double lo = std::min(t1, t2), hi = std::max(t1, t2);          /* the detector swaps them */
    lo = std::min(32767.0, lo); hi = std::min(32767.0, hi);
    if (lo > 0) lo *= lo;                                         /* L2gradient: squared magnitudes */
    if (hi > 0) hi *= hi;
    *low = (int)std::floor(lo); *high = (int)std::floor(hi);
}

int frames_default_slots(const dvo_ctx *c) { return std::min(2 * c->n_pairs + 2, 64); }

void frames_free(dvo_ctx *c) {
    for (FrameLevel &F : c->fs.lv) F = FrameLevel();
    c->fs.n_levels = 0;
    std::fill(c->fs.valid.begin(), c->fs.valid.end(), 0);
}

/* make the store hold `n_levels` levels of the given geometry (drops the stored frames if it changes) */
int frames_geometry(dvo_ctx *c, int n_levels, const int *rows, const int *cols) {
    FrameStore &S = c->fs;
    for (int l = 0; l < n_levels; l++)      /* squared distances are kept in 32-bit integers: (rows+cols+1)^2 < 2^31 */
        if ((long long)rows[l] + cols[l] + 1 > 46340)
            return fail(c, DVO_ERR_INVALID, "image too large for the exact distance transform (rows + cols must stay below 46339)");
    if (S.n_slots == 0) {
        S.n_slots = frames_default_slots(c);
        S.valid.assign(S.n_slots, 0); S.has_depth.assign(S.n_slots, 0);
    }
    bool same = S.n_levels == n_levels;
    for (int l = 0; same && l < n_levels; l++) same = S.lv[l].rows == rows[l] && S.lv[l].cols == cols[l];
    if (same) return DVO_OK;
    HIPCHK(c, stream_wait(c->stream));
    frames_free(c);
    for (int l = 0; l < n_levels; l++) {
        FrameLevel &F = S.lv[l];
        F.rows = rows[l]; F.cols = cols[l]; F.npx = (size_t)rows[l] * cols[l];
        HIPCHK(c, F.grey.alloc(F.npx * S.n_slots));
        HIPCHK(c, F.edge.alloc(F.npx * S.n_slots));
        HIPCHK(c, F.depth.alloc(F.npx * S.n_slots));
    }
    S.n_levels = n_levels;
    return DVO_OK;
}

bool slots_ok(const dvo_ctx *c, int first, int count) {
    return first >= 0 && count >= 1 && first + count <= c->fs.n_slots;
}

int chunk_for(size_t bytes_per_image, int count) {
    size_t k = kWorkBudget / std::max<size_t>(bytes_per_image, 1);
    if (k < 1) k = 1;
    return (int)std::min<size_t>(k, (size_t)count);
}

/* the now levels' texel slabs of every level, before a chunk's kernels are enqueued.  (Round 3 also ran the levels of small batches
 * on streams of their own, forked from and joined back into the context stream: ~0.13 ms saved per 640x480 frame on an idle GPU,
 * but a process that is not the first on the GPU found the cross-queue waits taking 14-33 ms EACH FRAME -- profiles/
 * r03_single_stream.  One stream, levels back to back.) */
int ensure_now_texels(dvo_ctx *c, int n_levels) {
    for (int l = 0; l < n_levels; l++) {
        const int rc = ensure_texels(c, l, c->fs.lv[l].rows, c->fs.lv[l].cols);
        if (rc) return rc;
    }
    return DVO_OK;
}

int run_canny(dvo_ctx *c, int level, int first_slot, int count, hipStream_t stream) {
    FrameLevel &F = c->fs.lv[level];
    int low, high;
    canny_thresholds(c, &low, &high);
    const int chunk = chunk_for(sizeof(int) * canny_work_ints(F.rows, F.cols, 1), count);
    int rc = ensure_work(c, sizeof(int) * canny_work_ints(F.rows, F.cols, chunk));
    if (rc) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b);
        const size_t off = (size_t)(first_slot + b) * F.npx;
        HIPCHK(c, launch_canny(F.grey + off, F.npx, ImgBatch{F.rows, F.cols, nc}, low, high, c->work,
                               F.edge + off, F.npx, stream));
    }
    return DVO_OK;
}

/* Canny of all pyramid levels of `count` stored frames: four launches for all levels when the images allow it, else per level */
int run_canny_all(dvo_ctx *c, int n_levels, int first_slot, int count, hipStream_t stream) {
    int rows[DVO_LEVELS], cols[DVO_LEVELS];
    unsigned char *edge[DVO_LEVELS]; size_t estride[DVO_LEVELS];
    for (int l = 0; l < n_levels; l++) {
        const FrameLevel &F = c->fs.lv[l];
        rows[l] = F.rows; cols[l] = F.cols; estride[l] = F.npx; edge[l] = F.edge + (size_t)first_slot * F.npx;
    }
    if (!canny_levels_ok(n_levels, rows, cols, edge, estride)) {
        for (int l = 0; l < n_levels; l++) { const int rc = run_canny(c, l, first_slot, count, stream); if (rc) return rc; }
        return DVO_OK;
    }
    int low, high;
    canny_thresholds(c, &low, &high);
    const int chunk = chunk_for(sizeof(int) * canny_levels_work_ints(n_levels, rows, cols, 1), count);
    int rc = ensure_work(c, sizeof(int) * canny_levels_work_ints(n_levels, rows, cols, chunk));
    if (rc) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b);
        const unsigned char *grey[DVO_LEVELS]; size_t gstride[DVO_LEVELS]; unsigned char *e[DVO_LEVELS];
        for (int l = 0; l < n_levels; l++) {
            const FrameLevel &F = c->fs.lv[l];
            grey[l] = F.grey + (size_t)(first_slot + b) * F.npx; gstride[l] = F.npx; e[l] = F.edge + (size_t)(first_slot + b) * F.npx;
        }
        HIPCHK(c, launch_canny_levels(n_levels, rows, cols, grey, gstride, e, estride, nc, low, high, c->work, stream));
    }
    return DVO_OK;
}

/* ---- per-pair ignore masks (dvo_frames_set_pair_mask) ---- */
bool pairs_have_mask(const dvo_ctx *c, int first_pair, int count) {
    if (c->pair_mask.empty()) return false;
    for (int p = first_pair; p < first_pair + count; p++)
        if (c->pair_mask[p] > 0) return true;
    return false;
}
/* the first pair of [first_pair, first_pair + count) whose mask was built for another level geometry; -1: none */
int mask_geometry_mismatch(const dvo_ctx *c, int first_pair, int count, int n_levels, const int *rows, const int *cols) {
    if (c->pair_mask.empty()) return -1;
    for (int p = first_pair; p < first_pair + count; p++) {
        if (c->pair_mask[p] <= 0) continue;
        const dvo_ctx::MaskSet &M = c->masks[c->pair_mask[p] - 1];
        bool same = M.n_levels == n_levels;
        for (int l = 0; same && l < n_levels; l++) same = M.rows[l] == rows[l] && M.cols[l] == cols[l];
        if (!same) return p;
    }
    return -1;
}
/* edge &= keep in the store for the frames that become the now frames of pairs first_pair ..: ONE launch for all levels and images
 * (DVO_FRAMES_MASK_LAUNCHES), none when no pair of the chunk has a mask */
int run_edge_masks(dvo_ctx *c, int n_levels, int first_slot, int first_pair, int count, hipStream_t stream) {
    if (!pairs_have_mask(c, first_pair, count)) return DVO_OK;
    int rows[DVO_LEVELS], cols[DVO_LEVELS];
    unsigned char *edge[DVO_LEVELS]; size_t estride[DVO_LEVELS];
    for (int l = 0; l < n_levels; l++) {
        const FrameLevel &F = c->fs.lv[l];
        rows[l] = F.rows; cols[l] = F.cols; estride[l] = F.npx; edge[l] = F.edge + (size_t)first_slot * F.npx;
    }
    HIPCHK(c, launch_edge_mask_levels(n_levels, rows, cols, edge, estride, count, c->d_mask_tab + (size_t)first_pair * DVO_LEVELS, stream));
    return DVO_OK;
}
int mask_table_upload(dvo_ctx *c) {
    const size_t n = (size_t)c->n_pairs * DVO_LEVELS;
    if (!c->d_mask_tab) HIPCHK(c, c->d_mask_tab.alloc(n));
    std::vector<const unsigned char *> tab(n, nullptr);
    for (int p = 0; p < c->n_pairs; p++) {
        if (c->pair_mask[p] <= 0) continue;
        const dvo_ctx::MaskSet &M = c->masks[c->pair_mask[p] - 1];
        for (int l = 0; l < M.n_levels; l++) tab[(size_t)p * DVO_LEVELS + l] = M.keep + M.off[l];
    }
    HIPCHK(c, stream_wait(c->stream));                 /* no launch in flight reads the old table */
    HIPCHK(c, hipMemcpy(c->d_mask_tab, tab.data(), sizeof(const unsigned char *) * n, hipMemcpyHostToDevice));
    return DVO_OK;
}

constexpr size_t kUploadHalf = (size_t)32 << 20;   /* landing buffer per pipeline stage */
constexpr size_t kSmallImage = (size_t)256 << 10;  /* images up to this size are gathered on the host before they go up */
constexpr size_t kMappedHalf = (size_t)64 << 20;   /* ... when a kernel pulls them out of mapped host memory */
constexpr size_t kDeviceHalf = (size_t)512 << 20;  /* landing buffer per stage when the sources are device buffers: whole batches */

/* landing buffers of at least `bytes` each (+ their pinned mirrors when the sources are host buffers) + copy streams + events */
int ensure_upload(dvo_ctx *c, size_t bytes, bool with_host = true) {
    if (!c->copy_stream) {
        /* highest priority: the kernels that pull mapped host memory (DVO_UPLOAD_MAPPED) must not queue behind the
         * preprocessing of the previous chunk -- the PCIe link is the longer pole */
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        HIPCHK(c, hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, prio_hi));
        HIPCHK(c, hipStreamCreateWithPriority(&c->copy_stream2, hipStreamNonBlocking, prio_hi));
        const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;      /* producers and consumers are kernels / DMAs of this device */
        for (int b = 0; b < 2; b++) {
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_copied[b], evf));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_copied2[b], evf));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_done[b], evf));
        }
    }
    const bool grow_dev = bytes > c->up_buf[0].size(), grow_host = with_host && bytes > c->up_host[0].size();
    if (!grow_dev && !grow_host) return DVO_OK;
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream2));
    HIPCHK(c, stream_wait(c->stream));
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2; b++) {
        if (grow_dev && e == hipSuccess) e = c->up_buf[b].alloc(bytes);
        if (grow_host && e == hipSuccess) e = c->up_host[b].alloc(bytes);
        c->up_used[b] = false;
    }
    if (e != hipSuccess)        /* both landing buffers and both mirrors, or none: buffer 0's size speaks for its twin */
        for (int b = 0; b < 2; b++) { c->up_buf[b].reset(); c->up_host[b].reset(); }
    HIPCHK(c, e);
    return DVO_OK;
}
/* stage A of a chunk: returns the landing buffer; copies must go to c->copy_stream */
int upload_begin(dvo_ctx *c, unsigned char **buf, int *slot) {
    const int b = c->up_next;
    if (c->up_used[b]) {                                /* its previous consumer finished */
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_done[b], 0));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream2, c->ev_done[b], 0));
    }
    *buf = c->up_buf[b]; *slot = b;
    return DVO_OK;
}
/* stage B: everything enqueued on c->stream after this sees the copies */
int upload_copied(dvo_ctx *c, int b) {
    HIPCHK(c, hipEventRecord(c->ev_copied[b], c->copy_stream));
    HIPCHK(c, hipEventRecord(c->ev_copied2[b], c->copy_stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied2[b], 0));
    return DVO_OK;
}
/* stage C: the kernels reading the landing buffer are enqueued */
int upload_consumed(dvo_ctx *c, int b) {
    HIPCHK(c, hipEventRecord(c->ev_done[b], c->stream));
    c->up_used[b] = true;
    c->up_next = b ^ 1;
    return DVO_OK;
}

size_t pix_bytes(int dtype) { return dtype == DVO_PIX_U8 ? 1 : (dtype == DVO_PIX_U16 ? 2 : 4); }

}  // namespace

static int frames_as_now_level(dvo_ctx *c, int level, int first_slot, int first_pair, int count, hipStream_t stream);
static int frames_as_now_all(dvo_ctx *c, int n_levels, int first_slot, int first_pair, int count, hipStream_t stream);

int dvo_frames_reserve(dvo_ctx *c, int n_slots) {
    DVO_ENTER(c);
    if (n_slots < 1) return fail(c, DVO_ERR_INVALID, "n_slots must be >= 1");
    HIPCHK(c, stream_wait(c->stream));
    frames_free(c);
    c->fs.n_slots = n_slots;
    c->fs.valid.assign(n_slots, 0);
    c->fs.has_depth.assign(n_slots, 0);
    return DVO_OK;
}

int dvo_frames_num_levels(const dvo_ctx *c) { return c ? c->fs.n_levels : 0; }

int dvo_frames_upload_pyramids(dvo_ctx *c, int first_slot, int count, int n_levels,
                               const dvo_image *grey, const dvo_image *depth, int now_first_pair, int flags) {
    DVO_ENTER(c);
    if (!grey || count < 1 || n_levels < 1 || n_levels > DVO_LEVELS) return fail(c, DVO_ERR_INVALID, "bad frame arguments");
    int rows[DVO_LEVELS], cols[DVO_LEVELS];
    for (int l = 0; l < n_levels; l++) { rows[l] = grey[l].rows; cols[l] = grey[l].cols; }
    for (int f = 0; f < count; f++)
        for (int l = 0; l < n_levels; l++) {
            const dvo_image &g = grey[(size_t)f * n_levels + l];
            if (!g.data || g.rows < 1 || g.cols < 1 || g.rows != rows[l] || g.cols != cols[l] ||
                (g.dtype != DVO_PIX_U8 && g.dtype != DVO_PIX_F32) || g.dtype != grey[l].dtype || g.layout != grey[l].layout)
                return fail(c, DVO_ERR_INVALID, "grey images of one level must share size, dtype (U8/F32) and layout");
            if (depth) {
                const dvo_image &d = depth[(size_t)f * n_levels + l];
                if (!d.data || d.rows != rows[l] || d.cols != cols[l] || (d.dtype != DVO_PIX_U16 && d.dtype != DVO_PIX_F32) ||
                    d.dtype != depth[l].dtype || d.layout != depth[l].layout)
                    return fail(c, DVO_ERR_INVALID, "depth images must match the grey size and share dtype (U16/F32) and layout");
            }
        }
    if (now_first_pair >= 0 && pair_ok(c, now_first_pair) && now_first_pair + count <= c->n_pairs) {
        const int p = mask_geometry_mismatch(c, now_first_pair, count, n_levels, rows, cols);
        if (p >= 0) return fail(c, DVO_ERR_INVALID, "pair " + std::to_string(p) + "'s ignore mask was built for another level geometry (dvo_frames_set_pair_mask)");
    }
    int rc = frames_geometry(c, n_levels, rows, cols);
    if (rc) return rc;
    if (!slots_ok(c, first_slot, count)) return fail(c, DVO_ERR_INVALID, "frame slot range out of bounds (dvo_frames_reserve)");
    if (now_first_pair >= 0 && (!pair_ok(c, now_first_pair) || now_first_pair + count > c->n_pairs))
        return fail(c, DVO_ERR_INVALID, "now_first_pair range out of bounds");
    /* chunks of frames flow through copy (copy stream) -> import + Canny (context stream), double-buffered */
    size_t g_img[DVO_LEVELS], d_img[DVO_LEVELS], g_off[DVO_LEVELS], d_off[DVO_LEVELS], frame_bytes = 0;
    for (int l = 0; l < n_levels; l++) {
        const size_t npx = c->fs.lv[l].npx;
        g_img[l] = (npx * pix_bytes(grey[l].dtype) + 15) / 16 * 16;           /* 16-byte aligned images */
        d_img[l] = depth ? (npx * pix_bytes(depth[l].dtype) + 15) / 16 * 16 : 0;
        frame_bytes += g_img[l] + d_img[l];
    }
    const bool mapped = (flags & DVO_UPLOAD_MAPPED) != 0;   /* pinned host memory the GPU addresses: pulled by a kernel (dvo_amd.h) */
    const int chunk = (int)std::min<size_t>(std::max<size_t>((mapped ? kMappedHalf : kUploadHalf) / frame_bytes, 1), (size_t)count);
    if ((rc = ensure_upload(c, frame_bytes * chunk, !mapped))) return rc;
    std::vector<const void *> srcs;
    {   size_t o = 0;                                   /* landing layout: per level, `chunk` grey images then `chunk` depth images */
        for (int l = 0; l < n_levels; l++) { g_off[l] = o; o += g_img[l] * chunk; d_off[l] = o; o += d_img[l] * chunk; }
    }
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b);
        unsigned char *buf; int ub;
        if ((rc = upload_begin(c, &buf, &ub))) return rc;
        /* A sub-megabyte hipMemcpyAsync costs ~10 us of host time however small it is, and a pyramid is mostly small
         * images (the reference's 320x240 ... 40x30 levels: eight per frame): those are gathered into the pinned mirror
         * of the landing buffer with memcpy and go up in one copy per run of small levels; big images go up directly. */
        unsigned char *hbuf = c->up_host[ub];
        if (c->up_used[ub] && !mapped) {      /* the mirror's previous copies have left: both queues (the cameras path sends its depth half on the second) */
            HIPCHK(c, hipEventSynchronize(c->ev_copied[ub]));
            HIPCHK(c, hipEventSynchronize(c->ev_copied2[ub]));
        }
        bool small[DVO_LEVELS];
        for (int l = 0; l < n_levels && mapped; l++) {      /* one gather launch per level and 32 images, grey and depth on the two copy streams */
            const size_t npx = c->fs.lv[l].npx, gb = pix_bytes(grey[l].dtype), db = depth ? pix_bytes(depth[l].dtype) : 0;
            small[l] = false;
            const int wgs = std::max(1, 32 / std::min(nc, 32));
            srcs.resize(nc);
            for (int i = 0; i < nc; i++) srcs[i] = grey[(size_t)(b + i) * n_levels + l].data;
            HIPCHK(c, launch_gather_images(srcs.data(), nc, buf + g_off[l], npx * gb, g_img[l], c->copy_stream, wgs));
            if (depth) {
                for (int i = 0; i < nc; i++) srcs[i] = depth[(size_t)(b + i) * n_levels + l].data;
                HIPCHK(c, launch_gather_images(srcs.data(), nc, buf + d_off[l], npx * db, d_img[l], c->copy_stream2, wgs));
            }
        }
        for (int l = 0; l < n_levels && !mapped; l++) {
            const size_t npx = c->fs.lv[l].npx, gb = pix_bytes(grey[l].dtype), db = depth ? pix_bytes(depth[l].dtype) : 0;
            small[l] = !(flags & DVO_UPLOAD_DIRECT) || npx * std::max(gb, db) <= kSmallImage;     /* default: through the pinned mirror */
            for (int i = 0; i < nc; i++) {
                const void *gsrc = grey[(size_t)(b + i) * n_levels + l].data;
                const void *dsrc = depth ? depth[(size_t)(b + i) * n_levels + l].data : nullptr;
                if (small[l]) {
                    std::memcpy(hbuf + g_off[l] + g_img[l] * i, gsrc, npx * gb);
                    if (depth) std::memcpy(hbuf + d_off[l] + d_img[l] * i, dsrc, npx * db);
                } else {
                    hipStream_t cs = (i & 1) ? c->copy_stream2 : c->copy_stream;
                    HIPCHK(c, hipMemcpyAsync(buf + g_off[l] + g_img[l] * i, gsrc, npx * gb, hipMemcpyHostToDevice, cs));
                    if (depth) HIPCHK(c, hipMemcpyAsync(buf + d_off[l] + d_img[l] * i, dsrc, npx * db, hipMemcpyHostToDevice, cs));
                }
            }
        }
        for (int l = 0; l < n_levels;) {                                  /* one copy per maximal run of small levels */
            if (!small[l]) { l++; continue; }
            int e = l;
            while (e + 1 < n_levels && small[e + 1]) e++;
            const size_t lo = g_off[l], hi = (e + 1 < n_levels) ? g_off[e + 1] : frame_bytes * chunk;
            HIPCHK(c, hipMemcpyAsync(buf + lo, hbuf + lo, hi - lo, hipMemcpyHostToDevice, c->copy_stream));
            l = e + 1;
        }
        if (now_first_pair >= 0 && (rc = ensure_now_texels(c, n_levels))) return rc;
        if ((rc = upload_copied(c, ub))) return rc;
        for (int l = 0; l < n_levels; l++) {                /* all imports, then release the landing buffer, then the rest */
            FrameLevel &F = c->fs.lv[l];
            const size_t off = (size_t)(first_slot + b) * F.npx;
            const ImgBatch ib{F.rows, F.cols, nc};
            HIPCHK(c, launch_import_grey(buf + g_off[l], grey[l].dtype, grey[l].layout == DVO_LAYOUT_ROW_MAJOR,
                                         g_img[l] / pix_bytes(grey[l].dtype), F.grey + off, F.npx, ib, c->stream));
            if (depth)
                HIPCHK(c, launch_import_depth(buf + d_off[l], depth[l].dtype, depth[l].layout == DVO_LAYOUT_ROW_MAJOR,
                                              d_img[l] / pix_bytes(depth[l].dtype), F.depth + off, F.npx, ib, c->stream));
        }
        if ((rc = upload_consumed(c, ub))) return rc;
        if ((rc = run_canny_all(c, n_levels, first_slot + b, nc, c->stream))) return rc;      /* one launch per stage for all levels */
        if (now_first_pair >= 0 && (rc = run_edge_masks(c, n_levels, first_slot + b, now_first_pair + b, nc, c->stream))) return rc;
        if (now_first_pair >= 0 && (rc = frames_as_now_all(c, n_levels, first_slot + b, now_first_pair + b, nc, c->stream))) return rc;
    }
    for (int f = 0; f < count; f++) { c->fs.valid[first_slot + f] = 1; c->fs.has_depth[first_slot + f] = depth ? 1 : 0; }
    if (!(flags & DVO_UPLOAD_ASYNC)) HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* cv::undistort's map for this camera (OpenCV 2.4 undistort.cpp: undistort() + initUndistortRectifyMap(), CV_16SC2 maps).
 * Built on the host in double precision exactly as OpenCV's CPU code does -- per stripe of min(max(1, 4096/cols), rows) rows
 * the new camera matrix is the camera matrix with cy moved by the stripe's first row, inverted by the 3x3 adjugate formula
 * cv::invert uses; the normalised coordinates advance by running sums along a row -- and uploaded once.
 * cvRound is the x86 cvtsd2si of OpenCV 2.4: round half to even, and INT_MIN ("integer indefinite") for everything that does not
 * fit an int -- u*32 of a calibration that throws a pixel beyond +-2^26 source pixels; (int)lrint() would wrap there instead. */
static bool calibration_ok(int rows, int cols, const double *K4, const double *D5) {
    if (!K4 || !D5 || rows < 1 || cols < 1) return false;
    for (int k = 0; k < 4; k++) if (!std::isfinite(K4[k])) return false;
    for (int k = 0; k < 5; k++) if (!std::isfinite(D5[k])) return false;
    return K4[0] != 0.0 && K4[1] != 0.0;
}
int dvo_undistort_map_host(int rows, int cols, const double *K4, const double *D5, short *xy, unsigned short *fr) {
    if (!calibration_ok(rows, cols, K4, D5) || !xy || !fr) return DVO_ERR_INVALID;
    const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const double k1 = D5[0], k2 = D5[1], p1 = D5[2], p2 = D5[3], k3 = D5[4];
    int stripe0 = std::min(std::max(1, (1 << 12) / std::max(cols, 1)), rows);
    auto cvround = [](double v) { return (v > -2147483648.5 && v < 2147483647.5) ? (int)std::nearbyint(v) : INT32_MIN; };
    for (int y0 = 0; y0 < rows; y0 += stripe0) {
        const int n = std::min(stripe0, rows - y0);
        /* inverse of [[fx 0 cx][0 fy cy'][0 0 1]], cy' = cy - y0, by cofactors: every entry is (minor) * (1/det) */
        const double m[3][3] = {{fx, 0, cx}, {0, fy, cy - y0}, {0, 0, 1}};
        const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
        const double d = 1. / det;
        double ir[9];
        ir[0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d; ir[1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d; ir[2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d;
        ir[3] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d; ir[4] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d; ir[5] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d;
        ir[6] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d; ir[7] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d; ir[8] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d;
        for (int i = 0; i < n; i++) {
            double X = i * ir[1] + ir[2], Y = i * ir[4] + ir[5], W = i * ir[7] + ir[8];
            short *pxy = xy + 2 * ((size_t)(y0 + i) * cols);
            unsigned short *pf = fr + (size_t)(y0 + i) * cols;
            for (int j = 0; j < cols; j++, X += ir[0], Y += ir[3], W += ir[6]) {
                const double w = 1. / W, x = X * w, y = Y * w;
                const double x2 = x * x, y2 = y * y, r2 = x2 + y2, two_xy = 2 * x * y;
                const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((0 * r2 + 0) * r2 + 0) * r2);
                const double u = fx * (x * kr + p1 * two_xy + p2 * (r2 + 2 * x2)) + cx;
                const double v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * two_xy) + cy;
                const int iu = cvround(u * 32), iv = cvround(v * 32);
                pxy[2 * j] = (short)(iu >> 5); pxy[2 * j + 1] = (short)(iv >> 5);
                pf[j] = (unsigned short)((iv & 31) * 32 + (iu & 31));
            }
        }
    }
    return DVO_OK;
}

static int build_undistort_map(dvo_ctx *c, int rows, int cols, const double *K4, const double *D5, DevBuf<short2> &xy_out,
                               DevBuf<unsigned short> &frac_out) {
    const size_t npx = (size_t)rows * cols;
    std::vector<short> xy(2 * npx);
    std::vector<unsigned short> fr(npx);
    if (dvo_undistort_map_host(rows, cols, K4, D5, xy.data(), fr.data()) != DVO_OK) return fail(c, DVO_ERR_INVALID, "bad calibration");
    HIPCHK(c, xy_out.alloc(npx));
    HIPCHK(c, frac_out.alloc(npx));
    HIPCHK(c, hipMemcpy(xy_out, xy.data(), sizeof(short) * 2 * npx, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(frac_out, fr.data(), sizeof(unsigned short) * npx, hipMemcpyHostToDevice));
    return DVO_OK;
}

int dvo_frames_set_undistort(dvo_ctx *c, int rows, int cols, const double *K4, const double *D5) {
    DVO_ENTER(c);
    /* refusals first: a refused call leaves the map in force as it was */
    if ((K4 || D5) && !calibration_ok(rows, cols, K4, D5))
        return fail(c, DVO_ERR_INVALID, "bad calibration (K4 and D5 finite, fx and fy not zero, rows and cols positive)");
    HIPCHK(c, stream_wait(c->stream));
    DevBuf<short2> xy;
    DevBuf<unsigned short> frac;
    if (K4) {
        const int rc = build_undistort_map(c, rows, cols, K4, D5, xy, frac);
        if (rc) return rc;
    }
    c->d_umap_xy = std::move(xy); c->d_umap_frac = std::move(frac);                       /* NULL: switched off, frames are taken as already undistorted */
    c->umap_rows = K4 ? rows : 0; c->umap_cols = K4 ? cols : 0;
    return c->d_umap_xy_tab ? pair_umap_tables_upload(c) : DVO_OK;      /* pairs that follow the context's map see the new one */
}

/* ---- ignore masks: the keep planes of every level (dvo_mask_levels.h is the definition) ---- */
int dvo_mask_levels_host(int rows, int cols, const unsigned char *mask, int n_levels, int first_shift, int margin,
                         unsigned char *const *keep_out, int *level_rows, int *level_cols) {
    return dvo_mask::build(rows, cols, mask, n_levels, first_shift, margin, keep_out, level_rows, level_cols) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_frames_set_pair_mask(dvo_ctx *c, int pair, int rows, int cols, const unsigned char *mask, int n_levels, int first_shift, int margin) {
    DVO_ENTER(c);
    /* refusals first: a refused call leaves every pair's mask in force as it was */
    if (pair < -1 || pair >= c->n_pairs) return fail(c, DVO_ERR_INVALID, "pair out of range (-1: every pair)");
    dvo_ctx::MaskSet M;
    if (mask && !dvo_mask::geometry(rows, cols, n_levels, first_shift, margin, M.rows, M.cols))
        return fail(c, DVO_ERR_INVALID, "bad mask arguments (rows, cols >= 1; n_levels in [1, DVO_MAX_LEVELS]; first_shift >= 0; no empty level; "
                                        "margin in [0, DVO_MASK_MAX_MARGIN])");
    if (!mask && c->pair_mask.empty()) return DVO_OK;                /* no pair has a mask already */
    HIPCHK(c, stream_wait(c->stream));
    int id = 0;
    if (mask) {
        M.n_levels = n_levels;
        const size_t total = mask_levels_bytes(n_levels, M.rows, M.cols, M.off);
        DevBuf<unsigned char> d_mask;
        HIPCHK(c, d_mask.alloc((size_t)rows * cols));
        HIPCHK(c, M.keep.alloc(total));
        HIPCHK(c, hipMemcpy(d_mask, mask, (size_t)rows * cols, hipMemcpyHostToDevice));
        unsigned char *keep[DVO_LEVELS];
        for (int l = 0; l < n_levels; l++) keep[l] = M.keep + M.off[l];
        HIPCHK(c, launch_mask_levels(d_mask, rows, cols, n_levels, first_shift, margin, M.rows, M.cols, keep, c->stream));
        HIPCHK(c, stream_wait(c->stream));                         /* the camera-resolution copy goes with this scope */
        size_t m = 0;
        while (m < c->masks.size() && c->masks[m].users > 0) m++;  /* a free slot, or a new one */
        if (m == c->masks.size()) c->masks.push_back(std::move(M)); else c->masks[m] = std::move(M);
        id = (int)m + 1;
    }
    if (c->pair_mask.empty()) c->pair_mask.assign(c->n_pairs, 0);
    for (int p = (pair < 0 ? 0 : pair); p < (pair < 0 ? c->n_pairs : pair + 1); p++) {
        const int old = c->pair_mask[p];
        if (id > 0) c->masks[id - 1].users++;
        c->pair_mask[p] = id;
        if (old > 0 && --c->masks[old - 1].users == 0) c->masks[old - 1] = dvo_ctx::MaskSet();      /* its last user changed: the planes go */
    }
    return mask_table_upload(c);
}

int dvo_frames_get_pair_mask_level(dvo_ctx *c, int pair, int level, unsigned char *keep_out, int capacity, int *rows, int *cols) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    if (c->pair_mask.empty() || c->pair_mask[pair] <= 0) return fail(c, DVO_ERR_STATE, "pair " + std::to_string(pair) + " has no ignore mask");
    const dvo_ctx::MaskSet &M = c->masks[c->pair_mask[pair] - 1];
    if (level < 0 || level >= M.n_levels) return fail(c, DVO_ERR_INVALID, "mask level out of range");
    if (rows) *rows = M.rows[level];
    if (cols) *cols = M.cols[level];
    if (!keep_out) return DVO_OK;
    const size_t npx = (size_t)M.rows[level] * M.cols[level];
    if (capacity < 0 || (size_t)capacity < npx) return fail(c, DVO_ERR_INVALID, "capacity is smaller than the level (rows * cols bytes)");
    HIPCHK(c, hipMemcpyAsync(keep_out, M.keep + M.off[level], npx, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

int dvo_frames_upload_cameras(dvo_ctx *c, int first_slot, int count, const unsigned char *const *bgr8,
                              const float *const *depth_m, int rows, int cols, int n_levels, int first_shift,
                              int now_first_pair, int flags) {
    return dvo_frames_upload_cameras_fmt(c, first_slot, count, reinterpret_cast<const void *const *>(bgr8), DVO_CAM_BGR8,
                                         reinterpret_cast<const void *const *>(depth_m), DVO_DEPTH_F32, rows, cols, n_levels, first_shift,
                                         now_first_pair, flags);
}

/* bgr8 / depth_m: the images in their sensor formats (the names are those of the first format pair) */
int dvo_frames_upload_cameras_fmt(dvo_ctx *c, int first_slot, int count, const void *const *bgr8, int image_format,
                                  const void *const *depth_m, int depth_format, int rows, int cols, int n_levels, int first_shift,
                                  int now_first_pair, int flags) {
    DVO_ENTER(c);
    if (image_format != DVO_CAM_BGR8 && image_format != DVO_CAM_RGB8 && image_format != DVO_CAM_MONO8)
        return fail(c, DVO_ERR_INVALID, "unknown image format (DVO_CAM_BGR8 / DVO_CAM_RGB8 / DVO_CAM_MONO8)");
    if (depth_format != DVO_DEPTH_F32 && depth_format != DVO_DEPTH_U16)
        return fail(c, DVO_ERR_INVALID, "unknown depth format (DVO_DEPTH_F32 / DVO_DEPTH_U16)");
    if (!bgr8 || count < 1 || rows < 1 || cols < 1 || n_levels < 1 || n_levels > DVO_LEVELS || first_shift < 0 ||
        first_shift + n_levels > 16)
        return fail(c, DVO_ERR_INVALID, "bad camera frame arguments");
    for (int f = 0; f < count; f++)
        if (!bgr8[f] || (depth_m && !depth_m[f])) return fail(c, DVO_ERR_INVALID, "NULL camera image");
    int lr[DVO_LEVELS], lc[DVO_LEVELS];
    for (int l = 0; l < n_levels; l++) {          /* cv::resize(Size(), s, s): dsize = cvRound(size * s) */
        const double sc = std::ldexp(1.0, -(first_shift + l));
        lr[l] = round_half_even_pos(rows * sc); lc[l] = round_half_even_pos(cols * sc);
        if (lr[l] < 1 || lc[l] < 1) return fail(c, DVO_ERR_INVALID, "pyramid level would be empty");
    }
    /* every refusal comes before frames_geometry, which drops the stored frames when the geometry changes */
    if (now_first_pair >= 0 && (!pair_ok(c, now_first_pair) || now_first_pair + count > c->n_pairs))
        return fail(c, DVO_ERR_INVALID, "now_first_pair range out of bounds");
    if (c->d_umap_xy && (c->umap_rows != rows || c->umap_cols != cols))
        return fail(c, DVO_ERR_INVALID, "the undistortion map was built for another image size (dvo_frames_set_undistort)");
    const bool per_pair_maps = now_first_pair >= 0 && !c->pair_umap.empty();
    if (per_pair_maps)
        for (int f = 0; f < count; f++) {
            const int m = c->pair_umap[now_first_pair + f];
            if (m > 0 && (c->umaps[m - 1].rows != rows || c->umaps[m - 1].cols != cols))
                return fail(c, DVO_ERR_INVALID, "pair " + std::to_string(now_first_pair + f) + "'s undistortion map was built for another image size");
        }
    if (now_first_pair >= 0) {
        const int p = mask_geometry_mismatch(c, now_first_pair, count, n_levels, lr, lc);
        if (p >= 0) return fail(c, DVO_ERR_INVALID, "pair " + std::to_string(p) + "'s ignore mask was built for another level geometry (dvo_frames_set_pair_mask)");
    }
    if (first_slot < 0 || first_slot + count > (c->fs.n_slots ? c->fs.n_slots : frames_default_slots(c)))
        return fail(c, DVO_ERR_INVALID, "frame slot range out of bounds (dvo_frames_reserve)");
    int rc = frames_geometry(c, n_levels, lr, lc);
    if (rc) return rc;
    const size_t npx = (size_t)rows * cols;
    /* the sources' real bytes per pixel size the landing buffers, the copies and the read-in-place alignment */
    const size_t bpp = image_format == DVO_CAM_MONO8 ? 1 : 3, dpp = depth_format == DVO_DEPTH_U16 ? 2 : 4;
    const size_t b_img = (npx * bpp + 15) / 16 * 16;
    const size_t d_img = !depth_m ? 0 : (dpp == 2 ? (npx * 2 + 15) / 16 * 16 : npx * 4);      /* 16-bit depth images: 16-byte aligned, like the colour images */
    const size_t d_px = d_img / dpp;                                                          /* ... their stride in pixels */
    const bool dev_src = (flags & DVO_UPLOAD_DEVICE) != 0;     /* no PCIe to overlap with: whole batches per stage */
    const bool pulled = dev_src || (flags & DVO_UPLOAD_MAPPED);  /* device-addressable sources: gathered by a kernel, no pinned mirror */
    /* Frames already in HBM are read where they are (round 6): their addresses go up as a table and the level kernels index it -- no
     * landing copy (per 256 VGA frames 236 MB each way, 71 us, and a stream hand-over: 1.60 -> 1.5 ms per `frames in HBM -> poses` step).
     * Needs the alignment of the widest load of the level kernels (4 bytes of the image; 16 of float depth, 8 of 16-bit depth); other
     * sources take the copy. */
    bool direct = dev_src;
    const size_t d_align = 4 * dpp - 1;
    for (int f = 0; f < count && direct; f++)
        direct = (reinterpret_cast<size_t>(bgr8[f]) & 3) == 0 && (!depth_m || (reinterpret_cast<size_t>(depth_m[f]) & d_align) == 0);
    const size_t half = dev_src ? kDeviceHalf : ((flags & DVO_UPLOAD_MAPPED) ? kMappedHalf : kUploadHalf);
    int chunk = direct ? count : (int)std::min<size_t>(std::max<size_t>(half / (b_img + d_img), 1), (size_t)count);
    if (!direct && pulled && chunk > 32) chunk -= chunk % 32;   /* whole gather launches of 32 images: a short tail launch runs far below the link rate */
    if (!direct && (rc = ensure_upload(c, (b_img + d_img) * chunk, !pulled))) return rc;
    SrcTab tab0 = {nullptr, nullptr};
    if (direct) {
        const int need = 2 * count;
        if ((size_t)need > c->src_tab_host.size()) {
            HIPCHK(c, stream_wait(c->stream));
            c->src_tab_host.reset();                        /* allocated last: its size speaks for both */
            HIPCHK(c, c->src_tab_dev.alloc((size_t)need));
            HIPCHK(c, c->src_tab_host.alloc((size_t)need));
        }
        if (!c->ev_src_tab) HIPCHK(c, hipEventCreateWithFlags(&c->ev_src_tab, hipEventDisableTiming));
        else HIPCHK(c, hipEventSynchronize(c->ev_src_tab));      /* the staging table's previous copy has gone up; the DEVICE table's readers are ahead of this call's copy on the stream */
        for (int f = 0; f < count; f++) {
            c->src_tab_host[f] = const_cast<void *>(bgr8[f]);
            c->src_tab_host[count + f] = depth_m ? const_cast<void *>(depth_m[f]) : nullptr;
        }
        HIPCHK(c, hipMemcpyAsync(c->src_tab_dev, c->src_tab_host, sizeof(void *) * (size_t)need, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_src_tab, c->stream));
        tab0.bgr = c->src_tab_dev;
        tab0.depth = depth_m ? c->src_tab_dev + count : nullptr;
    }
    /* chunk k+1 is copied (copy streams) while chunk k is preprocessed (context stream), over two landing buffers.  The copies
     * of chunk k+1 are SUBMITTED before the kernels of chunk k: measured on this pool (tools/experiments/exp_pull_overlap.sh),
     * work of two streams that becomes ready at the same moment starts in submission order, and a pull submitted after ~45
     * preprocessing launches waited for nearly all of them -- the link idled 0.6 ms of every 1.6 */
    struct Chunk { int b, nc, ub; unsigned char *sb, *sd; };
    int next_ub = c->up_next;
    auto issue_copy = [&](int b, Chunk &k) -> int {
        if (direct) { k.b = b; k.nc = std::min(chunk, count - b); k.ub = -1; k.sb = nullptr; k.sd = nullptr; return DVO_OK; }
        k.b = b; k.nc = std::min(chunk, count - b); k.ub = next_ub; next_ub ^= 1;
        k.sb = c->up_buf[k.ub]; k.sd = k.sb + b_img * chunk;
        if (c->up_used[k.ub]) {                             /* the buffer's previous consumer (two chunks back) has read it */
            HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_done[k.ub], 0));
            HIPCHK(c, hipStreamWaitEvent(c->copy_stream2, c->ev_done[k.ub], 0));
        }
        if (dev_src) {                                       /* device sources may be depth images a registration is still writing on the context stream */
            HIPCHK(c, depth_registered_ready(c, c->copy_stream));
            HIPCHK(c, depth_registered_ready(c, c->copy_stream2));
        }
        if (pulled) {                                        /* in HBM already, or in pinned host memory the GPU addresses: gathered */
            /* mapped host memory: ~32 workgroups per launch of up to 32 images keep the link busy (128 KB in flight) without taking
             * the wave slots the previous chunk's preprocessing needs; a single camera frame gets all 32 */
            const int wgs = dev_src ? 64 : std::max(1, 32 / std::min(k.nc, 32));
            HIPCHK(c, launch_gather_images(bgr8 + b, k.nc, k.sb, npx * bpp, b_img, c->copy_stream, wgs));
            if (depth_m) HIPCHK(c, launch_gather_images(depth_m + b, k.nc, k.sd, npx * dpp, d_img, c->copy_stream2, wgs));
        } else if (flags & DVO_UPLOAD_DIRECT) {
            for (int i = 0; i < k.nc; i++) {
                hipStream_t cs = (i & 1) ? c->copy_stream2 : c->copy_stream;
                HIPCHK(c, hipMemcpyAsync(k.sb + b_img * i, bgr8[b + i], npx * bpp, hipMemcpyHostToDevice, cs));
                if (depth_m) HIPCHK(c, hipMemcpyAsync(k.sd + d_img * i, depth_m[b + i], npx * dpp, hipMemcpyHostToDevice, cs));
            }
        } else {
            /* through the engine's pinned mirror of the landing buffer: one memcpy per image on the host, then two DMAs per
             * chunk; the caller's (pageable) memory is never registered with the driver (include/dvo_amd.h, DVO_UPLOAD_DIRECT) */
            unsigned char *hb = c->up_host[k.ub];
            unsigned char *hd = hb + b_img * chunk;
            if (c->up_used[k.ub]) { HIPCHK(c, hipEventSynchronize(c->ev_copied[k.ub])); HIPCHK(c, hipEventSynchronize(c->ev_copied2[k.ub])); }
            for (int i = 0; i < k.nc; i++) {
                std::memcpy(hb + b_img * i, bgr8[b + i], npx * bpp);
                if (depth_m) std::memcpy(hd + d_img * i, depth_m[b + i], npx * dpp);
            }
            HIPCHK(c, hipMemcpyAsync(k.sb, hb, b_img * (size_t)k.nc, hipMemcpyHostToDevice, c->copy_stream));
            if (depth_m) HIPCHK(c, hipMemcpyAsync(k.sd, hd, d_img * (size_t)k.nc, hipMemcpyHostToDevice, c->copy_stream2));
        }
        HIPCHK(c, hipEventRecord(c->ev_copied[k.ub], c->copy_stream));
        HIPCHK(c, hipEventRecord(c->ev_copied2[k.ub], c->copy_stream2));
        c->up_used[k.ub] = true;                            /* from here on the buffer has a pending ev_copied and, soon, ev_done */
        c->up_next = k.ub ^ 1;                              /* committed per chunk: an error further down leaves events and turn consistent */
        return DVO_OK;
    };
    auto issue_compute = [&](const Chunk &k) -> int {
        int rc2;
        if (now_first_pair >= 0 && (rc2 = ensure_now_texels(c, n_levels))) return rc2;
        const SrcTab tab = direct ? SrcTab{tab0.bgr + k.b, tab0.depth ? tab0.depth + k.b : nullptr} : SrcTab{nullptr, nullptr};
        const void *const dsrc = depth_m ? (direct ? reinterpret_cast<const void *>(16) /* "has depth"; the table holds the addresses */ : k.sd) : nullptr;
        const CamSrc src{k.sb, b_img, image_format, dsrc, d_px, depth_format};
        if (k.ub >= 0) {
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied[k.ub], 0));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied2[k.ub], 0));
        }
        /* undistortion: the context's map for every image, or -- per-pair calibration -- the one map all images of the chunk share, or
         * a table of the pairs' maps when they differ (the chunk stays one launch per stage) */
        const short2 *mxy = c->d_umap_xy;
        const unsigned short *mfr = c->d_umap_frac;
        UmapTab utab{nullptr, nullptr};
        if (per_pair_maps) {
            const int p0 = now_first_pair + k.b;
            pair_umap_of(c, p0, mxy, mfr);
            for (int i = 1; i < k.nc; i++) {
                const short2 *xy; const unsigned short *fr;
                pair_umap_of(c, p0 + i, xy, fr);
                if (xy != mxy) { utab = UmapTab{c->d_umap_xy_tab + p0, c->d_umap_frac_tab + p0}; mxy = nullptr; mfr = nullptr; break; }
            }
        }
        for (int l = 0; l < n_levels; l++) {
            FrameLevel &F = c->fs.lv[l];
            const size_t off = (size_t)(first_slot + k.b) * F.npx;
            if (l == 0 || n_levels == 2)
                HIPCHK(c, launch_camera_level(src, rows, cols, first_shift + l,
                                              mxy, mfr, (flags & DVO_UPLOAD_DEPTH_RAW) ? 1 : 0,
                                              F.grey + off, F.depth + off, F.npx, ImgBatch{F.rows, F.cols, k.nc}, c->stream, tab, utab));
            else if (l == 1) {                               /* levels 1 .. n-1 in one launch */
                int sh[DVO_LEVELS], lr2[DVO_LEVELS], lc2[DVO_LEVELS]; unsigned char *gl[DVO_LEVELS]; float *dl[DVO_LEVELS]; size_t st[DVO_LEVELS];
                for (int m = 1; m < n_levels; m++) {
                    FrameLevel &G = c->fs.lv[m];
                    sh[m - 1] = first_shift + m; lr2[m - 1] = G.rows; lc2[m - 1] = G.cols; st[m - 1] = G.npx;
                    gl[m - 1] = G.grey + (size_t)(first_slot + k.b) * G.npx; dl[m - 1] = G.depth + (size_t)(first_slot + k.b) * G.npx;
                }
                FrameLevel &F0 = c->fs.lv[0];
                if (camera_levels_decimate_ok(n_levels, lr, lc))      /* from level 0, written just before on this stream */
                    HIPCHK(c, launch_camera_decimate_levels(F0.grey + (size_t)(first_slot + k.b) * F0.npx, depth_m ? F0.depth + (size_t)(first_slot + k.b) * F0.npx : nullptr,
                                                            F0.npx, F0.rows, F0.cols, n_levels - 1, lr2, lc2, gl, dl, st, k.nc, c->stream));
                else
                    HIPCHK(c, launch_camera_levels(src, rows, cols, n_levels - 1, sh, lr2, lc2, mxy,
                                                   mfr, (flags & DVO_UPLOAD_DEPTH_RAW) ? 1 : 0, gl, dl, st, k.nc, c->stream, tab, utab));
            }
        }
        if (k.ub >= 0) HIPCHK(c, hipEventRecord(c->ev_done[k.ub], c->stream));     /* the landing buffer is free again */
        if ((rc2 = run_canny_all(c, n_levels, first_slot + k.b, k.nc, c->stream))) return rc2;      /* one launch per stage for all levels */
        if (now_first_pair >= 0 && (rc2 = run_edge_masks(c, n_levels, first_slot + k.b, now_first_pair + k.b, k.nc, c->stream))) return rc2;
        if (now_first_pair >= 0 && (rc2 = frames_as_now_all(c, n_levels, first_slot + k.b, now_first_pair + k.b, k.nc, c->stream))) return rc2;
        return DVO_OK;
    };
    {
        Chunk cur, nxt;
        if ((rc = issue_copy(0, cur))) return rc;
        for (int b = 0; b < count; b += chunk) {
            const bool more = b + chunk < count;
            /* pull kernels (few workgroups, latency-bound on the link) go in ahead of the chunk's preprocessing and run beside
             * it; DMA / blit copies submitted ahead would hold the preprocessing back instead (measured: 14.6 -> 22 ms per 256
             * frames with depth), so they keep their place behind it */
            const bool ahead = pulled;
            if (more && ahead && (rc = issue_copy(b + chunk, nxt))) return rc;
            if ((rc = issue_compute(cur))) return rc;
            if (more && !ahead && (rc = issue_copy(b + chunk, nxt))) return rc;
            cur = nxt;
        }
        if (!direct) c->up_next = next_ub;
    }
    for (int f = 0; f < count; f++) { c->fs.valid[first_slot + f] = 1; c->fs.has_depth[first_slot + f] = depth_m ? 1 : 0; }
    if (!(flags & DVO_UPLOAD_ASYNC)) HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

static int frames_check_use(dvo_ctx *c, int first_slot, int first_pair, int count, bool need_depth) {
    if (c->fs.n_levels < 1) return fail(c, DVO_ERR_STATE, "frame store is empty (dvo_frames_upload_*)");
    if (!slots_ok(c, first_slot, count)) return fail(c, DVO_ERR_INVALID, "frame slot range out of bounds");
    if (!pair_ok(c, first_pair) || first_pair + count > c->n_pairs) return fail(c, DVO_ERR_INVALID, "pair range out of bounds");
    for (int f = first_slot; f < first_slot + count; f++) {
        if (!c->fs.valid[f]) return fail(c, DVO_ERR_STATE, "frame slot " + std::to_string(f) + " holds no frame");
        if (need_depth && !c->fs.has_depth[f]) return fail(c, DVO_ERR_STATE, "frame slot " + std::to_string(f) + " has no depth");
    }
    return DVO_OK;
}

static int frames_as_now_level(dvo_ctx *c, int l, int first_slot, int first_pair, int count, hipStream_t stream) {
    int rc;
    FrameLevel &F = c->fs.lv[l];
    if ((rc = ensure_texels(c, l, F.rows, F.cols))) return rc;
    /* the now level is written in its compact form (dvo_palette.h) straight from the integer squared distances; 16-byte texels
     * only for images that form cannot hold, or when the caller switched the compact form off */
    const bool compact = native_compact_wanted(c);
    if (compact && (rc = ensure_compact_slabs(c, l))) return rc;
    Level &L = c->lv[l];
    unsigned *p4 = compact ? L.p4 : nullptr;
    /* sparse texel slab (dvo_ctx.h): the stage runs without texel output; the images the compact form cannot hold get their
     * texels mapped and written by a second run of the last pass -- per chunk, while the chunk's scratch still holds them */
    const bool defer = compact && L.tex_sparse;
    if (L.tex_sparse && !compact && (rc = map_texels(c, l, first_pair, count, stream))) return rc;
    auto run = [&](const unsigned char *edge, int nc, int *wk, int pair0) -> int {
        HIPCHK(c, launch_edges_to_now(edge, F.npx, ImgBatch{F.rows, F.cols, nc}, wk, defer ? nullptr : L.tex + (size_t)pair0 * L.tex_stride,
                                      L.tex_stride, p4, L.p4_stride, L.pal, L.d_pal_n, pair0, stream));
        if (defer) {
            int n_failed = 0, rc2;
            if ((rc2 = sparse_map_compact_failures(c, l, pair0, nc, stream, &n_failed))) return rc2;
            if (n_failed)
                HIPCHK(c, launch_edges_to_now(edge, F.npx, ImgBatch{F.rows, F.cols, nc}, wk, L.tex + (size_t)pair0 * L.tex_stride, L.tex_stride,
                                              p4, L.p4_stride, L.pal, L.d_pal_n, pair0, stream, true));
        }
        return DVO_OK;
    };
    const int chunk = chunk_for(sizeof(int) * edt_work_ints(F.rows, F.cols, 1), count);
    if ((rc = ensure_work(c, sizeof(int) * edt_work_ints(F.rows, F.cols, chunk)))) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b);
        if ((rc = run(F.edge + (size_t)(first_slot + b) * F.npx, nc, c->work, first_pair + b))) return rc;
    }
    return compact ? now_written_compact(c, l, first_pair, count) : now_written(c, l, first_pair, count);
}

/* every level of `count` stored frames as now levels of pairs first_pair..: one launch per stage for all levels when the
 * geometry allows it (dvo_frames.hip, launch_edges_to_now_levels), else level by level */
static int frames_as_now_all(dvo_ctx *c, int n_levels, int first_slot, int first_pair, int count, hipStream_t stream) {
    int rc;
    int rows[DVO_LEVELS], cols[DVO_LEVELS];
    for (int l = 0; l < n_levels; l++) { rows[l] = c->fs.lv[l].rows; cols[l] = c->fs.lv[l].cols; }
    if (!edt_levels_ok(n_levels, rows, cols)) {
        for (int l = 0; l < n_levels; l++)
            if ((rc = frames_as_now_level(c, l, first_slot, first_pair, count, stream))) return rc;
        return DVO_OK;
    }
    const bool compact = native_compact_wanted(c);
    for (int l = 0; l < n_levels; l++) {
        if ((rc = ensure_texels(c, l, rows[l], cols[l]))) return rc;
        if (compact && (rc = ensure_compact_slabs(c, l))) return rc;
    }
    /* Tried and dropped (round 4): the batch as two halves on two streams with their own scratch, so that the issue-bound row scan
     * of one half runs beside the memory-bound rank pack of the other -- 1.02-1.05 ms per 256 frames against 0.86 ms on one stream
     * (half-size launches fill the GPU less well, and work of two streams starts in submission order on this pool). */
    const int chunk = chunk_for(sizeof(int) * edt_levels_work_ints(n_levels, rows, cols, 1), count);
    if ((rc = ensure_work(c, sizeof(int) * edt_levels_work_ints(n_levels, rows, cols, chunk)))) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b);
        const unsigned char *edge[DVO_LEVELS]; size_t estride[DVO_LEVELS], tstride[DVO_LEVELS], pstride[DVO_LEVELS];
        float4 *tex[DVO_LEVELS]; unsigned *p4[DVO_LEVELS]; float2 *pal[DVO_LEVELS]; int *pal_n[DVO_LEVELS];
        bool defer = false;
        for (int l = 0; l < n_levels; l++) {
            const FrameLevel &F = c->fs.lv[l];
            Level &L = c->lv[l];
            edge[l] = F.edge + (size_t)(first_slot + b) * F.npx; estride[l] = F.npx;
            if (L.tex_sparse && !compact && (rc = map_texels(c, l, first_pair + b, nc, stream))) return rc;
            const bool dl = compact && L.tex_sparse;                 /* sparse texel slab: no texel output in the first run */
            defer = defer || dl;
            tex[l] = dl ? nullptr : L.tex + (size_t)(first_pair + b) * L.tex_stride; tstride[l] = L.tex_stride;
            p4[l] = compact ? L.p4 : nullptr; pstride[l] = L.p4_stride; pal[l] = L.pal; pal_n[l] = L.d_pal_n;
        }
        HIPCHK(c, launch_edges_to_now_levels(n_levels, rows, cols, edge, estride, nc, c->work, tex, tstride, p4, pstride, pal, pal_n,
                                             first_pair + b, stream));
        if (defer) {
            int failed_any = 0;
            for (int l = 0; l < n_levels; l++) {
                Level &L = c->lv[l];
                if (!L.tex_sparse) continue;
                int n_failed = 0;
                if ((rc = sparse_map_compact_failures(c, l, first_pair + b, nc, stream, &n_failed))) return rc;
                failed_any += n_failed;
                tex[l] = L.tex + (size_t)(first_pair + b) * L.tex_stride;      /* only the pairs just mapped are written (pal_n < 0) */
            }
            if (failed_any)
                HIPCHK(c, launch_edges_to_now_levels(n_levels, rows, cols, edge, estride, nc, c->work, tex, tstride, p4, pstride, pal, pal_n,
                                                     first_pair + b, stream, true));
        }
    }
    for (int l = 0; l < n_levels; l++)
        if ((rc = compact ? now_written_compact(c, l, first_pair, count) : now_written(c, l, first_pair, count))) return rc;
    return DVO_OK;
}

int dvo_frames_as_now(dvo_ctx *c, int first_slot, int first_pair, int count) {
    DVO_ENTER(c);
    int rc = frames_check_use(c, first_slot, first_pair, count, false);
    if (rc) return rc;
    return frames_as_now_all(c, c->fs.n_levels, first_slot, first_pair, count, c->stream);
}

int dvo_frames_as_ref(dvo_ctx *c, int first_slot, int first_pair, int count, int *N_out) {
    DVO_ENTER(c);
    if (!c->have_K) return fail(c, DVO_ERR_STATE, "intrinsics not set (dvo_set_intrinsics)");
    int rc = frames_check_use(c, first_slot, first_pair, count, true);
    if (rc) return rc;
    const int nl = c->fs.n_levels;
    size_t cc_off[DVO_LEVELS + 1];                      /* per level: count x (cols+2) column counters ... */
    size_t bc_off[DVO_LEVELS + 1];                      /* ... and count x enlist_block_ints() block-order counters */
    cc_off[0] = 0;
    for (int l = 0; l < nl; l++) cc_off[l + 1] = cc_off[l] + (size_t)count * (c->fs.lv[l].cols + 2);
    bc_off[0] = cc_off[nl];
    for (int l = 0; l < nl; l++) bc_off[l + 1] = bc_off[l] + (size_t)count * enlist_block_ints(c->fs.lv[l].rows, c->fs.lv[l].cols);
    if ((rc = ensure_work(c, sizeof(int) * bc_off[nl]))) return rc;
    std::vector<int> hN((size_t)count * nl);
    for (int l = 0; l < nl; l++) {
        FrameLevel &F = c->fs.lv[l];
        const size_t off = (size_t)first_slot * F.npx;
        int *cc = c->work + cc_off[l];
        HIPCHK(c, launch_enlist_count(F.edge + off, 1, F.npx, F.depth + off, F.npx, ImgBatch{F.rows, F.cols, count}, cc,
                                      c->work + bc_off[l], c->stream));
        HIPCHK(c, hipMemcpy2DAsync(hN.data() + (size_t)l * count, sizeof(int), cc + F.cols, sizeof(int) * (F.cols + 2),
                                   sizeof(int), count, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, stream_wait(c->stream));
    int bad_level = -1, bad_frame = -1;
    for (int l = 0; l < nl; l++) {
        FrameLevel &F = c->fs.lv[l];
        int maxN = 0;
        for (int i = 0; i < count; i++) {
            const int N = hN[(size_t)l * count + i];
            maxN = std::max(maxN, N);
            if (N < 1 && bad_level < 0) { bad_level = l; bad_frame = i; }
            if (N_out) N_out[(size_t)i * nl + l] = N;
        }
        if ((rc = ensure_points(c, l, std::max(maxN, 1)))) return rc;
        Level &L = c->lv[l];
        const size_t off = (size_t)first_slot * F.npx;
        Intrinsics kb = c->K;                           /* the kernel indexes the table by image: pair first_pair + image */
        if (kb.pair_K) kb.pair_K += first_pair;
        HIPCHK(c, launch_enlist_write(F.edge + off, 1, F.npx, F.depth + off, F.npx, ImgBatch{F.rows, F.cols, count}, l, kb,
                                      c->work + cc_off[l], c->work + bc_off[l], L.pts + (size_t)first_pair * L.pt_cap * 3, (size_t)L.pt_cap * 3,
                                      L.cpts + (size_t)first_pair * L.pt_cap, L.cidx + (size_t)first_pair * L.pt_cap, nullptr, L.pt_cap,
                                      L.dN + first_pair, c->stream));
        HIPCHK(c, launch_points4_build(L.cpts, L.dN, L.pt_cap, F.rows, L.cpt4, L.chdr, L.d_pt4_ok, first_pair, count, c->stream));
        for (int i = 0; i < count; i++) { L.hN.w(first_pair + i) = hN[(size_t)l * count + i]; L.compact_ok.w(first_pair + i) = 1; }
        ref_list_written(c, l, first_pair, count, F.rows);
    }
    if (bad_level >= 0)
        return fail(c, DVO_ERR_INVALID, "no reference point selected in frame " + std::to_string(first_slot + bad_frame) +
                                            " level " + std::to_string(bad_level) +
                                            " (reference asserts nSelectedPts > 0, SolveDVO.cpp:282)");
    return DVO_OK;
}

}  // extern "C"

/* dvo_frames_as_ref for any set: slot h_slots[i] becomes the reference frame of pair h_pairs[i], every stage one launch for the whole
 * set (enlist_count / _write and points4_build in their index-list form, d_map[i] = {h_slots[i], h_pairs[i]}); one host
 * synchronisation for the point counts */
int dvo_host::frames_as_ref_list(dvo_ctx *c, const int *h_slots, const int *h_pairs, const int2 *d_map, int count, int *N_out) {
    if (!c->have_K) return fail(c, DVO_ERR_STATE, "intrinsics not set (dvo_set_intrinsics)");
    if (c->fs.n_levels < 1) return fail(c, DVO_ERR_STATE, "frame store is empty (dvo_frames_upload_*)");
    if (count < 1 || !d_map) return fail(c, DVO_ERR_INVALID, "empty slot list");
    for (int i = 0; i < count; i++) {
        const int f = h_slots[i];
        if (!slots_ok(c, f, 1) || !pair_ok(c, h_pairs[i])) return fail(c, DVO_ERR_INVALID, "slot / pair list entry out of bounds");
        if (!c->fs.valid[f]) return fail(c, DVO_ERR_STATE, "frame slot " + std::to_string(f) + " holds no frame");
        if (!c->fs.has_depth[f]) return fail(c, DVO_ERR_STATE, "frame slot " + std::to_string(f) + " has no depth");
    }
    const int nl = c->fs.n_levels;
    size_t cc_off[DVO_LEVELS + 1], bc_off[DVO_LEVELS + 1];
    cc_off[0] = 0;
    for (int l = 0; l < nl; l++) cc_off[l + 1] = cc_off[l] + (size_t)count * (c->fs.lv[l].cols + 2);
    bc_off[0] = cc_off[nl];
    for (int l = 0; l < nl; l++) bc_off[l + 1] = bc_off[l] + (size_t)count * enlist_block_ints(c->fs.lv[l].rows, c->fs.lv[l].cols);
    int rc;
    if ((rc = ensure_work(c, sizeof(int) * bc_off[nl]))) return rc;
    std::vector<int> hN((size_t)count * nl);
    for (int l = 0; l < nl; l++) {
        FrameLevel &F = c->fs.lv[l];
        int *cc = c->work + cc_off[l];
        HIPCHK(c, launch_enlist_count(F.edge, 1, F.npx, F.depth, F.npx, ImgBatch{F.rows, F.cols, count}, cc,
                                      c->work + bc_off[l], c->stream, d_map));
        HIPCHK(c, hipMemcpy2DAsync(hN.data() + (size_t)l * count, sizeof(int), cc + F.cols, sizeof(int) * (F.cols + 2),
                                   sizeof(int), count, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, stream_wait(c->stream));
    int bad_level = -1, bad_frame = -1;
    for (int l = 0; l < nl; l++) {
        FrameLevel &F = c->fs.lv[l];
        int maxN = 0;
        for (int i = 0; i < count; i++) {
            const int N = hN[(size_t)l * count + i];
            maxN = std::max(maxN, N);
            if (N < 1 && bad_level < 0) { bad_level = l; bad_frame = i; }
            if (N_out) N_out[(size_t)i * nl + l] = N;
        }
        if ((rc = ensure_points(c, l, std::max(maxN, 1)))) return rc;
        Level &L = c->lv[l];
        HIPCHK(c, launch_enlist_write(F.edge, 1, F.npx, F.depth, F.npx, ImgBatch{F.rows, F.cols, count}, l, c->K,
                                      c->work + cc_off[l], c->work + bc_off[l], L.pts, (size_t)L.pt_cap * 3,
                                      L.cpts, L.cidx, nullptr, L.pt_cap, L.dN, c->stream, d_map));
        HIPCHK(c, launch_points4_build_list(L.cpts, L.dN, L.pt_cap, F.rows, L.cpt4, L.chdr, L.d_pt4_ok, d_map, count, c->stream));
        for (int i = 0; i < count; i++) {
            const int p = h_pairs[i];
            L.hN.w(p) = hN[(size_t)l * count + i];
            L.compact_ok.w(p) = 1;
            ref_list_written(c, l, p, 1, F.rows);
        }
    }
    if (bad_level >= 0)
        return fail(c, DVO_ERR_INVALID, "no reference point selected in frame " + std::to_string(h_slots[bad_frame]) +
                                            " level " + std::to_string(bad_level) +
                                            " (reference asserts nSelectedPts > 0, SolveDVO.cpp:282)");
    return DVO_OK;
}

/* ---- per-pair undistortion (the tracker's per-stream calibration) ------------------------------------------------------------ */
int dvo_host::pair_umap_tables_upload(dvo_ctx *c) {
    if (c->pair_umap.empty()) return DVO_OK;
    const size_t n = (size_t)c->n_pairs;
    if (!c->d_umap_xy_tab) {
        HIPCHK(c, c->d_umap_frac_tab.alloc(n));
        HIPCHK(c, c->d_umap_xy_tab.alloc(n));             /* last: the test for both */
    }
    std::vector<const short2 *> xy(n);
    std::vector<const unsigned short *> fr(n);
    for (size_t p = 0; p < n; p++) pair_umap_of(c, (int)p, xy[p], fr[p]);
    HIPCHK(c, stream_wait(c->stream));                 /* no launch in flight reads the old tables */
    HIPCHK(c, hipMemcpy(c->d_umap_xy_tab, xy.data(), sizeof(short2 *) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_umap_frac_tab, fr.data(), sizeof(unsigned short *) * n, hipMemcpyHostToDevice));
    return DVO_OK;
}

int dvo_host::pair_undistort_set(dvo_ctx *c, int pair, int mode, int rows, int cols, const double *K4, const double *D5) {
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    if (mode == 1 && !calibration_ok(rows, cols, K4, D5))
        return fail(c, DVO_ERR_INVALID, "bad calibration (K4 and D5 finite, fx and fy not zero, rows and cols positive)");
    if (mode < 0 && c->pair_umap.empty()) return DVO_OK;          /* every pair follows the context's map already */
    HIPCHK(c, stream_wait(c->stream));
    int id = mode < 0 ? -1 : 0;
    if (mode == 1) {                                   /* one device map per distinct calibration: dedupe by value */
        double key[9];
        for (int k = 0; k < 4; k++) key[k] = K4[k];
        for (int k = 0; k < 5; k++) key[4 + k] = D5[k];
        for (size_t m = 0; m < c->umaps.size() && id == 0; m++) {
            const dvo_ctx::UMap &U = c->umaps[m];
            bool same = U.users > 0 && U.rows == rows && U.cols == cols;
            for (int k = 0; k < 9 && same; k++) same = U.key[k] == key[k];
            if (same) id = (int)m + 1;
        }
        if (id == 0) {
            dvo_ctx::UMap U;
            std::memcpy(U.key, key, sizeof(key));
            U.rows = rows; U.cols = cols;
            const int rc = build_undistort_map(c, rows, cols, K4, D5, U.xy, U.frac);
            if (rc) return rc;
            size_t m = 0;
            while (m < c->umaps.size() && c->umaps[m].users > 0) m++;       /* a free slot, or a new one */
            if (m == c->umaps.size()) c->umaps.push_back(std::move(U)); else c->umaps[m] = std::move(U);
            id = (int)m + 1;
        }
    }
    if (c->pair_umap.empty()) c->pair_umap.assign(c->n_pairs, -1);
    const int old = c->pair_umap[pair];
    if (id > 0) c->umaps[id - 1].users++;
    c->pair_umap[pair] = id;
    if (old > 0 && --c->umaps[old - 1].users == 0) c->umaps[old - 1] = dvo_ctx::UMap();      /* its last user changed: the map goes */
    return pair_umap_tables_upload(c);
}

extern "C" {

int dvo_frame_get_level(dvo_ctx *c, int slot, int level, int *rows, int *cols, unsigned char *grey,
                        float *depth_mm, unsigned char *edge, int *n_edges) {
    DVO_ENTER(c);
    if (level < 0 || level >= c->fs.n_levels) return fail(c, DVO_ERR_INVALID, "frame level out of range");
    if (!slots_ok(c, slot, 1) || !c->fs.valid[slot]) return fail(c, DVO_ERR_STATE, "frame slot holds no frame");
    FrameLevel &F = c->fs.lv[level];
    if (rows) *rows = F.rows;
    if (cols) *cols = F.cols;
    const size_t off = (size_t)slot * F.npx;
    if (grey) HIPCHK(c, hipMemcpyAsync(grey, F.grey + off, F.npx, hipMemcpyDeviceToHost, c->stream));
    if (edge) HIPCHK(c, hipMemcpyAsync(edge, F.edge + off, F.npx, hipMemcpyDeviceToHost, c->stream));
    if (depth_mm) {
        if (!c->fs.has_depth[slot]) return fail(c, DVO_ERR_STATE, "frame slot has no depth");
        HIPCHK(c, hipMemcpyAsync(depth_mm, F.depth + off, sizeof(float) * F.npx, hipMemcpyDeviceToHost, c->stream));
    }
    if (n_edges) {
        int rc = ensure_work(c, sizeof(int));
        if (rc) return rc;
        HIPCHK(c, launch_count_edges(F.edge + off, F.npx, c->work, c->stream));
        HIPCHK(c, hipMemcpyAsync(n_edges, c->work, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    /* round 6: a question about the level's size alone touches no device memory and must not wait for the stream (the Python binding asks
     * after every upload: four host syncs per step of a frames -> poses pipeline, 45 us of idle GPU in front of every alignment) */
    if (grey || edge || depth_mm || n_edges) HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

}  // extern "C"
