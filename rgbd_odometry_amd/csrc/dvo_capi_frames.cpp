/*
 * dvo_capi_frames.cpp -- the frame-store half of the C ABI (include/dvo_amd.h, "frames in"): SURVEY.md section 8f rows
 * f1 + f2.  Host side only: slabs, uploads (double-buffered landing buffers, two copy streams, pinned mirror for small
 * images), kernel launches of dvo_frames.hip.  No CPU compute path.
 */
#include "dvo_ctx.h"
#include "dvo_mask_levels.h"
#include "dvo_upload_plan.h"
#include <chrono>
#include <cstdio>

using namespace dvo;
using namespace dvo_host;

static_assert(PLAN_LEVELS == DVO_LEVELS, "dvo_upload_plan.h mirrors DVO_LEVELS of dvo_launch.h");

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

void canny_thresholds(const dvo_ctx *c, int *low, int *high) {
    double t1 = c->prm.canny_threshold1, t2 = c->prm.canny_threshold2;
    if (t1 == 0 && t2 == 0) { t1 = 150; t2 = 100; }               /* SolveDVO.cpp:1704, :1764 */
    double lo = std::min(t1, t2), hi = std::max(t1, t2);          /* the detector swaps them */
    lo = std::min(32767.0, lo); hi = std::min(32767.0, hi);
    if (lo > 0) lo *= lo;                                         /* L2gradient: squared magnitudes */
    if (hi > 0) hi *= hi;
    *low = (int)std::floor(lo); *high = (int)std::floor(hi);
}

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
        S.n_slots = frames_default_slots(c->n_pairs);
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

/* the store's levels as the arrays the all-level launches take; the edge maps from slot `first_slot` on */
struct LevelView {
    int rows[DVO_LEVELS], cols[DVO_LEVELS];
    unsigned char *edge[DVO_LEVELS];
    size_t estride[DVO_LEVELS];
};
LevelView level_view(const dvo_ctx *c, int n_levels, int first_slot) {
    LevelView v;
    for (int l = 0; l < n_levels; l++) {
        const FrameLevel &F = c->fs.lv[l];
        v.rows[l] = F.rows; v.cols[l] = F.cols; v.estride[l] = F.npx; v.edge[l] = F.edge + (size_t)first_slot * F.npx;
    }
    return v;
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
    const LevelView v = level_view(c, n_levels, first_slot);
    if (!canny_levels_ok(n_levels, v.rows, v.cols, v.edge, v.estride)) {
        for (int l = 0; l < n_levels; l++) { const int rc = run_canny(c, l, first_slot, count, stream); if (rc) return rc; }
        return DVO_OK;
    }
    int low, high;
    canny_thresholds(c, &low, &high);
    const int chunk = chunk_for(sizeof(int) * canny_levels_work_ints(n_levels, v.rows, v.cols, 1), count);
    int rc = ensure_work(c, sizeof(int) * canny_levels_work_ints(n_levels, v.rows, v.cols, chunk));
    if (rc) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b);
        const LevelView vb = level_view(c, n_levels, first_slot + b);
        const unsigned char *grey[DVO_LEVELS];
        for (int l = 0; l < n_levels; l++) grey[l] = c->fs.lv[l].grey + (size_t)(first_slot + b) * c->fs.lv[l].npx;
        HIPCHK(c, launch_canny_levels(n_levels, v.rows, v.cols, grey, v.estride, vb.edge, v.estride, nc, low, high, c->work, stream));
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
    const LevelView v = level_view(c, n_levels, first_slot);
    HIPCHK(c, launch_edge_mask_levels(n_levels, v.rows, v.cols, v.edge, v.estride, count, c->d_mask_tab + (size_t)first_pair * DVO_LEVELS, stream));
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

/* landing buffers of at least `bytes` each (+ their pinned mirrors when the sources are host buffers) + copy streams + events */
int ensure_upload(dvo_ctx *c, size_t bytes, bool mirrors) {
    HIPCHK(c, c->upload.create());
    HIPCHK(c, c->upload.grow(bytes, mirrors, [c] { return stream_wait(c->stream); }));
    return DVO_OK;
}

int frames_as_now_all(dvo_ctx *c, int n_levels, int first_slot, int first_pair, int count, hipStream_t stream);

/* the tail of a chunk of either upload, once its frames' grey and depth levels are in the store: Canny of all levels, the
 * ignore masks and the now levels of the pairs they belong to (now_first_pair < 0: nobody's) */
int chunk_tail(dvo_ctx *c, int n_levels, int first_slot, int now_first_pair, int count) {
    int rc;
    if ((rc = run_canny_all(c, n_levels, first_slot, count, c->stream))) return rc;      /* one launch per stage for all levels */
    if (now_first_pair < 0) return DVO_OK;
    if ((rc = run_edge_masks(c, n_levels, first_slot, now_first_pair, count, c->stream))) return rc;
    return frames_as_now_all(c, n_levels, first_slot, now_first_pair, count, c->stream);
}
/* ... and of the call */
int upload_finish(dvo_ctx *c, int first_slot, int count, bool has_depth, int flags) {
    for (int f = 0; f < count; f++) { c->fs.valid[first_slot + f] = 1; c->fs.has_depth[first_slot + f] = has_depth ? 1 : 0; }
    if (!(flags & DVO_UPLOAD_ASYNC)) HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

int mask_refusal(dvo_ctx *c, int pair) {
    return fail(c, DVO_ERR_INVALID, "pair " + std::to_string(pair) + "'s ignore mask was built for another level geometry (dvo_frames_set_pair_mask)");
}

/* ---- dvo_frames_upload_pyramids: a chunk's copies into landing buffer `ub`, then its imports into the store ---- */
struct PyramidCall { int first_slot, count, n_levels; const dvo_image *grey, *depth; };

int pyramid_copy(dvo_ctx *c, const PyramidCall &A, const PyramidPlan &P, int b, int nc, int ub) {
    UploadRing &R = c->upload;
    unsigned char *buf = R.landing(ub), *hbuf = R.mirror(ub);
    const int n_levels = A.n_levels;
    if (P.mirror) HIPCHK(c, R.mirror_free(ub));
    std::vector<const void *> srcs(nc);
    for (int l = 0; l < n_levels; l++) {
        const size_t npx = c->fs.lv[l].npx, gb = npx * pix_bytes(A.grey[l].dtype), db = A.depth ? npx * pix_bytes(A.depth[l].dtype) : 0;
        if (P.mapped) {         /* one gather launch per level and 32 images, grey and depth on the two copy streams */
            const int wgs = mapped_gather_wgs(nc);
            for (int i = 0; i < nc; i++) srcs[i] = A.grey[(size_t)(b + i) * n_levels + l].data;
            HIPCHK(c, launch_gather_images(srcs.data(), nc, buf + P.g_off[l], gb, P.g_img[l], R.copy_stream(0), wgs));
            if (A.depth) {
                for (int i = 0; i < nc; i++) srcs[i] = A.depth[(size_t)(b + i) * n_levels + l].data;
                HIPCHK(c, launch_gather_images(srcs.data(), nc, buf + P.d_off[l], db, P.d_img[l], R.copy_stream(1), wgs));
            }
            continue;
        }
        for (int i = 0; i < nc; i++) {
            const void *gsrc = A.grey[(size_t)(b + i) * n_levels + l].data;
            const void *dsrc = A.depth ? A.depth[(size_t)(b + i) * n_levels + l].data : nullptr;
            if (P.small[l]) {
                std::memcpy(hbuf + P.g_off[l] + P.g_img[l] * i, gsrc, gb);
                if (A.depth) std::memcpy(hbuf + P.d_off[l] + P.d_img[l] * i, dsrc, db);
            } else {
                hipStream_t cs = R.copy_stream(i & 1);
                HIPCHK(c, hipMemcpyAsync(buf + P.g_off[l] + P.g_img[l] * i, gsrc, gb, hipMemcpyHostToDevice, cs));
                if (A.depth) HIPCHK(c, hipMemcpyAsync(buf + P.d_off[l] + P.d_img[l] * i, dsrc, db, hipMemcpyHostToDevice, cs));
            }
        }
    }
    for (int r = 0; r < P.n_runs; r++)                                  /* one copy per maximal run of small levels */
        HIPCHK(c, hipMemcpyAsync(buf + P.run_lo[r], hbuf + P.run_lo[r], P.run_hi[r] - P.run_lo[r], hipMemcpyHostToDevice, R.copy_stream(0)));
    return DVO_OK;
}

int pyramid_import(dvo_ctx *c, const PyramidCall &A, const PyramidPlan &P, int b, int nc, int ub) {
    const unsigned char *buf = c->upload.landing(ub);
    for (int l = 0; l < A.n_levels; l++) {
        FrameLevel &F = c->fs.lv[l];
        const size_t off = (size_t)(A.first_slot + b) * F.npx;
        const ImgBatch ib{F.rows, F.cols, nc};
        HIPCHK(c, launch_import_grey(buf + P.g_off[l], A.grey[l].dtype, A.grey[l].layout == DVO_LAYOUT_ROW_MAJOR,
                                     P.g_img[l] / pix_bytes(A.grey[l].dtype), F.grey + off, F.npx, ib, c->stream));
        if (A.depth)
            HIPCHK(c, launch_import_depth(buf + P.d_off[l], A.depth[l].dtype, A.depth[l].layout == DVO_LAYOUT_ROW_MAJOR,
                                          P.d_img[l] / pix_bytes(A.depth[l].dtype), F.depth + off, F.npx, ib, c->stream));
    }
    return DVO_OK;
}

}  // namespace

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
    /* validate: every refusal comes before frames_geometry, which drops the stored frames when the geometry changes */
    PyramidFacts f;
    f.first_slot = first_slot; f.count = count; f.n_levels = n_levels; f.has_grey = grey != nullptr; f.has_depth = depth != nullptr;
    f.flags = flags; f.now_first_pair = now_first_pair; f.n_pairs = c->n_pairs; f.n_slots = c->fs.n_slots;
    for (int l = 0; grey && l < std::min(std::max(n_levels, 0), DVO_LEVELS); l++) {
        f.rows[l] = grey[l].rows; f.cols[l] = grey[l].cols; f.grey_dtype[l] = grey[l].dtype;
        if (depth) f.depth_dtype[l] = depth[l].dtype;
    }
    const PyramidPlan plan = plan_pyramid_upload(f);
    if (plan.err && !plan.late) return fail(c, plan.err, plan.msg);
    const int *rows = f.rows, *cols = f.cols;
    for (int i = 0; i < count; i++)
        for (int l = 0; l < n_levels; l++) {
            const dvo_image &g = grey[(size_t)i * n_levels + l];
            if (!g.data || g.rows < 1 || g.cols < 1 || g.rows != rows[l] || g.cols != cols[l] ||
                (g.dtype != DVO_PIX_U8 && g.dtype != DVO_PIX_F32) || g.dtype != grey[l].dtype || g.layout != grey[l].layout)
                return fail(c, DVO_ERR_INVALID, "grey images of one level must share size, dtype (U8/F32) and layout");
            if (depth) {
                const dvo_image &d = depth[(size_t)i * n_levels + l];
                if (!d.data || d.rows != rows[l] || d.cols != cols[l] || (d.dtype != DVO_PIX_U16 && d.dtype != DVO_PIX_F32) ||
                    d.dtype != depth[l].dtype || d.layout != depth[l].layout)
                    return fail(c, DVO_ERR_INVALID, "depth images must match the grey size and share dtype (U16/F32) and layout");
            }
        }
    if (now_first_pair >= 0 && now_range_ok(now_first_pair, count, c->n_pairs)) {
        const int p = mask_geometry_mismatch(c, now_first_pair, count, n_levels, rows, cols);
        if (p >= 0) return mask_refusal(c, p);
    }
    if (plan.err) return fail(c, plan.err, plan.msg);
    /* reserve */
    int rc = frames_geometry(c, n_levels, rows, cols);
    if (rc) return rc;
    if ((rc = ensure_upload(c, plan.landing_bytes, plan.mirror))) return rc;
    /* chunks of frames flow through copy (copy streams) -> import + Canny (context stream), double-buffered */
    const PyramidCall A{first_slot, count, n_levels, grey, depth};
    for (int b = 0; b < count; b += plan.chunk) {
        const int nc = std::min(plan.chunk, count - b);
        int ub;
        HIPCHK(c, c->upload.acquire(&ub));
        if ((rc = pyramid_copy(c, A, plan, b, nc, ub))) return rc;
        if (now_first_pair >= 0 && (rc = ensure_now_texels(c, n_levels))) return rc;
        HIPCHK(c, c->upload.copied(ub));
        HIPCHK(c, c->upload.consumer_waits(ub, c->stream));
        if ((rc = pyramid_import(c, A, plan, b, nc, ub))) return rc;       /* all imports, then release the landing buffer, then the rest */
        HIPCHK(c, c->upload.consumed(ub, c->stream));
        if ((rc = chunk_tail(c, n_levels, first_slot + b, now_first_pair < 0 ? -1 : now_first_pair + b, nc))) return rc;
    }
    return upload_finish(c, first_slot, count, depth != nullptr, flags);
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

namespace {
/* ---- dvo_frames_upload_cameras_fmt: a chunk's copies into the next landing buffer, then its kernels ---- */
struct CameraCall {
    int first_slot, count;
    const void *const *img, *const *depth;
    int image_format, depth_format, rows, cols, n_levels, first_shift, now_first_pair, flags;
    bool per_pair_maps;
    SrcTab tab;                     /* read in place: the device table of the call's addresses */
};
struct Chunk { int b, nc, ub; unsigned char *sb, *sd; };      /* frames [b, b + nc); landing buffer ub (-1: none), its image and depth halves */

int camera_copy(dvo_ctx *c, const CameraCall &A, const CameraPlan &P, int b, Chunk &k) {
    k = Chunk{b, std::min(P.chunk, A.count - b), -1, nullptr, nullptr};
    if (P.route == ROUTE_IN_PLACE) return DVO_OK;
    UploadRing &R = c->upload;
    HIPCHK(c, R.acquire(&k.ub));
    k.sb = R.landing(k.ub); k.sd = k.sb + P.b_img * P.chunk;
    const size_t npx = (size_t)A.rows * A.cols;
    if (P.device_sources) {                                  /* device sources may be depth images a registration is still writing on the context stream */
        HIPCHK(c, depth_registered_ready(c, R.copy_stream(0)));
        HIPCHK(c, depth_registered_ready(c, R.copy_stream(1)));
    }
    if (P.route == ROUTE_GATHER) {                           /* in HBM already, or in pinned host memory the GPU addresses: gathered */
        const int wgs = P.gather_wgs(k.nc);
        HIPCHK(c, launch_gather_images(A.img + b, k.nc, k.sb, npx * P.bpp, P.b_img, R.copy_stream(0), wgs));
        if (A.depth) HIPCHK(c, launch_gather_images(A.depth + b, k.nc, k.sd, npx * P.dpp, P.d_img, R.copy_stream(1), wgs));
    } else if (P.route == ROUTE_DMA) {
        for (int i = 0; i < k.nc; i++) {
            hipStream_t cs = R.copy_stream(i & 1);
            HIPCHK(c, hipMemcpyAsync(k.sb + P.b_img * i, A.img[b + i], npx * P.bpp, hipMemcpyHostToDevice, cs));
            if (A.depth) HIPCHK(c, hipMemcpyAsync(k.sd + P.d_img * i, A.depth[b + i], npx * P.dpp, hipMemcpyHostToDevice, cs));
        }
    } else {
        /* through the engine's pinned mirror of the landing buffer: one memcpy per image on the host, then two DMAs per
         * chunk; the caller's (pageable) memory is never registered with the driver (include/dvo_amd.h, DVO_UPLOAD_DIRECT) */
        unsigned char *hb = R.mirror(k.ub);
        unsigned char *hd = hb + P.b_img * P.chunk;
        HIPCHK(c, R.mirror_free(k.ub));
        for (int i = 0; i < k.nc; i++) {
            std::memcpy(hb + P.b_img * i, A.img[b + i], npx * P.bpp);
            if (A.depth) std::memcpy(hd + P.d_img * i, A.depth[b + i], npx * P.dpp);
        }
        HIPCHK(c, hipMemcpyAsync(k.sb, hb, P.b_img * (size_t)k.nc, hipMemcpyHostToDevice, R.copy_stream(0)));
        if (A.depth) HIPCHK(c, hipMemcpyAsync(k.sd, hd, P.d_img * (size_t)k.nc, hipMemcpyHostToDevice, R.copy_stream(1)));
    }
    HIPCHK(c, R.copied(k.ub));                               /* the turn is committed per chunk: an error further down leaves events and turn consistent */
    return DVO_OK;
}

int camera_compute(dvo_ctx *c, const CameraCall &A, const CameraPlan &P, const Chunk &k) {
    int rc;
    const int n_levels = A.n_levels, depth_raw = (A.flags & DVO_UPLOAD_DEPTH_RAW) ? 1 : 0;
    const size_t slot0 = (size_t)(A.first_slot + k.b);
    if (A.now_first_pair >= 0 && (rc = ensure_now_texels(c, n_levels))) return rc;
    const bool in_place = P.route == ROUTE_IN_PLACE;
    const SrcTab tab = in_place ? SrcTab{A.tab.bgr + k.b, A.tab.depth ? A.tab.depth + k.b : nullptr} : SrcTab{nullptr, nullptr};
    const void *const dsrc = A.depth ? (in_place ? reinterpret_cast<const void *>(16) /* "has depth"; the table holds the addresses */ : k.sd) : nullptr;
    const CamSrc src{k.sb, P.b_img, A.image_format, dsrc, P.d_px, A.depth_format};
    if (k.ub >= 0) HIPCHK(c, c->upload.consumer_waits(k.ub, c->stream));
    /* undistortion: the context's map for every image, or -- per-pair calibration -- the one map all images of the chunk share, or
     * a table of the pairs' maps when they differ (the chunk stays one launch per stage) */
    const short2 *mxy = c->d_umap_xy;
    const unsigned short *mfr = c->d_umap_frac;
    UmapTab utab{nullptr, nullptr};
    if (A.per_pair_maps) {
        const int p0 = A.now_first_pair + k.b;
        pair_umap_of(c, p0, mxy, mfr);
        for (int i = 1; i < k.nc; i++) {
            const short2 *xy; const unsigned short *fr;
            pair_umap_of(c, p0 + i, xy, fr);
            if (xy != mxy) { utab = UmapTab{c->d_umap_xy_tab + p0, c->d_umap_frac_tab + p0}; mxy = nullptr; mfr = nullptr; break; }
        }
    }
    for (int l = 0; l < n_levels; l++) {
        FrameLevel &F = c->fs.lv[l];
        if (l == 0 || n_levels == 2)
            HIPCHK(c, launch_camera_level(src, A.rows, A.cols, A.first_shift + l, mxy, mfr, depth_raw, F.grey + slot0 * F.npx, F.depth + slot0 * F.npx,
                                          F.npx, ImgBatch{F.rows, F.cols, k.nc}, c->stream, tab, utab));
        else if (l == 1) {                               /* levels 1 .. n-1 in one launch */
            int sh[DVO_LEVELS], lr[DVO_LEVELS], lc[DVO_LEVELS]; unsigned char *gl[DVO_LEVELS]; float *dl[DVO_LEVELS]; size_t st[DVO_LEVELS];
            for (int m = 1; m < n_levels; m++) {
                FrameLevel &G = c->fs.lv[m];
                sh[m - 1] = A.first_shift + m; lr[m - 1] = G.rows; lc[m - 1] = G.cols; st[m - 1] = G.npx;
                gl[m - 1] = G.grey + slot0 * G.npx; dl[m - 1] = G.depth + slot0 * G.npx;
            }
            FrameLevel &F0 = c->fs.lv[0];
            if (camera_levels_decimate_ok(n_levels, P.rows, P.cols))      /* from level 0, written just before on this stream */
                HIPCHK(c, launch_camera_decimate_levels(F0.grey + slot0 * F0.npx, A.depth ? F0.depth + slot0 * F0.npx : nullptr,
                                                        F0.npx, F0.rows, F0.cols, n_levels - 1, lr, lc, gl, dl, st, k.nc, c->stream));
            else
                HIPCHK(c, launch_camera_levels(src, A.rows, A.cols, n_levels - 1, sh, lr, lc, mxy, mfr, depth_raw, gl, dl, st, k.nc, c->stream, tab, utab));
        }
    }
    if (k.ub >= 0) HIPCHK(c, c->upload.consumed(k.ub, c->stream));     /* the landing buffer is free again */
    return chunk_tail(c, n_levels, A.first_slot + k.b, A.now_first_pair < 0 ? -1 : A.now_first_pair + k.b, k.nc);
}
}  // namespace

/* bgr8 / depth_m: the images in their sensor formats (the names are those of the first format pair) */
int dvo_frames_upload_cameras_fmt(dvo_ctx *c, int first_slot, int count, const void *const *bgr8, int image_format,
                                  const void *const *depth_m, int depth_format, int rows, int cols, int n_levels, int first_shift,
                                  int now_first_pair, int flags) {
    DVO_ENTER(c);
    /* validate: every refusal comes before frames_geometry, which drops the stored frames when the geometry changes */
    CameraFacts f;
    f.first_slot = first_slot; f.count = count; f.rows = rows; f.cols = cols; f.n_levels = n_levels; f.first_shift = first_shift;
    f.image_format = image_format; f.depth_format = depth_format; f.has_images = bgr8 != nullptr; f.has_depth = depth_m != nullptr;
    f.flags = flags; f.now_first_pair = now_first_pair; f.n_pairs = c->n_pairs; f.n_slots = c->fs.n_slots;
    f.aligned = true;
    const size_t d_align = (depth_format == DVO_DEPTH_U16 ? 8 : 16) - 1;      /* the widest load of the level kernels: 4 * dpp bytes */
    for (int i = 0; bgr8 && i < count; i++) {
        f.null_image = f.null_image || !bgr8[i] || (depth_m && !depth_m[i]);
        f.aligned = f.aligned && (reinterpret_cast<size_t>(bgr8[i]) & 3) == 0 && (!depth_m || (reinterpret_cast<size_t>(depth_m[i]) & d_align) == 0);
    }
    const CameraPlan plan = plan_camera_upload(f);
    if (plan.err && !plan.late) return fail(c, plan.err, plan.msg);
    if (c->d_umap_xy && (c->umap_rows != rows || c->umap_cols != cols))
        return fail(c, DVO_ERR_INVALID, "the undistortion map was built for another image size (dvo_frames_set_undistort)");
    const bool per_pair_maps = now_first_pair >= 0 && !c->pair_umap.empty();
    if (per_pair_maps)
        for (int i = 0; i < count; i++) {
            const int m = c->pair_umap[now_first_pair + i];
            if (m > 0 && (c->umaps[m - 1].rows != rows || c->umaps[m - 1].cols != cols))
                return fail(c, DVO_ERR_INVALID, "pair " + std::to_string(now_first_pair + i) + "'s undistortion map was built for another image size");
        }
    if (now_first_pair >= 0) {
        const int p = mask_geometry_mismatch(c, now_first_pair, count, n_levels, plan.rows, plan.cols);
        if (p >= 0) return mask_refusal(c, p);
    }
    if (plan.err) return fail(c, plan.err, plan.msg);
    /* reserve */
    int rc = frames_geometry(c, n_levels, plan.rows, plan.cols);
    if (rc) return rc;
    CameraCall A{first_slot, count, bgr8, depth_m, image_format, depth_format, rows, cols, n_levels, first_shift, now_first_pair, flags,
                 per_pair_maps, SrcTab{nullptr, nullptr}};
    if (plan.route == ROUTE_IN_PLACE) {
        SourceTable &T = c->src_tab;
        HIPCHK(c, T.reserve((size_t)plan.table_entries, [c] { return stream_wait(c->stream); }));
        for (int i = 0; i < count; i++) {
            T.staging()[i] = const_cast<void *>(bgr8[i]);
            T.staging()[count + i] = depth_m ? const_cast<void *>(depth_m[i]) : nullptr;
        }
        HIPCHK(c, T.send((size_t)plan.table_entries, c->stream));
        A.tab = SrcTab{T.device(), depth_m ? T.device() + count : nullptr};
    } else if ((rc = ensure_upload(c, plan.landing_bytes, plan.mirror))) return rc;
    /* chunk k+1 is copied (copy streams) while chunk k is preprocessed (context stream), over two landing buffers.  The copies
     * of chunk k+1 are SUBMITTED before the kernels of chunk k where the plan says so: measured on this pool
     * (tools/experiments/exp_pull_overlap.sh), work of two streams that becomes ready at the same moment starts in submission
     * order, and a pull submitted after ~45 preprocessing launches waited for nearly all of them -- the link idled 0.6 ms of
     * every 1.6 (why DMA copies keep their place behind the compute: dvo_upload_plan.h, copies_ahead) */
    Chunk cur{}, nxt{};
    if ((rc = camera_copy(c, A, plan, 0, cur))) return rc;
    for (int b = 0; b < count; b += plan.chunk) {
        const bool more = b + plan.chunk < count;
        if (more && plan.copies_ahead && (rc = camera_copy(c, A, plan, b + plan.chunk, nxt))) return rc;
        if ((rc = camera_compute(c, A, plan, cur))) return rc;
        if (more && !plan.copies_ahead && (rc = camera_copy(c, A, plan, b + plan.chunk, nxt))) return rc;
        cur = nxt;
    }
    return upload_finish(c, first_slot, count, depth_m != nullptr, flags);
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

namespace {
/* Sparse texel slabs (dvo_ctx.h) under the compact form: the stage runs without texel output for them; the images the compact form
 * cannot hold get their texels mapped and written by a second run of the last pass -- per chunk, while the chunk's scratch still
 * holds them.  issue(second) enqueues the stage for levels [l0, l1) of pairs [pair0, pair0 + nc); now_tex gives it the texel output */
float4 *now_tex(const Level &L, bool compact, bool second, int pair0) {
    return (compact && L.tex_sparse && !second) ? nullptr : L.tex + (size_t)pair0 * L.tex_stride;
}
int issue_deferring_texels(dvo_ctx *c, int l0, int l1, bool compact, int pair0, int nc, hipStream_t stream, const std::function<int(bool)> &issue) {
    int rc, failed = 0;
    if ((rc = issue(false))) return rc;
    for (int l = l0; l < l1 && compact; l++) {
        if (!c->lv[l].tex_sparse) continue;
        int n_failed = 0;
        if ((rc = sparse_map_compact_failures(c, l, pair0, nc, stream, &n_failed))) return rc;
        failed += n_failed;
    }
    return failed ? issue(true) : DVO_OK;      /* only the pairs just mapped are written (pal_n < 0) */
}

int frames_as_now_level(dvo_ctx *c, int l, int first_slot, int first_pair, int count, hipStream_t stream) {
    int rc;
    FrameLevel &F = c->fs.lv[l];
    if ((rc = ensure_texels(c, l, F.rows, F.cols))) return rc;
    /* the now level is written in its compact form (dvo_palette.h) straight from the integer squared distances; 16-byte texels
     * only for images that form cannot hold, or when the caller switched the compact form off */
    const bool compact = native_compact_wanted(c);
    if (compact && (rc = ensure_compact_slabs(c, l))) return rc;
    Level &L = c->lv[l];
    if (L.tex_sparse && !compact && (rc = map_texels(c, l, first_pair, count, stream))) return rc;
    const int chunk = chunk_for(sizeof(int) * edt_work_ints(F.rows, F.cols, 1), count);
    if ((rc = ensure_work(c, sizeof(int) * edt_work_ints(F.rows, F.cols, chunk)))) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b), pair0 = first_pair + b;
        rc = issue_deferring_texels(c, l, l + 1, compact, pair0, nc, stream, [&](bool second) -> int {
            HIPCHK(c, launch_edges_to_now(F.edge + (size_t)(first_slot + b) * F.npx, F.npx, ImgBatch{F.rows, F.cols, nc}, c->work,
                                          now_tex(L, compact, second, pair0), L.tex_stride, compact ? L.p4.get() : nullptr, L.p4_stride, L.pal,
                                          L.d_pal_n, pair0, stream, second));
            return DVO_OK;
        });
        if (rc) return rc;
    }
    return compact ? now_written_compact(c, l, first_pair, count) : now_written(c, l, first_pair, count);
}

/* every level of `count` stored frames as now levels of pairs first_pair..: one launch per stage for all levels when the
 * geometry allows it (dvo_frames.hip, launch_edges_to_now_levels), else level by level */
int frames_as_now_all(dvo_ctx *c, int n_levels, int first_slot, int first_pair, int count, hipStream_t stream) {
    int rc;
    const LevelView v = level_view(c, n_levels, first_slot);
    if (!edt_levels_ok(n_levels, v.rows, v.cols)) {
        for (int l = 0; l < n_levels; l++)
            if ((rc = frames_as_now_level(c, l, first_slot, first_pair, count, stream))) return rc;
        return DVO_OK;
    }
    const bool compact = native_compact_wanted(c);
    for (int l = 0; l < n_levels; l++) {
        if ((rc = ensure_texels(c, l, v.rows[l], v.cols[l]))) return rc;
        if (compact && (rc = ensure_compact_slabs(c, l))) return rc;
    }
    /* Tried and dropped (round 4): the batch as two halves on two streams with their own scratch, so that the issue-bound row scan
     * of one half runs beside the memory-bound rank pack of the other -- 1.02-1.05 ms per 256 frames against 0.86 ms on one stream
     * (half-size launches fill the GPU less well, and work of two streams starts in submission order on this pool). */
    const int chunk = chunk_for(sizeof(int) * edt_levels_work_ints(n_levels, v.rows, v.cols, 1), count);
    if ((rc = ensure_work(c, sizeof(int) * edt_levels_work_ints(n_levels, v.rows, v.cols, chunk)))) return rc;
    for (int b = 0; b < count; b += chunk) {
        const int nc = std::min(chunk, count - b), pair0 = first_pair + b;
        const LevelView vb = level_view(c, n_levels, first_slot + b);
        size_t tstride[DVO_LEVELS], pstride[DVO_LEVELS];
        float4 *tex[DVO_LEVELS]; unsigned *p4[DVO_LEVELS]; float2 *pal[DVO_LEVELS]; int *pal_n[DVO_LEVELS];
        for (int l = 0; l < n_levels; l++) {
            Level &L = c->lv[l];
            if (L.tex_sparse && !compact && (rc = map_texels(c, l, pair0, nc, stream))) return rc;
            tstride[l] = L.tex_stride; p4[l] = compact ? L.p4.get() : nullptr; pstride[l] = L.p4_stride; pal[l] = L.pal; pal_n[l] = L.d_pal_n;
        }
        rc = issue_deferring_texels(c, 0, n_levels, compact, pair0, nc, stream, [&](bool second) -> int {
            for (int l = 0; l < n_levels; l++) tex[l] = now_tex(c->lv[l], compact, second, pair0);
            HIPCHK(c, launch_edges_to_now_levels(n_levels, v.rows, v.cols, vb.edge, v.estride, nc, c->work, tex, tstride, p4, pstride, pal, pal_n,
                                                 pair0, stream, second));
            return DVO_OK;
        });
        if (rc) return rc;
    }
    for (int l = 0; l < n_levels; l++)
        if ((rc = compact ? now_written_compact(c, l, first_pair, count) : now_written(c, l, first_pair, count))) return rc;
    return DVO_OK;
}
}  // namespace

int dvo_frames_as_now(dvo_ctx *c, int first_slot, int first_pair, int count) {
    DVO_ENTER(c);
    int rc = frames_check_use(c, first_slot, first_pair, count, false);
    if (rc) return rc;
    return frames_as_now_all(c, c->fs.n_levels, first_slot, first_pair, count, c->stream);
}

namespace {
/* which slot becomes the reference frame of which pair: image i of a contiguous range, or of a list (d_map[i] = {h_slots[i],
 * h_pairs[i]} on the device, for the launches in their index-list form) */
struct RefMap {
    int first_slot, first_pair;
    const int *h_slots, *h_pairs;
    const int2 *d_map;              /* NULL: the range */
    int slot(int i) const { return d_map ? h_slots[i] : first_slot + i; }
    int pair(int i) const { return d_map ? h_pairs[i] : first_pair + i; }
};

/* the edge points of `count` checked frames as reference lists: every stage one launch for the whole set, one host synchronisation
 * for the point counts.  The range form reaches its slots and pairs through pointer offsets, the list form through d_map */
int frames_as_ref_mapped(dvo_ctx *c, const RefMap &m, int count, int *N_out) {
    const int nl = c->fs.n_levels;
    const size_t slot0 = m.d_map ? 0 : (size_t)m.first_slot, pair0 = m.d_map ? 0 : (size_t)m.first_pair;
    size_t cc_off[DVO_LEVELS + 1];                      /* per level: count x (cols+2) column counters ... */
    size_t bc_off[DVO_LEVELS + 1];                      /* ... and count x enlist_block_ints() block-order counters */
    cc_off[0] = 0;
    for (int l = 0; l < nl; l++) cc_off[l + 1] = cc_off[l] + (size_t)count * (c->fs.lv[l].cols + 2);
    bc_off[0] = cc_off[nl];
    for (int l = 0; l < nl; l++) bc_off[l + 1] = bc_off[l] + (size_t)count * enlist_block_ints(c->fs.lv[l].rows, c->fs.lv[l].cols);
    int rc;
    if ((rc = ensure_work(c, sizeof(int) * bc_off[nl]))) return rc;
    std::vector<int> hN((size_t)count * nl);
    for (int l = 0; l < nl; l++) {
        FrameLevel &F = c->fs.lv[l];
        const size_t off = slot0 * F.npx;
        int *cc = c->work + cc_off[l];
        HIPCHK(c, launch_enlist_count(F.edge + off, 1, F.npx, F.depth + off, F.npx, ImgBatch{F.rows, F.cols, count}, cc,
                                      c->work + bc_off[l], c->stream, m.d_map));
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
        const size_t off = slot0 * F.npx;
        Intrinsics kb = c->K;                           /* the range form's kernel indexes the table by image: pair first_pair + image */
        if (kb.pair_K) kb.pair_K += pair0;
        HIPCHK(c, launch_enlist_write(F.edge + off, 1, F.npx, F.depth + off, F.npx, ImgBatch{F.rows, F.cols, count}, l, kb,
                                      c->work + cc_off[l], c->work + bc_off[l], L.pts + pair0 * L.pt_cap * 3, (size_t)L.pt_cap * 3,
                                      L.cpts + pair0 * L.pt_cap, L.cidx + pair0 * L.pt_cap, nullptr, L.pt_cap,
                                      L.dN + pair0, c->stream, m.d_map));
        if (m.d_map) HIPCHK(c, launch_points4_build_list(L.cpts, L.dN, L.pt_cap, F.rows, L.cpt4, L.chdr, L.d_pt4_ok, m.d_map, count, c->stream));
        else HIPCHK(c, launch_points4_build(L.cpts, L.dN, L.pt_cap, F.rows, L.cpt4, L.chdr, L.d_pt4_ok, m.first_pair, count, c->stream));
        for (int i = 0; i < count; i++) {
            L.hN.w(m.pair(i)) = hN[(size_t)l * count + i];
            L.compact_ok.w(m.pair(i)) = 1;
            if (m.d_map) ref_list_written(c, l, m.pair(i), 1, F.rows);
        }
        if (!m.d_map) ref_list_written(c, l, m.first_pair, count, F.rows);
    }
    if (bad_level >= 0)
        return fail(c, DVO_ERR_INVALID, "no reference point selected in frame " + std::to_string(m.slot(bad_frame)) +
                                            " level " + std::to_string(bad_level) +
                                            " (reference asserts nSelectedPts > 0, SolveDVO.cpp:282)");
    return DVO_OK;
}
}  // namespace

int dvo_frames_as_ref(dvo_ctx *c, int first_slot, int first_pair, int count, int *N_out) {
    DVO_ENTER(c);
    if (!c->have_K) return fail(c, DVO_ERR_STATE, "intrinsics not set (dvo_set_intrinsics)");
    int rc = frames_check_use(c, first_slot, first_pair, count, true);
    if (rc) return rc;
    return frames_as_ref_mapped(c, RefMap{first_slot, first_pair, nullptr, nullptr, nullptr}, count, N_out);
}

}  // extern "C"

/* dvo_frames_as_ref for any set: slot h_slots[i] becomes the reference frame of pair h_pairs[i], every stage one launch for the whole
 * set (enlist_count / _write and points4_build in their index-list form, d_map[i] = {h_slots[i], h_pairs[i]}) */
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
    return frames_as_ref_mapped(c, RefMap{0, 0, h_slots, h_pairs, d_map}, count, N_out);
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
