/*
 * dvo_capi_photo_streams.cpp -- many camera streams on the photometric engine (include/dvo_amd.h, "many camera streams on the
 * photometric engine"): K streams, each following RGBDOdometry::processFrame (src/RGBDOdometry.cpp:146-163) as dvo_amd::RGBDOdometry
 * does for one camera, advanced together by the index-list forms of the dvo_photo.hip kernels.  Host side only.
 */
#include <algorithm>
#include <array>

#include "dvo_ctx.h"

using namespace dvo;
using namespace dvo_host;

namespace {
constexpr int kLevels = 4;            /* the node's pyramid: 1, 1/2, 1/4, 1/8 of the full frame (:316-318) */
}

struct dvo_photo_streams {
    dvo_ctx *ctx = nullptr;
    int K = 0;
    dvo_photo_streams_params prm{};
    int lr[kLevels] = {}, lc[kLevels] = {};             /* level geometry */
    struct Lvl {                                         /* per-stream slabs of one level (stream s at offset s * stride) */
        DevBuf<double> J, zref, A;
        DevBuf<int> sel, n, work;
        DevBuf<float> gref;
        int cap = 0;
        size_t work_stride = 0;
    } lv[kLevels];
    struct Stream {
        long n_frame = 0;                                /* nFrame of the node */
        bool has_ref = false;
        int n[kLevels] = {};                             /* rows of J of the current reference */
        double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   /* the last T (what a refused frame reports) */
    };
    std::vector<Stream> st;
    DevBuf<double> d_T;                                  /* K x 16: each stream's T between ticks (the warm start) */
    DevBuf<PhotoEntry> d_list; PinnedBuf<PhotoEntry> h_list;   /* 2K entries: the reference set | the accepted set; then K for Gauss-Newton */
    DevBuf<PhotoOut> d_out; PinnedBuf<PhotoOut> h_out;
    DevBuf<int> d_info; PinnedBuf<int> h_info;           /* K x DVO_LEVELS x {n, last pixel selected} */
    /* per-stream camera matrices: K x {fx, fy, cx, cy} (the handle's where a stream has none of its own); allocated at the first
     * dvo_photo_streams_set_stream_intrinsics, uploaded there -- NULL = every stream uses the handle's */
    DevBuf<double> d_cam;
    std::vector<double> h_cam;
    int s_launches = 0, s_syncs = 0, s_runs = 0, s_refs = 0, s_refused = 0;
    std::string err;
};

namespace {

int pfail(dvo_photo_streams *h, int code, const std::string &msg) {
    h->err = msg;
    return code;
}
#define PSHIP(expr) DVO_HIP_CHECK(pfail, h, expr, #expr)

int level_size(int n, int shift) {                     /* INTER_NEAREST resize by 2^-shift: cvRound, half to even */
    return (int)std::nearbyint(std::ldexp((double)n, -shift));
}

PhotoLevelSlab slab_of(const dvo_photo_streams *h, int l) {
    const dvo_photo_streams::Lvl &L = h->lv[l];
    const FrameLevel &F = h->ctx->fs.lv[l];
    PhotoLevelSlab s{};
    s.J = L.J; s.zref = L.zref; s.A = L.A; s.sel = L.sel; s.n = L.n; s.gref = L.gref; s.work = L.work;
    s.work_stride = L.work_stride; s.cap = L.cap;
    s.grey = F.grey; s.depth = F.depth; s.npx = F.npx; s.rows = F.rows; s.cols = F.cols;
    return s;
}

int check_params(const dvo_photo_streams_params &p, int max_streams, std::string &why) {
    const dvo_photo_params &q = p.photo;
    if (!(q.fx != 0.0) || !(q.fy != 0.0) || q.max_jacobian_size < 1 || q.iterations < 1 || q.iterations > 64)
        return why = "bad photometric parameters (fx, fy, max_jacobian_size, iterations)", DVO_ERR_INVALID;
    if (max_streams < 1 || max_streams > 65535) return why = "max_streams must be in [1, 65535]", DVO_ERR_INVALID;
    if (p.ref_every < 1) return why = "ref_every must be >= 1", DVO_ERR_INVALID;
    if (p.first_level < 0 || p.first_level >= kLevels) return why = "first_level out of range", DVO_ERR_INVALID;
    if (p.n_run < 1 || p.n_run > DVO_MAX_LEVELS) return why = "n_run must be in [1, DVO_MAX_LEVELS]", DVO_ERR_INVALID;
    if (p.n_run * q.iterations > 64) return why = "n_run * iterations exceeds 64", DVO_ERR_INVALID;
    for (int r = 0; r < p.n_run; r++)
        if (p.levels[r] < p.first_level || p.levels[r] >= kLevels)
            return why = "level " + std::to_string(p.levels[r]) + " has no Jacobian (levels must lie in [first_level, 4))", DVO_ERR_INVALID;
    if (p.rows < 1 || p.cols < 1) return why = "bad frame geometry", DVO_ERR_INVALID;
    for (int l = p.first_level; l < kLevels; l++) {
        const int r = level_size(p.rows, l), c = level_size(p.cols, l);
        if (r < 1 || c < 1) return why = "pyramid level would be empty", DVO_ERR_INVALID;
        if (r > 65535 || c > 32767) return why = "image too large for the photometric engine", DVO_ERR_INVALID;
    }
    return DVO_OK;
}

}  // namespace

extern "C" {

int dvo_photo_streams_params_default(dvo_photo_streams_params *p) {
    if (!p) return DVO_ERR_INVALID;
    std::memset(p, 0, sizeof(*p));
    dvo_photo_params_default(&p->photo);
    p->ref_every = 10000;               /* (nFrame % 10000) == 0, "renew ref-frame every 30 frames"   RGBDOdometry.cpp:146 */
    p->first_level = 1;                 /* computeJacobianAllLevels: levels 1..3                      :373 */
    p->n_run = 2;                       /* gaussNewtonIterations(3, T); gaussNewtonIterations(2, T)   :162-163 */
    p->levels[0] = 3;
    p->levels[1] = 2;
    p->rows = 480; p->cols = 640;
    return DVO_OK;
}

const char *dvo_photo_streams_last_error(const dvo_photo_streams *h) { return h ? h->err.c_str() : dvo_last_error(nullptr); }

int dvo_photo_streams_create(const dvo_photo_streams_params *pp, int max_streams, dvo_photo_streams **out) {
    if (!out) return fail(nullptr, DVO_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!pp) return fail(nullptr, DVO_ERR_INVALID, "params is NULL (dvo_photo_streams_params_default, then the camera matrix)");
    std::string why;
    int rc = check_params(*pp, max_streams, why);
    if (rc) return fail(nullptr, rc, why);
    dvo_ctx *c = nullptr;
    if ((rc = dvo_create(nullptr, &c))) return rc;
    dvo_photo_streams *h = new dvo_photo_streams();
    h->ctx = c;
    h->K = max_streams;
    h->prm = *pp;
    h->st.assign(max_streams, dvo_photo_streams::Stream());
    for (int l = 0; l < kLevels; l++) { h->lr[l] = level_size(pp->rows, l); h->lc[l] = level_size(pp->cols, l); }
    auto setup = [&]() -> int {
        DeviceGuard g(c);
        const size_t K = (size_t)max_streams;
        /* the slabs: checked against the free memory first, so that an oversized K fails cleanly */
        size_t bytes = 0;
        for (int l = pp->first_level; l < kLevels; l++) {
            dvo_photo_streams::Lvl &L = h->lv[l];
            L.cap = (int)std::min<long long>(pp->photo.max_jacobian_size, (long long)h->lr[l] * h->lc[l]);
            L.work_stride = 2 * ((size_t)h->lc[l] + 1);
            bytes += K * ((size_t)L.cap * (6 * sizeof(double) + sizeof(double) + sizeof(int) + sizeof(float)) + 36 * sizeof(double) +
                          sizeof(int) + L.work_stride * sizeof(int));
        }
        size_t free_b = 0, total_b = 0;
        PSHIP(hipMemGetInfo(&free_b, &total_b));
        if (bytes > free_b)
            return pfail(h, DVO_ERR_NOMEM, "the per-stream slabs need " + std::to_string(bytes >> 20) + " MiB, " + std::to_string(free_b >> 20) +
                                               " MiB are free (fewer streams, or a smaller max_jacobian_size)");
        for (int l = pp->first_level; l < kLevels; l++) {
            dvo_photo_streams::Lvl &L = h->lv[l];
            const size_t rows = K * (size_t)L.cap;
            PSHIP(L.J.alloc(6 * rows));
            PSHIP(L.zref.alloc(rows));
            PSHIP(L.sel.alloc(rows));
            PSHIP(L.gref.alloc(rows));
            PSHIP(L.A.alloc(36 * K));
            PSHIP(L.n.alloc(K));
            PSHIP(L.work.alloc(L.work_stride * K));
        }
        PSHIP(h->d_T.alloc(16 * K));
        PSHIP(h->d_list.alloc(3 * K));
        PSHIP(h->h_list.alloc(3 * K));
        PSHIP(h->d_out.alloc(K));
        PSHIP(h->h_out.alloc(K));
        PSHIP(h->d_info.alloc(2 * DVO_LEVELS * K));
        PSHIP(h->h_info.alloc(2 * DVO_LEVELS * K));
        const int frc = dvo_frames_reserve(c, max_streams);
        if (frc) return pfail(h, frc, c->err);
        PSHIP(stream_wait(c->stream));
        return DVO_OK;
    };
    rc = setup();
    if (rc) {
        fail(nullptr, rc, h->err);
        dvo_photo_streams_destroy(h);
        return rc;
    }
    *out = h;
    return DVO_OK;
}

int dvo_photo_streams_destroy(dvo_photo_streams *h) {
    if (!h) return DVO_ERR_INVALID;
    dvo_ctx *c = h->ctx;
    DeviceGuard g(c);
    if (c) (void)stream_wait(c->stream);
    delete h;               /* the handle's buffers go before its context's stream does */
    return dvo_destroy(c);
}

int dvo_photo_streams_reset_stream(dvo_photo_streams *h, int stream) {
    if (!h) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= h->K) return pfail(h, DVO_ERR_INVALID, "stream out of range");
    h->st[stream] = dvo_photo_streams::Stream();
    return DVO_OK;
}

int dvo_photo_streams_set_stream_intrinsics(dvo_photo_streams *h, int stream, double fx, double fy, double cx, double cy) {
    if (!h) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= h->K) return pfail(h, DVO_ERR_INVALID, "stream out of range");
    if (!(fx > 0.0) || !(fy > 0.0)) return pfail(h, DVO_ERR_INVALID, "fx, fy must be positive");
    const dvo_photo_streams::Stream &S = h->st[stream];
    if (S.n_frame != 0 || S.has_ref)                   /* the reference's Jacobians were computed with the old matrix */
        return pfail(h, DVO_ERR_STATE, "stream " + std::to_string(stream) + " is running: its camera matrix may change only before its first "
                                       "frame (dvo_photo_streams_reset_stream)");
    DeviceGuard g(h->ctx);
    PSHIP(stream_wait(h->ctx->stream));
    if (!h->d_cam) {
        PSHIP(h->d_cam.alloc(4 * (size_t)h->K));
        const dvo_photo_params &P = h->prm.photo;
        h->h_cam.resize(4 * (size_t)h->K);
        for (int s = 0; s < h->K; s++) { double *k = &h->h_cam[4 * (size_t)s]; k[0] = P.fx; k[1] = P.fy; k[2] = P.cx; k[3] = P.cy; }
    }
    double *k = &h->h_cam[4 * (size_t)stream];
    k[0] = fx; k[1] = fy; k[2] = cx; k[3] = cy;
    PSHIP(hipMemcpy(h->d_cam, h->h_cam.data(), sizeof(double) * h->h_cam.size(), hipMemcpyHostToDevice));
    return DVO_OK;
}

int dvo_photo_streams_step(dvo_photo_streams *h, int count, const int *streams, const unsigned char *const *bgr8, const float *const *depth,
                           int rows, int cols, int flags, double *T16_out, double *eps_norms, int *updates, int *event) {
    return dvo_photo_streams_step_fmt(h, count, streams, reinterpret_cast<const void *const *>(bgr8), DVO_CAM_BGR8,
                                      reinterpret_cast<const void *const *>(depth), DVO_DEPTH_F32, rows, cols, flags, T16_out, eps_norms,
                                      updates, event);
}

int dvo_photo_streams_step_fmt(dvo_photo_streams *h, int count, const int *streams, const void *const *bgr8, int image_format,
                               const void *const *depth, int depth_format, int rows, int cols, int flags, double *T16_out,
                               double *eps_norms, int *updates, int *event) {
    if (!h) return DVO_ERR_INVALID;
    /* refusals: nothing is changed before they pass */
    if (count < 1 || count > h->K) return pfail(h, DVO_ERR_INVALID, "count must be in [1, max_streams]");
    if (!streams || !bgr8 || !depth || !T16_out || !event) return pfail(h, DVO_ERR_INVALID, "NULL argument");
    if (image_format < DVO_CAM_BGR8 || image_format > DVO_CAM_MONO8 || depth_format < DVO_DEPTH_F32 || depth_format > DVO_DEPTH_U16)
        return pfail(h, DVO_ERR_INVALID, "unknown image or depth format (DVO_CAM_* / DVO_DEPTH_*)");
    if (rows != h->prm.rows || cols != h->prm.cols)
        return pfail(h, DVO_ERR_INVALID, "frame geometry differs from the handle's (dvo_photo_streams_params.rows / cols)");
    {
        std::vector<char> seen(h->K, 0);
        for (int i = 0; i < count; i++) {
            const int s = streams[i];
            if (s < 0 || s >= h->K) return pfail(h, DVO_ERR_INVALID, "stream " + std::to_string(s) + " out of range");
            if (seen[s]) return pfail(h, DVO_ERR_INVALID, "stream " + std::to_string(s) + " listed twice");
            seen[s] = 1;
            if (!bgr8[i] || !depth[i]) return pfail(h, DVO_ERR_INVALID, "NULL camera image");
        }
    }
    dvo_ctx *c = h->ctx;
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    h->s_runs = h->s_refs = h->s_refused = 0;
    const dvo_photo_params &P = h->prm.photo;
    const int K = h->K, fl = h->prm.first_level, it = P.iterations, n_run = h->prm.n_run;

    /* 1. frames: one batched upload per run of consecutive listed streams (slot = stream) */
    std::vector<int> order(count);
    for (int i = 0; i < count; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return streams[a] < streams[b]; });
    const int up_flags = (flags & (DVO_UPLOAD_DEVICE | DVO_UPLOAD_MAPPED | DVO_UPLOAD_DIRECT)) | DVO_UPLOAD_DEPTH_RAW | DVO_UPLOAD_ASYNC;
    std::vector<const void *> b(count), d(count);
    for (int a = 0; a < count;) {
        int e = a + 1;
        while (e < count && streams[order[e]] == streams[order[e - 1]] + 1) e++;
        for (int k = a; k < e; k++) { b[k - a] = bgr8[order[k]]; d[k - a] = depth[order[k]]; }
        h->s_runs++;
        const int rc = dvo_frames_upload_cameras_fmt(c, streams[order[a]], e - a, b.data(), image_format, d.data(), depth_format, rows, cols,
                                                     kLevels, 0, -1, up_flags);
        if (rc) return pfail(h, rc, c->err);
        a = e;
    }
    for (int l = fl; l < kLevels; l++)
        if (c->fs.lv[l].rows != h->lr[l] || c->fs.lv[l].cols != h->lc[l])
            return pfail(h, DVO_ERR_STATE, "the frame store's level " + std::to_string(l) + " differs from the handle's geometry");

    /* 2. reference ticks: select for all of them, one read, the rules of dvo_photo_set_ref per stream, fill for the accepted ones */
    std::vector<int> refset, accepted;                   /* indices into streams[], sorted by stream */
    std::vector<char> is_ref(count, 0), refused(count, 0);
    for (int i : order)
        if (h->st[streams[i]].n_frame % h->prm.ref_every == 0) { refset.push_back(i); is_ref[i] = 1; }
    const int nR = (int)refset.size();
    std::vector<std::array<int, kLevels>> n_new(count);
    if (nR > 0) {
        PhotoEntry *sl = h->h_list;
        for (int k = 0; k < nR; k++) sl[k] = PhotoEntry{streams[refset[k]], streams[refset[k]], 0, 0};
        PSHIP(hipMemcpyAsync(h->d_list, sl, sizeof(PhotoEntry) * nR, hipMemcpyHostToDevice, c->stream));
        for (int l = fl; l < kLevels; l++)
            PSHIP(launch_photo_select_list(h->d_list, nR, slab_of(h, l), l, (double)P.gradient_threshold, h->d_info, c->stream));
        PSHIP(hipMemcpyAsync(h->h_info, h->d_info, sizeof(int) * 2 * DVO_LEVELS * nR, hipMemcpyDeviceToHost, c->stream));
        PSHIP(stream_wait(c->stream));
        const int cap = P.max_jacobian_size;
        for (int k = 0; k < nR; k++) {
            bool ok = true;
            for (int l = fl; l < kLevels; l++) {
                const int n = h->h_info[(k * DVO_LEVELS + l) * 2], last = h->h_info[(k * DVO_LEVELS + l) * 2 + 1];
                n_new[refset[k]][l] = n;
                /* RGBDOdometry.cpp:464 asserts xc < const_maxJacobianSize before every scanned pixel, :500 asserts xc > min */
                if (n > cap || (n == cap && !last) || n <= P.min_required_pts) ok = false;
            }
            if (ok) accepted.push_back(refset[k]);
            else refused[refset[k]] = 1;
        }
        const int nA = (int)accepted.size();
        if (nA > 0) {
            PhotoEntry *al = h->h_list + K;
            for (int k = 0; k < nA; k++) al[k] = PhotoEntry{streams[accepted[k]], streams[accepted[k]], 0, 0};
            PSHIP(hipMemcpyAsync(h->d_list + K, al, sizeof(PhotoEntry) * nA, hipMemcpyHostToDevice, c->stream));
            for (int l = fl; l < kLevels; l++)
                PSHIP(launch_photo_fill_list(h->d_list + K, nA, slab_of(h, l), l, P.fx, P.fy, P.cx, P.cy, P.fixed, (double)P.gradient_threshold,
                                             c->stream, h->d_cam));
        }
    }

    /* 3. ONE Gauss-Newton launch for every listed stream that has a reference now; 4. ONE read */
    std::vector<int> gn;                                 /* indices into streams[] */
    for (int i : order) {
        if (refused[i]) continue;
        if (is_ref[i] || h->st[streams[i]].has_ref) gn.push_back(i);
    }
    const int nG = (int)gn.size();
    if (nG > 0) {
        PhotoEntry *gl = h->h_list + 2 * K;
        for (int k = 0; k < nG; k++) gl[k] = PhotoEntry{streams[gn[k]], streams[gn[k]], is_ref[gn[k]] ? 1 : 0, 0};
        PSHIP(hipMemcpyAsync(h->d_list + 2 * K, gl, sizeof(PhotoEntry) * nG, hipMemcpyHostToDevice, c->stream));
        PhotoSlabs S{};
        for (int l = fl; l < kLevels; l++) S.l[l] = slab_of(h, l);
        PhotoRun run{};
        run.n_run = n_run;
        for (int r = 0; r < n_run; r++) run.levels[r] = h->prm.levels[r];
        PSHIP(launch_photo_gauss_newton_list(h->d_list + 2 * K, nG, S, run, P.fx, P.fy, P.cx, P.cy, P.fixed, it, P.eps_norm_stop, h->d_T,
                                             h->d_out, c->stream, h->d_cam));
        PSHIP(hipMemcpyAsync(h->h_out, h->d_out, sizeof(PhotoOut) * nG, hipMemcpyDeviceToHost, c->stream));
    }
    PSHIP(stream_wait(c->stream));                       /* also the end of the borrowing of the caller's frame buffers */

    /* 5. outputs and the streams' state */
    for (int i = 0; i < count; i++) {
        event[i] = -1;
        if (eps_norms) for (int k = 0; k < n_run * it; k++) eps_norms[(size_t)i * n_run * it + k] = -1.0;
        if (updates) for (int r = 0; r < n_run; r++) updates[(size_t)i * n_run + r] = 0;
        std::memcpy(T16_out + 16 * (size_t)i, h->st[streams[i]].T, sizeof(double) * 16);
    }
    for (int k = 0; k < nG; k++) {
        const int i = gn[k];
        dvo_photo_streams::Stream &S = h->st[streams[i]];
        const PhotoOut &o = h->h_out[k];
        std::memcpy(S.T, o.T, sizeof(double) * 16);
        std::memcpy(T16_out + 16 * (size_t)i, o.T, sizeof(double) * 16);
        if (eps_norms) std::memcpy(eps_norms + (size_t)i * n_run * it, o.norms, sizeof(double) * n_run * it);
        if (updates) for (int r = 0; r < n_run; r++) updates[(size_t)i * n_run + r] = o.updates[r];
        event[i] = is_ref[i] ? 1 : 0;
        if (is_ref[i]) {
            S.has_ref = true;
            for (int l = fl; l < kLevels; l++) S.n[l] = n_new[i][l];
            h->s_refs++;
        }
        S.n_frame++;
    }
    for (int i = 0; i < count; i++) h->s_refused += refused[i];
    h->s_launches = (int)(g_kernel_launches - launches0);
    h->s_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_photo_streams_get_jacobian(dvo_photo_streams *h, int stream, int level, double *J, int *sel_i, int *sel_j, int capacity,
                                   double *A36, int *n_out) {
    if (!h) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= h->K) return pfail(h, DVO_ERR_INVALID, "stream out of range");
    const dvo_photo_streams::Stream &S = h->st[stream];
    if (!S.has_ref || level < h->prm.first_level || level >= kLevels)
        return pfail(h, DVO_ERR_STATE, "no Jacobian for this stream and level");
    DeviceGuard g(h->ctx);
    const dvo_photo_streams::Lvl &L = h->lv[level];
    PSHIP(stream_wait(h->ctx->stream));
    const int n = std::min(S.n[level], std::max(capacity, 0));
    const size_t r0 = (size_t)stream * L.cap;
    if (n_out) *n_out = S.n[level];
    if (J && n > 0) PSHIP(hipMemcpy(J, L.J + r0 * 6, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost));
    if ((sel_i || sel_j) && n > 0) {
        std::vector<int> s(n);
        PSHIP(hipMemcpy(s.data(), L.sel + r0, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        for (int k = 0; k < n; k++) { if (sel_i) sel_i[k] = s[k] & 0xffff; if (sel_j) sel_j[k] = s[k] >> 16; }
    }
    if (A36) PSHIP(hipMemcpy(A36, L.A + (size_t)stream * 36, sizeof(double) * 36, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_photo_streams_get_stats(dvo_photo_streams *h, int *kernel_launches, int *host_syncs, int *runs, int *ref_events, int *refused) {
    if (!h) return DVO_ERR_INVALID;
    if (kernel_launches) *kernel_launches = h->s_launches;
    if (host_syncs) *host_syncs = h->s_syncs;
    if (runs) *runs = h->s_runs;
    if (ref_events) *ref_events = h->s_refs;
    if (refused) *refused = h->s_refused;
    return DVO_OK;
}

dvo_ctx *dvo_photo_streams_context(dvo_photo_streams *h) { return h ? h->ctx : nullptr; }

}  // extern "C"
