/*
 * dvo_capi_tracker.cpp -- the multi-stream tracker of the C ABI (include/dvo_amd.h, "many camera streams"): K camera streams,
 * each following SolveDVO::loop (SolveDVO.cpp:1970-2241) as dvo_amd::SolveDVO does for one camera, advanced together by
 * batched calls of the frame store and the fused alignment.  Host side only; the key-frame rule and the pose gather run in
 * dvo_tracker.hip.
 */
#include "dvo_archive_blob.h"
#include "dvo_ctx.h"
#include "dvo_depth_register.h"
#include "dvo_place_guess.h"

using namespace dvo;
using namespace dvo_host;

struct dvo_tracker {
    dvo_ctx *ctx = nullptr;
    int K = 0;
    dvo_tracker_params tp{};
    int n_levels = 0, last_level = 0;
    int lr[DVO_LEVELS] = {}, lc[DVO_LEVELS] = {};         /* level geometry */
    struct Stream {
        bool started = false;
        long n_frame = 0, last_ref = 0;                    /* nFrame / lastRefFrame of SolveDVO::loop */
        int bank = -1;                                     /* bank of the stream's latest frame: slot bank * K + stream */
        bool have_signals = false;
        float b_cap = 0.0f, ratio = 0.0f;
        int n_points = 0;
        bool have_info = false;                            /* info describes the pose the stream's last step returned */
        TrackerInfo info{};
        bool have_views = false;                           /* the stream's images and vrec show the pose its last step returned */
        TrackerViewRecord vrec{};
    };
    std::vector<Stream> st;
    DevBuf<TrackerEntry> d_list; PinnedBuf<TrackerEntry> h_list;
    DevBuf<TrackerOut> d_out; PinnedBuf<TrackerOut> h_out;       /* K entries + one slot for the team-mode error word */
    DevBuf<int> d_pairs; PinnedBuf<int> h_pairs;           /* index lists of the alignment launches: aligned streams, then switching ones */
    DevBuf<int2> d_map; PinnedBuf<int2> h_map;             /* {slot, pair} of the reference extractions: first frames, then switches */
    DevBuf<float> d_scratch;
    bool info_on = false;                                  /* dvo_tracker_set_information */
    DevBuf<TrackerInfo> d_info; PinnedBuf<TrackerInfo> h_info;   /* one record per listed stream, beside d_out / h_out; allocated when first switched on */
    bool views_on = false;                                 /* dvo_tracker_set_views; everything below is allocated when first switched on */
    DevBuf<unsigned char> d_views;                         /* 2 planes of K images: view v of stream p at d_views + (v * K + p) * view_stride */
    size_t view_stride = 0;                                /* rows * cols * 3 of the finest running level, rounded up to 256 bytes */
    DevBuf<TrackerViewRecord> d_vrec; PinnedBuf<TrackerViewRecord> h_vrec;   /* one record per listed stream, like d_info / h_info */
    DevBuf<int> d_vslot; PinnedBuf<int> h_vslot;           /* per listed stream: the frame store slot its frame went to in this step */
    int s_launches = 0, s_syncs = 0, s_runs = 0, s_keys = 0, s_growths = 0;
    /* dvo_tracker_set_stream_depth_rig / dvo_tracker_step_raw_depth; nothing of it exists in a tracker that never got a rig.  Host colour
     * images are staged here (stream s at s * col_stride, through the pinned mirror) so that the upload reads both sources in place */
    std::vector<char> has_rig;
    DevBuf<unsigned char> d_col; PinnedBuf<unsigned char> h_col;
    size_t col_stride = 0;
    hipEvent_t ev_col = nullptr;                           /* the last staging copy has left h_col */
    bool ev_col_pending = false;
    /* dvo_tracker_set_archive: the ring of key frames in HBM (dvo_tracker_archive.hip) and the private context dvo_tracker_match aligns in.
     * Everything below is allocated when the archive is switched on */
    struct Archive {
        bool on = false;
        int capacity = 0, max_matches = 0;
        int cap[DVO_LEVELS] = {};                          /* points per slot and level, multiples of 64 */
        ArchiveView view{};                                /* the kernels' argument: filled once from the buffers below */
        struct LevelBufs { DevBuf<uint2> cpts; DevBuf<unsigned> cidx, cpt4, chdr; } lb[DVO_LEVELS];
        DevBuf<ArchiveHeader> hdr;
        struct Meta {                                      /* what the host knows of a slot */
            long long id = -1;
            int stream = -1;
            long frame = 0;
            int N[DVO_LEVELS] = {};
            float4 K{};
            bool has_desc = false;                         /* its place descriptor was stored with it (dvo_tracker_set_places) */
            long long origin_id = -1;                      /* who made it: itself, or -- imported (stream == -1) -- what its blob recorded */
            int origin_stream = -1;
            long long origin_frame = 0;
        };
        std::vector<Meta> slot;
        long long next_id = 0;                             /* ids never repeat, also across re-configurations */
        std::vector<long long> key_id;                     /* per stream: id of its current key frame, -1 = not archived */
        long long n_archived = 0, n_refused = 0, n_evicted = 0;
        DevBuf<ArchiveStore> d_store; PinnedBuf<ArchiveStore> h_store;    /* 2 K entries: first frames, then switches */
        DevBuf<float> d_xyz;                               /* dvo_tracker_archive_get_points: one decoded list */
        dvo_ctx *mc = nullptr;                             /* max_matches pairs */
        DevBuf<ArchiveLoad> d_load; PinnedBuf<ArchiveLoad> h_load;
        DevBuf<ScoreCand> d_cand; PinnedBuf<ScoreCand> h_cand;
        DevBuf<double> d_cpose; PinnedBuf<double> h_cpose;   /* dvo_tracker_score: the candidates' poses; dvo_tracker_match: the poses read back */
        DevBuf<ScoreRecord> d_rec; PinnedBuf<ScoreRecord> h_rec;
        DevBuf<VerifyCand> d_vcand; PinnedBuf<VerifyCand> h_vcand;      /* dvo_tracker_verify: its candidates and records (the poses go through d_cpose) */
        DevBuf<VerifyRecord> d_vfy; PinnedBuf<VerifyRecord> h_vfy;
        DevBuf<int> d_iota;
        std::vector<int> h_iota;
        int last_launches = 0, last_syncs = 0;
        /* dvo_tracker_archive_export / _import: the blob's device staging buffer, the entry list and the recomputed payload checksums.
         * Allocated and grown inside those calls, never in a step */
        DevBuf<unsigned char> d_blob;
        DevBuf<BlobEntry> d_bent; PinnedBuf<BlobEntry> h_bent;
        DevBuf<unsigned long long> d_bsum; PinnedBuf<unsigned long long> h_bsum;
        /* dvo_tracker_set_places: one descriptor row per slot beside the ring (dvo_tracker_places.hip).  Allocated when switched on */
        struct Places {
            bool on = false;
            int level = -1;
            PlaceView view{};                                      /* the kernels' argument: desc and mark point into the two buffers below */
            DevBuf<unsigned char> desc;
            DevBuf<int> mark;
            DevBuf<PlaceEntry> d_ent; PinnedBuf<PlaceEntry> h_ent;       /* 2 K entries, beside d_store / h_store */
            DevBuf<PlaceQuery> d_query; PinnedBuf<PlaceQuery> h_query;   /* K queries */
            DevBuf<unsigned> d_dist;                               /* K x capacity distances */
            DevBuf<unsigned char> d_out; PinnedBuf<unsigned char> h_out;   /* n * k PlaceOut, then n counts: one copy */
            DevBuf<PlaceShiftCand> d_scand; PinnedBuf<PlaceShiftCand> h_scand;   /* dvo_tracker_place_shifts: K * DVO_TRACKER_PLACES_MAX_K candidates */
            DevBuf<PlaceShiftOut> d_shift; PinnedBuf<PlaceShiftOut> h_shift;     /* ... and their records */
        } pl;
    } ar;
    std::string err;
};

namespace {

int tfail(dvo_tracker *tr, int code, const std::string &msg) {
    tr->err = msg;
    return code;
}
/* an engine call failed: its message becomes the tracker's */
int tchk(dvo_tracker *tr, int rc) {
    if (rc != DVO_OK) tr->err = tr->ctx->err;
    return rc;
}
#define TRK(expr)                                        \
    do {                                                 \
        const int rc_ = tchk(tr, (expr));                \
        if (rc_ != DVO_OK) return rc_;                   \
    } while (0)
#define TRKHIP(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return tfail(tr, DVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

/* the end of a step's launch sequence: the error word of its team launches (if any ran) rides on the step's wait */
int wait_team_checked(dvo_tracker *tr, bool team) {
    dvo_ctx *c = tr->ctx;
    int *team_err = reinterpret_cast<int *>(tr->h_out + tr->K);
    *team_err = 0;
    if (team) TRKHIP(hipMemcpyAsync(team_err, c->d_team_cnt + c->n_pairs, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    if (*team_err) {
        c->team_err_dirty = true;
        return tfail(tr, DVO_ERR_HIP, "team mode: a workgroup gave up waiting for its team; the results of this step are void -- "
                                      "set dvo_params.team_size = 1");
    }
    return DVO_OK;
}

int level_size(int n, int shift) {                     /* cv::resize(Size(), s, s): cvRound(n * 2^-shift), half to even */
    return (int)std::nearbyint(std::ldexp((double)n, -shift));
}

/* the grey image of the descriptor level as the frame store holds it (dvo_tracker_set_places) */
PlaceGrey place_grey(const dvo_tracker *tr) {
    const FrameLevel &F = tr->ctx->fs.lv[tr->ar.pl.level];
    return PlaceGrey{F.grey, F.npx, tr->ctx->fs.n_slots, 0};
}

/* consecutive streams that go to the same bank form one run: [a, b) of the sorted entries */
template <typename F>
int for_runs(const std::vector<int> &sorted, const std::vector<int> &stream_of, const std::vector<int> &bank_of, bool by_bank, F fn) {
    for (size_t a = 0; a < sorted.size();) {
        size_t b = a + 1;
        while (b < sorted.size() && stream_of[sorted[b]] == stream_of[sorted[b - 1]] + 1 &&
               (!by_bank || bank_of[sorted[b]] == bank_of[sorted[a]]))
            b++;
        const int rc = fn(a, b);
        if (rc) return rc;
        a = b;
    }
    return DVO_OK;
}

using Uploader = std::function<int(const std::vector<int> &idx, int slot0, int pair0)>;

int step_impl(dvo_tracker *tr, int count, const int *streams, const Uploader &upload, double *R_rel, double *t_rel, int *event) {
    dvo_ctx *c = tr->ctx;
    const int K = tr->K;
    if (!c->have_K) return tfail(tr, DVO_ERR_STATE, "intrinsics not set (dvo_tracker_set_intrinsics)");
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    int cap0[DVO_LEVELS];
    for (int l = 0; l < tr->n_levels; l++) cap0[l] = c->lv[l].pt_cap;
    tr->s_runs = tr->s_keys = tr->s_growths = 0;

    /* banks: a stream's new frame goes to the bank its previous frame is not in; a first frame joins the bank most of the others
     * write this tick, so that a stream that joins late still runs with them */
    std::vector<int> stream_of(count), bank_of(count), order(count);
    int votes[2] = {0, 0};
    for (int i = 0; i < count; i++) {
        stream_of[i] = streams[i];
        order[i] = i;
        const dvo_tracker::Stream &S = tr->st[streams[i]];
        if (S.started) votes[bank_of[i] = 1 - S.bank]++;
    }
    const int join_bank = votes[1] > votes[0] ? 1 : 0;
    for (int i = 0; i < count; i++)
        if (!tr->st[streams[i]].started) bank_of[i] = join_bank;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return stream_of[a] < stream_of[b]; });
    std::vector<int> first, align;                       /* sorted by stream */
    for (int i : order) (tr->st[stream_of[i]].started ? align : first).push_back(i);

    /* 1. frames: upload + pyramid + Canny, installed as the streams' now frames -- one call per run */
    TRK(for_runs(order, stream_of, bank_of, true, [&](size_t a, size_t b) {
        tr->s_runs++;
        const std::vector<int> idx(order.begin() + a, order.begin() + b);
        return upload(idx, bank_of[idx[0]] * K + stream_of[idx[0]], stream_of[idx[0]]);
    }));
    /* reference extraction of any set of streams (entries `set`, frames in bank bank[i]): ONE call of the index-list form, whose
     * launches cover the whole set; its one host synchronisation reads the point counts */
    auto extract = [&](const std::vector<int> &set, const std::vector<int> &bank, int map_off) -> int {
        if (set.empty()) return DVO_OK;
        tr->s_runs++;
        const int n = (int)set.size();
        std::vector<int> slots(n), pairs(n);
        for (int k = 0; k < n; k++) {
            pairs[k] = stream_of[set[k]];
            slots[k] = bank[set[k]] * K + pairs[k];
            tr->h_map[map_off + k] = make_int2(slots[k], pairs[k]);
        }
        TRKHIP(hipMemcpyAsync(tr->d_map + map_off, tr->h_map + map_off, sizeof(int2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        return tchk(tr, frames_as_ref_list(c, slots.data(), pairs.data(), tr->d_map + map_off, n, nullptr));
    };
    /* the level schedule for any set of streams: ONE fused launch through its index list (the packed kernel's launch order), or, for
     * the one-point-per-lane kernel (dvo_params.engine_variant = 1 / interpolate_dt), one launch per run of consecutive streams */
    const bool listed = fused_uses_compact(c->prm.points_in_flight, c->prm.interpolate_dt) && c->prm.engine_variant != 1;
    bool team = false;
    auto align_set = [&](const std::vector<int> &set, int list_off, int aflags) -> int {
        if (set.empty()) return DVO_OK;
        const int n = (int)set.size();
        if (listed) {
            tr->s_runs++;
            for (int k = 0; k < n; k++) tr->h_pairs[list_off + k] = stream_of[set[k]];
            TRKHIP(hipMemcpyAsync(tr->d_pairs + list_off, tr->h_pairs + list_off, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            const int rc = enqueue_pair_list(c, tr->h_pairs + list_off, tr->d_pairs + list_off, n, tr->n_levels, tr->tp.iters, aflags);
            team = team || c->team_used;
            return tchk(tr, rc);
        }
        return tchk(tr, for_runs(set, stream_of, bank_of, false, [&](size_t a, size_t b) {
            tr->s_runs++;
            const int rc = dvo_align_batch_enqueue(c, stream_of[set[a]], (int)(b - a), tr->n_levels, tr->tp.iters, aflags);
            team = team || c->team_used;
            return rc;
        }));
    };

    /* the key-frame archive (dvo_tracker_archive.hip): the lists `extract` has just written for `set` go to the next slots of the ring --
     * ONE launch, ordered on the stream, no wait; the host knows the counts from the extraction's own synchronisation */
    auto archive = [&](const std::vector<int> &set, const std::vector<int> &bank, int off, bool is_first) -> int {
        if (!tr->ar.on || set.empty()) return DVO_OK;
        dvo_tracker::Archive &A = tr->ar;
        int n = 0;
        for (int i : set) {
            const int p = stream_of[i];
            bool fits = true;
            for (int l = 0; l < tr->n_levels; l++) fits = fits && c->lv[l].hN[p] <= A.cap[l];
            if (!fits) { A.key_id[p] = -1; A.n_refused++; continue; }
            const long long id = A.next_id++;
            const int slot = (int)(id % A.capacity);
            dvo_tracker::Archive::Meta &M = A.slot[slot];
            if (M.id >= 0) {
                A.n_evicted++;
                for (long long &k : A.key_id) if (k == M.id) k = -1;      /* a stream that still tracks against it keeps tracking; the id is gone */
            }
            const Intrinsics Ks = intrinsics_of(c, p);
            M.id = id; M.stream = p; M.frame = is_first ? 0 : tr->st[p].n_frame - 1;
            M.origin_id = id; M.origin_stream = p; M.origin_frame = M.frame;       /* a native key frame is its own origin */
            M.K = make_float4(Ks.fx, Ks.fy, Ks.cx, Ks.cy);
            for (int l = 0; l < DVO_LEVELS; l++) M.N[l] = l < tr->n_levels ? c->lv[l].hN[p] : 0;
            A.key_id[p] = id; A.n_archived++;
            M.has_desc = A.pl.on;
            if (A.pl.on) A.pl.h_ent[off + n] = PlaceEntry{bank[i] * K + p, slot};      /* the frame that has just become the reference */
            A.h_store[off + n++] = ArchiveStore{p, slot, (long long)M.frame, M.K};
        }
        /* more new key frames in one tick than the ring has slots: the earlier ones were evicted by the later ones before they were written */
        int kept = 0;
        for (int j = 0; j < n; j++) {
            bool reused = false;
            for (int k = j + 1; k < n; k++) reused = reused || A.h_store[off + k].slot == A.h_store[off + j].slot;
            if (!reused) {
                if (A.pl.on) A.pl.h_ent[off + kept] = A.pl.h_ent[off + j];
                A.h_store[off + kept++] = A.h_store[off + j];
            }
        }
        n = kept;
        if (n == 0) return DVO_OK;
        LevelSet ls;
        for (int l = 0; l < DVO_LEVELS; l++) ls.l[l] = slab_of(c, l);
        TRKHIP(hipMemcpyAsync(A.d_store + off, A.h_store + off, sizeof(ArchiveStore) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        TRKHIP(launch_archive_store(A.d_store + off, n, ls, A.view, c->stream));
        /* their place descriptors, from the grey level the frame store holds: ONE more launch, same order, no wait */
        if (A.pl.on) {
            TRKHIP(hipMemcpyAsync(A.pl.d_ent + off, A.pl.h_ent + off, sizeof(PlaceEntry) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            TRKHIP(launch_place_store(A.pl.d_ent + off, n, place_grey(tr), A.pl.view, c->stream));
        }
        return DVO_OK;
    };

    /* 2. first frames: reference frame + first key frame (processFirstFrame, SolveDVO.cpp:1972-2021) */
    {
        int rc = extract(first, bank_of, 0);
        if (rc) return rc;
        if ((rc = archive(first, bank_of, 0, true))) return rc;
    }
    const int nA = (int)align.size(), nF = (int)first.size();
    for (int k = 0; k < nA; k++) {
        const dvo_tracker::Stream &S = tr->st[stream_of[align[k]]];
        int f = 0;
        if (S.n_frame - S.last_ref == tr->tp.key_frame_every) f |= DVO_TRK_FORCED;        /* :2155-2160 */
        if (S.last_ref != S.n_frame - 1) f |= DVO_TRK_MAY_SWITCH;                          /* :2198 */
        tr->h_list[k] = TrackerEntry{stream_of[align[k]], f};
    }
    for (int k = 0; k < nF; k++) tr->h_list[nA + k] = TrackerEntry{stream_of[first[k]], 0};
    TRKHIP(hipMemcpyAsync(tr->d_list, tr->h_list, sizeof(TrackerEntry) * (size_t)(nA + nF), hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_tracker_reset_listed(tr->d_list + nA, nF, c->d_poses, c->stream));    /* identityPose of processFirstFrame */

    /* the pose information of the aligned streams (dvo_tracker_info.hip): ONE launch over the list -- of the entries that did not switch
     * key frame (switched = 0, after the signals kernel wrote their events) or of those that did (1, after their re-run) -- and the
     * records' copy, which the step's next wait covers */
    auto information = [&](int switched) -> int {
        TRKHIP(launch_tracker_information(tr->d_list, tr->d_out, switched, nA, c->d_poses, slab_of(c, tr->last_level), tr->last_level, c->K,
                                          native_compact_wanted(c), tr->d_info, c->stream));
        TRKHIP(hipMemcpyAsync(tr->h_info, tr->d_info, sizeof(TrackerInfo) * (size_t)nA, hipMemcpyDeviceToHost, c->stream));
        return DVO_OK;
    };
    /* the debug views of the listed streams (dvo_tracker_views.hip): one rendering = TWO launches over the list, with the filter of
     * information() -- switched = 0 also covers the streams on their first frame (backgrounds only) -- and the histogram records' copy */
    auto views = [&](int switched) -> int {
        const FrameLevel &F = c->fs.lv[tr->last_level];
        TRKHIP(launch_tracker_views(tr->d_list, tr->d_out, tr->d_vslot, nA, switched ? nA : nA + nF, switched, c->d_poses,
                                    slab_of(c, tr->last_level), tr->last_level, c->K, native_compact_wanted(c), F.grey, F.npx, tr->d_views, tr->view_stride,
                                    tr->view_stride * (size_t)K, tr->d_vrec, c->stream));
        TRKHIP(hipMemcpyAsync(tr->h_vrec, tr->d_vrec, sizeof(TrackerViewRecord) * (size_t)(nA + nF), hipMemcpyDeviceToHost, c->stream));
        return DVO_OK;
    };
    if (tr->views_on) {
        for (int k = 0; k < nA + nF; k++) {
            const int i = k < nA ? align[k] : first[k - nA];
            tr->h_vslot[k] = bank_of[i] * K + stream_of[i];
        }
        TRKHIP(hipMemcpyAsync(tr->d_vslot, tr->h_vslot, sizeof(int) * (size_t)(nA + nF), hipMemcpyHostToDevice, c->stream));
    }
    /* 3. the other streams: the level schedule from their last estimate (:2097-2104) */
    {
        const int rc = align_set(align, 0, tr->tp.adaptive ? DVO_FLAG_FINAL_OUTPUTS : 0);
        if (rc) return rc;
    }
    if (nA > 0) {
        /* 4. signals + key-frame rule + poses of every aligned stream: one launch, one read */
        const Level &Lf = c->lv[tr->last_level];
        const bool with_eps = tr->tp.adaptive != 0;
        const bool blk = with_eps && c->sched.final_blk;
        if (blk && (size_t)nA * c->final_cap > tr->d_scratch.size()) {
            TRKHIP(stream_wait(c->stream));
            TRKHIP(tr->d_scratch.alloc((size_t)K * c->final_cap));
        }
        const TrackerRule rule{tr->tp.adaptive, tr->tp.laplacian_b_thresh, tr->tp.visible_ratio_thresh, tr->tp.min_points};
        TRKHIP(launch_tracker_signals(tr->d_list, nA, c->d_poses, c->d_ratio, tr->last_level, with_eps ? c->d_final_N : Lf.dN,
                                      with_eps ? c->d_final_eps : nullptr, blk ? Lf.cidx : nullptr, c->final_cap, Lf.pt_cap,
                                      tr->d_scratch, c->final_cap, rule, tr->d_out, c->stream));
        TRKHIP(hipMemcpyAsync(tr->h_out, tr->d_out, sizeof(TrackerOut) * (size_t)nA, hipMemcpyDeviceToHost, c->stream));
        /* 4b. pose information of the streams that keep their key frame: one launch, its records ride on the same wait */
        if (tr->info_on) {
            const int rc = information(0);
            if (rc) return rc;
        }
    }
    /* 4c. the views of the streams that keep their key frame and of those on their first frame: one rendering, same wait */
    if (tr->views_on) {
        const int rc = views(0);
        if (rc) return rc;
    }
    if (const int rc = wait_team_checked(tr, team)) return rc;

    /* 5. key-frame switches (:2198-2232): the previous frame becomes the reference, the estimate the identity, the alignment re-runs */
    std::vector<int> sw;                                   /* sorted by stream */
    std::vector<int> old_bank(count);
    for (int k = 0; k < nA; k++) {
        const int i = align[k];
        old_bank[i] = tr->st[stream_of[i]].bank;
        if (tr->h_out[k].event >= 2) sw.push_back(i);
    }
    if (!sw.empty()) {
        tr->s_keys = (int)sw.size();
        int rc = extract(sw, old_bank, K);
        if (rc) return rc;
        if ((rc = archive(sw, old_bank, K, false))) return rc;
        TRKHIP(launch_tracker_reset_switched(tr->d_list, tr->d_out, nA, c->d_poses, c->stream));
        team = false;
        if ((rc = align_set(sw, K, 0))) return rc;
        TRKHIP(launch_tracker_gather_switched(tr->d_list, nA, c->d_poses, tr->d_out, c->stream));
        TRKHIP(hipMemcpyAsync(tr->h_out, tr->d_out, sizeof(TrackerOut) * (size_t)nA, hipMemcpyDeviceToHost, c->stream));
        /* ... and of the streams that switched: at the re-run's pose, against their new reference */
        if (tr->info_on) {
            const int rc = information(1);
            if (rc) return rc;
        }
        if (tr->views_on) {
            const int rc = views(1);
            if (rc) return rc;
        }
        if ((rc = wait_team_checked(tr, team))) return rc;
    }

    /* 6. outputs and the streams' counters */
    for (int k = 0; k < nA; k++) {
        const int i = align[k];
        const TrackerOut &o = tr->h_out[k];
        std::memcpy(R_rel + 9 * (size_t)i, o.pose, sizeof(double) * 9);
        std::memcpy(t_rel + 3 * (size_t)i, o.pose + 9, sizeof(double) * 3);
        event[i] = o.event;
        dvo_tracker::Stream &S = tr->st[stream_of[i]];
        S.have_signals = true;
        S.b_cap = o.b_cap; S.ratio = o.ratio; S.n_points = o.n_points;
        S.have_info = tr->info_on;
        if (tr->info_on) S.info = tr->h_info[k];
        S.have_views = tr->views_on;
        if (tr->views_on) S.vrec = tr->h_vrec[k];
        if (o.event >= 2) S.last_ref = S.n_frame - 1;
        S.n_frame++;
        S.bank = bank_of[i];
    }
    for (int i : first) {
        for (int k = 0; k < 9; k++) R_rel[9 * (size_t)i + k] = (k % 4 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 3; k++) t_rel[3 * (size_t)i + k] = 0.0;
        event[i] = 1;
        dvo_tracker::Stream &S = tr->st[stream_of[i]];
        S = dvo_tracker::Stream();
        S.started = true;
        S.n_frame = 1;                                     /* lastRefFrame = 0; nFrame++ (:2014-2021) */
        S.have_info = tr->info_on;                         /* no alignment happened: the zero record */
        S.info.level = -1;
        S.have_views = tr->views_on;                       /* plain backgrounds, the zero histogram */
        S.vrec.level = -1;
        S.bank = bank_of[i];
    }
    for (int l = 0; l < tr->n_levels; l++) tr->s_growths += (c->lv[l].pt_cap != cap0[l]);
    tr->s_launches = (int)(g_kernel_launches - launches0);
    tr->s_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

/* the refusals of both step forms; nothing is changed before they pass */
int check_step(dvo_tracker *tr, int count, const int *streams, const void *R_rel, const void *t_rel, const int *event) {
    if (count < 1 || count > tr->K) return tfail(tr, DVO_ERR_INVALID, "count must be in [1, max_streams]");
    if (!streams || !R_rel || !t_rel || !event) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    std::vector<char> seen(tr->K, 0);
    for (int i = 0; i < count; i++) {
        const int s = streams[i];
        if (s < 0 || s >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(s) + " out of range");
        if (seen[s]) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(s) + " listed twice");
        seen[s] = 1;
    }
    return DVO_OK;
}


/* ---- key-frame archive (dvo_tracker_set_archive ...): host side of dvo_tracker_archive.hip ------------------------------------ */
void places_release(dvo_tracker *tr) {
    dvo_tracker::Archive::Places &P = tr->ar.pl;
    P = dvo_tracker::Archive::Places();
    for (dvo_tracker::Archive::Meta &M : tr->ar.slot) M.has_desc = false;
}

void archive_release(dvo_tracker *tr) {
    dvo_tracker::Archive &A = tr->ar;
    places_release(tr);
    if (A.mc) { A.mc->stream = A.mc->own_stream; dvo_destroy(A.mc); }
    const long long next = A.next_id;
    A = dvo_tracker::Archive();
    A.next_id = next;
}

/* the slot that holds `id`, or NULL (never given, refused, evicted, or the archive is off) */
const dvo_tracker::Archive::Meta *archive_find(const dvo_tracker *tr, long long id, int *slot = nullptr) {
    const dvo_tracker::Archive &A = tr->ar;
    if (!A.on || id < 0 || id >= A.next_id) return nullptr;
    const int s = (int)(id % A.capacity);
    if (A.slot[s].id != id) return nullptr;
    if (slot) *slot = s;
    return &A.slot[s];
}

/* the refusals of dvo_tracker_score and dvo_tracker_match; nothing is changed before they pass */
int check_candidates(dvo_tracker *tr, int n, const int *stream, const long long *key_id, const void *R, const void *t, const void *records) {
    const dvo_tracker::Archive &A = tr->ar;
    if (!A.on) return tfail(tr, DVO_ERR_STATE, "the key-frame archive is off (dvo_tracker_set_archive)");
    if (n < 1 || n > A.max_matches) return tfail(tr, DVO_ERR_INVALID, "n must be in [1, max_matches]");
    if (!stream || !key_id || !R || !t || !records) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; i++)
        if (stream[i] < 0 || stream[i] >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(stream[i]) + " out of range");
    for (int i = 0; i < n; i++) {
        if (!tr->st[stream[i]].started)
            return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream[i]) + " has not been stepped yet: it has no now frame");
        for (int l = 0; l < tr->n_levels; l++)
            if (!tr->ctx->lv[l].now[stream[i]].ready())
                return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream[i]) + " has no now frame");
        const dvo_tracker::Archive::Meta *M = archive_find(tr, key_id[i]);
        if (!M) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " is not in the archive (unknown or evicted)");
    }
    for (int i = 0; i < n; i++) {
        const Intrinsics Ks = intrinsics_of(tr->ctx, stream[i]);
        const float4 k = make_float4(Ks.fx, Ks.fy, Ks.cx, Ks.cy);
        if (std::memcmp(&k, &archive_find(tr, key_id[i])->K, sizeof(float4)) != 0)
            return tfail(tr, DVO_ERR_INVALID, "key frame " + std::to_string(key_id[i]) + " was enlisted under another camera model than stream " +
                                                  std::to_string(stream[i]) + "'s: a pair is decoded and projected under one model");
    }
    return DVO_OK;
}

/* information, views and the archive read the packed engine's resident forms (the compact point lists of the index-list alignment;
 * the one-point-per-lane engine keeps other forms): the refusal of whatever `what_needs` them */
int check_resident_forms(dvo_tracker *tr, const char *what_needs) {
    const dvo_params &prm = tr->ctx->prm;
    if (prm.interpolate_dt || prm.engine_variant == 1 || !fused_uses_compact(prm.points_in_flight, prm.interpolate_dt) || prm.debug_alias_mod > 0)
        return tfail(tr, DVO_ERR_INVALID, std::string(what_needs) + " the packed engine's resident forms: not available with "
                                                                    "dvo_params.interpolate_dt, engine_variant = 1 or debug_alias_mod");
    return DVO_OK;
}

/* the 21 upper-triangle entries of a symmetric 6x6 matrix, row by row -> all 36 */
void expand_sym6(const double *H21, double *H36) {
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { H36[i * 6 + j] = H21[k]; H36[j * 6 + i] = H21[k]; k++; }
}

void expand_record(const ScoreRecord &r, dvo_tracker_score_record &o) {
    expand_sym6(r.H, o.H36);
    std::memcpy(o.g6, r.g, sizeof(double) * 6);
    o.sum_eps2 = r.sum_eps2;
    o.n_points = r.n_points;
    o.n_visible = r.n_visible;
}

/* ---- export and import of the archive (dvo_tracker_archive_export ...): host side of dvo_tracker_archive_blob.hip -------------- */
const char *kArchiveOff = "the key-frame archive is off (dvo_tracker_set_archive)";

/* the slots an export lists, in its order, and the size of its blob; nothing is changed */
int export_plan(dvo_tracker *tr, int n, const long long *key_id, std::vector<int> &slots, size_t &total) {
    const dvo_tracker::Archive &A = tr->ar;
    if (!A.on) return tfail(tr, DVO_ERR_STATE, kArchiveOff);
    if (n < 0) return tfail(tr, DVO_ERR_INVALID, "n must be >= 0");
    slots.clear();
    if (!key_id) {                                         /* every live key frame, ascending id */
        for (long long id = std::max(0LL, A.next_id - A.capacity); id < A.next_id; id++) {
            int slot = 0;
            if (archive_find(tr, id, &slot)) slots.push_back(slot);
        }
    } else {
        for (int i = 0; i < n; i++) {
            int slot = 0;
            if (!archive_find(tr, key_id[i], &slot))
                return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " is not in the archive (unknown, refused or evicted)");
            slots.push_back(slot);
        }
    }
    if (slots.size() > (size_t)INT32_MAX) return tfail(tr, DVO_ERR_INVALID, "too many key frames for one blob");
    uint64_t bytes = sizeof(dvo_blob::Header) + sizeof(dvo_blob::Record) * (uint64_t)slots.size();
    for (int slot : slots) {
        const dvo_tracker::Archive::Meta &M = A.slot[slot];
        bytes += dvo_blob::payload_bytes(M.N, tr->n_levels, A.pl.on && M.has_desc, A.pl.view.D);
    }
    total = (size_t)bytes;
    return DVO_OK;
}

/* room for a blob of `bytes` and n entries in the archive's staging buffers.  Nothing of an earlier call is pending on them but an
 * import's scatter launch: the stream is drained before a buffer is replaced */
int blob_buffers(dvo_tracker *tr, size_t bytes, size_t n) {
    dvo_tracker::Archive &A = tr->ar;
    if (A.d_blob.size() >= bytes && A.d_bent.size() >= n) return DVO_OK;
    TRKHIP(stream_wait(tr->ctx->stream));
    if (A.d_blob.size() < bytes) TRKHIP(A.d_blob.alloc(bytes));
    if (A.d_bent.size() < n) {
        A.d_bsum.reset(); A.h_bsum.reset(); A.h_bent.reset();
        TRKHIP(A.d_bsum.alloc(n));
        TRKHIP(A.h_bsum.alloc(n));
        TRKHIP(A.h_bent.alloc(n));
        TRKHIP(A.d_bent.alloc(n));                         /* last: the test for all four */
    }
    return DVO_OK;
}

}  // namespace

extern "C" {

int dvo_tracker_params_default(dvo_tracker_params *tp) {
    if (!tp) return DVO_ERR_INVALID;
    std::memset(tp, 0, sizeof(*tp));
    for (int l = 0; l < DVO_MAX_LEVELS; l++) tp->iters[l] = 50;       /* iterationsConfig, SolveDVO.cpp:30-33 */
    tp->key_frame_every = 5;                                          /* :2156 */
    tp->adaptive = 0;
    tp->laplacian_b_thresh = 3.0f;                                    /* :22-23 */
    tp->visible_ratio_thresh = 0.8f;
    tp->min_points = 50;                                              /* :2146 */
    tp->rows = 480; tp->cols = 640; tp->n_levels = 4; tp->first_shift = 1;
    return DVO_OK;
}

const char *dvo_tracker_last_error(const dvo_tracker *tr) { return tr ? tr->err.c_str() : dvo_last_error(nullptr); }

int dvo_tracker_create(const dvo_params *p, int max_streams, const dvo_tracker_params *tpp, dvo_tracker **out) {
    if (!out) return fail(nullptr, DVO_ERR_INVALID, "out is NULL");
    *out = nullptr;
    dvo_tracker_params tp;
    if (tpp) tp = *tpp; else dvo_tracker_params_default(&tp);
    if (max_streams < 1) return fail(nullptr, DVO_ERR_INVALID, "max_streams must be >= 1");
    if (tp.n_levels < 1 || tp.n_levels > DVO_LEVELS || tp.rows < 1 || tp.cols < 1 || tp.first_shift < 0 || tp.first_shift + tp.n_levels > 16 ||
        tp.key_frame_every < 1)
        return fail(nullptr, DVO_ERR_INVALID, "bad tracker parameters (geometry / key_frame_every)");
    int last = -1;
    for (int l = tp.n_levels - 1; l >= 0; l--) if (tp.iters[l] > 0) last = l;
    if (last < 0) return fail(nullptr, DVO_ERR_INVALID, "the level schedule has no iterations");
    dvo_ctx *c = nullptr;
    int rc = dvo_create_batch(p, max_streams, &c);
    if (rc) return rc;
    dvo_tracker *tr = new dvo_tracker();
    tr->ctx = c;
    tr->K = max_streams;
    tr->tp = tp;
    tr->n_levels = tp.n_levels;
    tr->last_level = last;
    for (int l = 0; l < tp.n_levels; l++) {
        tr->lr[l] = level_size(tp.rows, tp.first_shift + l);
        tr->lc[l] = level_size(tp.cols, tp.first_shift + l);
        if (tr->lr[l] < 1 || tr->lc[l] < 1) { rc = tfail(tr, DVO_ERR_INVALID, "pyramid level would be empty"); break; }
    }
    tr->st.assign(max_streams, dvo_tracker::Stream());
    auto setup = [&]() -> int {
        DeviceGuard g(c);
        TRK(dvo_frames_reserve(c, 2 * max_streams));                   /* two banks of K slots */
        for (int l = 0; l < tp.n_levels; l++)
            if (tp.points_capacity[l] > 0) TRK(ensure_points(c, l, tp.points_capacity[l]));
        const size_t K = (size_t)max_streams;
        TRKHIP(tr->d_list.alloc(K));
        TRKHIP(tr->h_list.alloc(K));
        TRKHIP(tr->d_out.alloc(K));
        TRKHIP(tr->h_out.alloc(K + 1));
        TRKHIP(tr->d_pairs.alloc(2 * K));
        TRKHIP(tr->h_pairs.alloc(2 * K));
        TRKHIP(tr->d_map.alloc(2 * K));
        TRKHIP(tr->h_map.alloc(2 * K));
        TRKHIP(stream_wait(c->stream));
        return DVO_OK;
    };
    if (rc == DVO_OK) rc = setup();
    if (rc) {
        fail(nullptr, rc, tr->err);
        dvo_tracker_destroy(tr);
        return rc;
    }
    *out = tr;
    return DVO_OK;
}

int dvo_tracker_destroy(dvo_tracker *tr) {
    if (!tr) return DVO_ERR_INVALID;
    dvo_ctx *c = tr->ctx;
    DeviceGuard g(c);
    if (c) {
        (void)stream_wait(c->stream);
        archive_release(tr);
        if (tr->ev_col) (void)hipEventDestroy(tr->ev_col);
    }
    delete tr;              /* the tracker's buffers go before its context's stream does */
    return dvo_destroy(c);
}

int dvo_tracker_set_intrinsics(dvo_tracker *tr, float fx, float fy, float cx, float cy) {
    if (!tr) return DVO_ERR_INVALID;
    return tchk(tr, dvo_set_intrinsics(tr->ctx, fx, fy, cx, cy));
}

/* per-stream calibration: refusals first (nothing changes), then the start-of-stream rule -- a reference's points were enlisted
 * under the stream's old camera model */
static int stream_camera_check(dvo_tracker *tr, int stream) {
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    return DVO_OK;
}
static int stream_at_start(dvo_tracker *tr, int stream) {
    if (tr->st[stream].started)
        return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream) + " is running: its calibration may change only before its first "
                                        "frame (dvo_tracker_reset_stream)");
    return DVO_OK;
}

int dvo_tracker_set_stream_intrinsics(dvo_tracker *tr, int stream, float fx, float fy, float cx, float cy) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = stream_camera_check(tr, stream);
    if (rc) return rc;
    if (!(fx > 0.0f) || !(fy > 0.0f)) return tfail(tr, DVO_ERR_INVALID, "fx, fy must be positive");
    if ((rc = stream_at_start(tr, stream))) return rc;
    DeviceGuard g(tr->ctx);
    return tchk(tr, pair_intrinsics_set(tr->ctx, stream, true, fx, fy, cx, cy));
}

int dvo_tracker_set_stream_undistort(dvo_tracker *tr, int stream, const double *K4, const double *D5) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = stream_camera_check(tr, stream);
    if (rc) return rc;
    if (!K4 != !D5) return tfail(tr, DVO_ERR_INVALID, "K4 and D5 go together (both NULL: no undistortion for this stream)");
    if (K4 && (!(K4[0] > 0.0) || !(K4[1] > 0.0))) return tfail(tr, DVO_ERR_INVALID, "fx, fy must be positive");
    for (int k = 0; K4 && k < 9; k++)
        if (!std::isfinite(k < 4 ? K4[k] : D5[k - 4])) return tfail(tr, DVO_ERR_INVALID, "K4 and D5 must be finite");
    if ((rc = stream_at_start(tr, stream))) return rc;
    DeviceGuard g(tr->ctx);
    return tchk(tr, pair_undistort_set(tr->ctx, stream, K4 ? 1 : 0, tr->tp.rows, tr->tp.cols, K4, D5));
}

int dvo_tracker_clear_stream_camera(dvo_tracker *tr, int stream) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = stream_camera_check(tr, stream);
    if (rc) return rc;
    if ((rc = stream_at_start(tr, stream))) return rc;
    DeviceGuard g(tr->ctx);
    TRK(pair_intrinsics_set(tr->ctx, stream, false, 0.0f, 0.0f, 0.0f, 0.0f));
    return tchk(tr, pair_undistort_set(tr->ctx, stream, -1, 0, 0, nullptr, nullptr));
}

/* the stream's ignore mask (stream = pair): the frame stage applies it to the stream's next frame; nothing of the tracker's own state
 * depends on it, so it may change while the stream runs */
int dvo_tracker_set_stream_mask(dvo_tracker *tr, int stream, const unsigned char *mask, int margin) {
    if (!tr) return DVO_ERR_INVALID;
    if (stream < -1 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range (-1: every stream)");
    return tchk(tr, dvo_frames_set_pair_mask(tr->ctx, stream, tr->tp.rows, tr->tp.cols, mask, tr->n_levels, tr->tp.first_shift, margin));
}

int dvo_tracker_reset_stream(dvo_tracker *tr, int stream) {
    if (!tr) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    tr->st[stream] = dvo_tracker::Stream();
    return DVO_OK;
}

int dvo_tracker_step(dvo_tracker *tr, int count, const int *streams, const unsigned char *const *bgr8, const float *const *depth_m,
                     int rows, int cols, int flags, double *R_rel, double *t_rel, int *event) {
    return dvo_tracker_step_fmt(tr, count, streams, reinterpret_cast<const void *const *>(bgr8), DVO_CAM_BGR8,
                                reinterpret_cast<const void *const *>(depth_m), DVO_DEPTH_F32, rows, cols, flags, R_rel, t_rel, event);
}

int dvo_tracker_step_fmt(dvo_tracker *tr, int count, const int *streams, const void *const *bgr8, int image_format,
                         const void *const *depth_m, int depth_format, int rows, int cols, int flags, double *R_rel, double *t_rel, int *event) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = check_step(tr, count, streams, R_rel, t_rel, event);
    if (rc) return rc;
    if (image_format < DVO_CAM_BGR8 || image_format > DVO_CAM_MONO8 || depth_format < DVO_DEPTH_F32 || depth_format > DVO_DEPTH_U16)
        return tfail(tr, DVO_ERR_INVALID, "unknown image or depth format (DVO_CAM_* / DVO_DEPTH_*)");
    if (rows != tr->tp.rows || cols != tr->tp.cols)
        return tfail(tr, DVO_ERR_INVALID, "frame geometry differs from the tracker's (dvo_tracker_params.rows / cols)");
    if (!bgr8 || !depth_m) return tfail(tr, DVO_ERR_INVALID, "colour and depth frames are both needed (every frame can become a reference)");
    for (int i = 0; i < count; i++)
        if (!bgr8[i] || !depth_m[i]) return tfail(tr, DVO_ERR_INVALID, "NULL camera image");
    DeviceGuard g(tr->ctx);
    const int up_flags = (flags & (DVO_UPLOAD_DEVICE | DVO_UPLOAD_MAPPED | DVO_UPLOAD_DIRECT | DVO_UPLOAD_DEPTH_RAW)) | DVO_UPLOAD_ASYNC;
    std::vector<const void *> b(count), d(count);
    const Uploader up = [&](const std::vector<int> &idx, int slot0, int pair0) {
        for (size_t k = 0; k < idx.size(); k++) { b[k] = bgr8[idx[k]]; d[k] = depth_m[idx[k]]; }
        return dvo_frames_upload_cameras_fmt(tr->ctx, slot0, (int)idx.size(), b.data(), image_format, d.data(), depth_format, rows, cols,
                                             tr->n_levels, tr->tp.first_shift, pair0, up_flags);
    };
    return step_impl(tr, count, streams, up, R_rel, t_rel, event);
}

/* the stream's depth rig (stream = pair): the frame stage registers the stream's raw depth images under it.  The registered depth
 * decides which reference points a key frame gets, so the rig may change only where the calibration may */
int dvo_tracker_set_stream_depth_rig(dvo_tracker *tr, int stream, const dvo_depth_rig *rig) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = stream_camera_check(tr, stream);
    if (rc) return rc;
    if (rig && !dvo_depth::rig_ok(rig))
        return tfail(tr, DVO_ERR_INVALID, "bad depth rig (sizes >= 1, focal lengths positive, every number finite, has_Dc5 0 or 1)");
    if ((rc = stream_at_start(tr, stream))) return rc;
    TRK(dvo_frames_set_pair_depth_rig(tr->ctx, stream, rig, tr->tp.rows, tr->tp.cols));
    if (tr->has_rig.empty()) tr->has_rig.assign(tr->K, 0);
    tr->has_rig[stream] = rig ? 1 : 0;
    return DVO_OK;
}

int dvo_tracker_step_raw_depth(dvo_tracker *tr, int count, const int *streams, const void *const *image, int image_format,
                               const void *const *depth, int depth_format, int rows, int cols, int flags, double *R_rel, double *t_rel, int *event) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = check_step(tr, count, streams, R_rel, t_rel, event);
    if (rc) return rc;
    if (image_format < DVO_CAM_BGR8 || image_format > DVO_CAM_MONO8 || depth_format < DVO_DEPTH_F32 || depth_format > DVO_DEPTH_U16)
        return tfail(tr, DVO_ERR_INVALID, "unknown image or depth format (DVO_CAM_* / DVO_DEPTH_*)");
    if (rows != tr->tp.rows || cols != tr->tp.cols)
        return tfail(tr, DVO_ERR_INVALID, "frame geometry differs from the tracker's (dvo_tracker_params.rows / cols)");
    if (flags & ~DVO_UPLOAD_DEVICE) return tfail(tr, DVO_ERR_INVALID, "raw-depth steps take host frames (0) or DVO_UPLOAD_DEVICE");
    if (!image || !depth) return tfail(tr, DVO_ERR_INVALID, "colour and depth frames are both needed (every frame can become a reference)");
    for (int i = 0; i < count; i++)
        if (!image[i] || !depth[i]) return tfail(tr, DVO_ERR_INVALID, "NULL camera image");
    for (int i = 0; i < count; i++)
        if (tr->has_rig.empty() || !tr->has_rig[streams[i]])
            return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(streams[i]) + " has no depth rig (dvo_tracker_set_stream_depth_rig)");
    dvo_ctx *c = tr->ctx;
    DeviceGuard g(c);
    const bool dev_src = (flags & DVO_UPLOAD_DEVICE) != 0;
    const size_t col_stride = ((size_t)rows * cols * (image_format == DVO_CAM_MONO8 ? 1 : 3) + 15) / 16 * 16;
    if (!dev_src) {
        if (!tr->ev_col) TRKHIP(hipEventCreateWithFlags(&tr->ev_col, hipEventDisableTiming));
        if (tr->ev_col_pending) { TRKHIP(hipEventSynchronize(tr->ev_col)); tr->ev_col_pending = false; }     /* only after a step that failed: a step ends with a wait */
        if (col_stride * tr->K > tr->h_col.size()) {
            if (tr->d_col.size()) TRKHIP(stream_wait(c->stream));
            tr->h_col.reset();                              /* allocated last: its size speaks for both */
            TRKHIP(tr->d_col.alloc(col_stride * tr->K));
            TRKHIP(tr->h_col.alloc(col_stride * tr->K));
        }
    }
    std::vector<const void *> b(count), d(count);
    std::vector<const unsigned short *> reg(count);
    const Uploader up = [&](const std::vector<int> &idx, int slot0, int pair0) -> int {
        const int n = (int)idx.size();
        for (int k = 0; k < n; k++) d[k] = depth[idx[k]];
        int rc2 = dvo_frames_register_depth(c, pair0, n, d.data(), depth_format, (flags & DVO_UPLOAD_DEVICE) | DVO_UPLOAD_ASYNC, reg.data());
        if (rc2) return rc2;
        if (dev_src) {
            for (int k = 0; k < n; k++) b[k] = image[idx[k]];
        } else {                                            /* the streams of a run are consecutive: one copy */
            const size_t bytes = (size_t)rows * cols * (image_format == DVO_CAM_MONO8 ? 1 : 3), off = col_stride * (size_t)pair0;
            for (int k = 0; k < n; k++) {
                std::memcpy(tr->h_col + off + col_stride * k, image[idx[k]], bytes);
                b[k] = tr->d_col + off + col_stride * k;
            }
            HIPCHK(c, hipMemcpyAsync(tr->d_col + off, tr->h_col + off, col_stride * (size_t)n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipEventRecord(tr->ev_col, c->stream));
            tr->ev_col_pending = true;
        }
        for (int k = 0; k < n; k++) d[k] = reg[k];
        return dvo_frames_upload_cameras_fmt(c, slot0, n, b.data(), image_format, d.data(), DVO_DEPTH_U16, rows, cols, tr->n_levels,
                                             tr->tp.first_shift, pair0, DVO_UPLOAD_DEVICE | DVO_UPLOAD_ASYNC);
    };
    rc = step_impl(tr, count, streams, up, R_rel, t_rel, event);
    if (rc == DVO_OK) tr->ev_col_pending = false;           /* the step's wait covered the staging copies */
    return rc;
}

int dvo_tracker_step_pyramids(dvo_tracker *tr, int count, const int *streams, const dvo_image *grey, const dvo_image *depth,
                              int flags, double *R_rel, double *t_rel, int *event) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = check_step(tr, count, streams, R_rel, t_rel, event);
    if (rc) return rc;
    const int nl = tr->n_levels;
    if (!grey || !depth) return tfail(tr, DVO_ERR_INVALID, "grey and depth pyramids are both needed");
    for (int i = 0; i < count; i++)
        for (int l = 0; l < nl; l++) {
            const dvo_image &gi = grey[(size_t)i * nl + l], &di = depth[(size_t)i * nl + l];
            if (gi.rows != tr->lr[l] || gi.cols != tr->lc[l] || di.rows != tr->lr[l] || di.cols != tr->lc[l])
                return tfail(tr, DVO_ERR_INVALID, "pyramid level geometry differs from the tracker's");
        }
    DeviceGuard g(tr->ctx);
    const int up_flags = (flags & (DVO_UPLOAD_MAPPED | DVO_UPLOAD_DIRECT)) | DVO_UPLOAD_ASYNC;
    std::vector<dvo_image> gs((size_t)count * nl), ds((size_t)count * nl);
    const Uploader up = [&](const std::vector<int> &idx, int slot0, int pair0) {
        for (size_t k = 0; k < idx.size(); k++)
            for (int l = 0; l < nl; l++) { gs[k * nl + l] = grey[(size_t)idx[k] * nl + l]; ds[k * nl + l] = depth[(size_t)idx[k] * nl + l]; }
        return dvo_frames_upload_pyramids(tr->ctx, slot0, (int)idx.size(), nl, gs.data(), ds.data(), pair0, up_flags);
    };
    return step_impl(tr, count, streams, up, R_rel, t_rel, event);
}

int dvo_tracker_get_signals(dvo_tracker *tr, int stream, float *b_cap, float *visible_ratio, int *n_points) {
    if (!tr) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    const dvo_tracker::Stream &S = tr->st[stream];
    if (!S.have_signals) return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream) + " has not been aligned yet");
    if (b_cap) *b_cap = S.b_cap;
    if (visible_ratio) *visible_ratio = S.ratio;
    if (n_points) *n_points = S.n_points;
    return DVO_OK;
}

int dvo_tracker_set_information(dvo_tracker *tr, int on) {
    if (!tr) return DVO_ERR_INVALID;
    dvo_ctx *c = tr->ctx;
    if (on) {
        if (const int rc = check_resident_forms(tr, "pose information needs")) return rc;
        if (!tr->d_info) {
            DeviceGuard g(c);
            TRKHIP(tr->h_info.alloc((size_t)tr->K));
            TRKHIP(tr->d_info.alloc((size_t)tr->K));           /* last: the test for both */
        }
    }
    if (tr->info_on != (on != 0))
        for (dvo_tracker::Stream &S : tr->st) S.have_info = false;     /* records exist for steps made while it was on */
    tr->info_on = on != 0;
    return DVO_OK;
}

int dvo_tracker_get_information(dvo_tracker *tr, int stream, double *H36, double *g6, double *sum_eps2, int *n_visible, int *level) {
    if (!tr) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    if (!tr->info_on) return tfail(tr, DVO_ERR_STATE, "pose information is off (dvo_tracker_set_information)");
    const dvo_tracker::Stream &S = tr->st[stream];
    if (!S.have_info)
        return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream) + " has not been stepped since pose information was switched on "
                                        "or the stream was reset");
    if (H36) expand_sym6(S.info.H, H36);
    if (g6) std::memcpy(g6, S.info.g, sizeof(double) * 6);
    if (sum_eps2) *sum_eps2 = S.info.sum_eps2;
    if (n_visible) *n_visible = S.info.n_visible;
    if (level) *level = S.info.level;
    return DVO_OK;
}

int dvo_tracker_set_views(dvo_tracker *tr, int on) {
    if (!tr) return DVO_ERR_INVALID;
    dvo_ctx *c = tr->ctx;
    if (on) {
        if (const int rc = check_resident_forms(tr, "views need")) return rc;
        if (!tr->d_views) {
            DeviceGuard g(c);
            const size_t K = (size_t)tr->K;
            tr->view_stride = ((size_t)tr->lr[tr->last_level] * (size_t)tr->lc[tr->last_level] * 3 + 255) & ~(size_t)255;
            TRKHIP(tr->d_vrec.alloc(K));
            TRKHIP(tr->h_vrec.alloc(K));
            TRKHIP(tr->d_vslot.alloc(K));
            TRKHIP(tr->h_vslot.alloc(K));
            TRKHIP(tr->d_views.alloc(2 * K * tr->view_stride));      /* last: the test for all five */
        }
    }
    if (tr->views_on != (on != 0))
        for (dvo_tracker::Stream &S : tr->st) S.have_views = false;    /* views exist for steps made while they were on */
    tr->views_on = on != 0;
    return DVO_OK;
}

/* the refusals of the four getters */
static int views_check(dvo_tracker *tr, int stream, int view) {
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    if (view != DVO_VIEW_REPROJ_ON_DT && view != DVO_VIEW_RESIDUE_HEAT) return tfail(tr, DVO_ERR_INVALID, "unknown view (DVO_VIEW_*)");
    if (!tr->views_on) return tfail(tr, DVO_ERR_STATE, "views are off (dvo_tracker_set_views)");
    if (!tr->st[stream].have_views)
        return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream) + " has not been stepped since views were switched on "
                                        "or the stream was reset");
    return DVO_OK;
}

int dvo_tracker_get_residue_histogram(dvo_tracker *tr, int stream, unsigned *hist260, int *n_points, int *level) {
    if (!tr) return DVO_ERR_INVALID;
    const int rc = views_check(tr, stream, DVO_VIEW_REPROJ_ON_DT);
    if (rc) return rc;
    const TrackerViewRecord &r = tr->st[stream].vrec;
    if (hist260) std::memcpy(hist260, r.hist, sizeof(r.hist));
    if (n_points) *n_points = r.n_points;
    if (level) *level = r.level;
    return DVO_OK;
}

int dvo_tracker_view_size(dvo_tracker *tr, int *rows, int *cols, int *level) {
    if (!tr) return DVO_ERR_INVALID;
    if (rows) *rows = tr->lr[tr->last_level];
    if (cols) *cols = tr->lc[tr->last_level];
    if (level) *level = tr->last_level;
    return DVO_OK;
}

int dvo_tracker_view_device(dvo_tracker *tr, int stream, int view, const unsigned char **d_bgr8) {
    if (!tr) return DVO_ERR_INVALID;
    if (!d_bgr8) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    *d_bgr8 = nullptr;
    const int rc = views_check(tr, stream, view);
    if (rc) return rc;
    *d_bgr8 = tr->d_views + ((size_t)view * (size_t)tr->K + (size_t)stream) * tr->view_stride;
    return DVO_OK;
}

int dvo_tracker_get_view(dvo_tracker *tr, int stream, int view, unsigned char *bgr8) {
    if (!tr) return DVO_ERR_INVALID;
    if (!bgr8) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    const unsigned char *d = nullptr;
    const int rc = dvo_tracker_view_device(tr, stream, view, &d);
    if (rc) return rc;
    DeviceGuard g(tr->ctx);
    TRKHIP(hipMemcpyAsync(bgr8, d, (size_t)tr->lr[tr->last_level] * (size_t)tr->lc[tr->last_level] * 3, hipMemcpyDeviceToHost, tr->ctx->stream));
    TRKHIP(stream_wait(tr->ctx->stream));
    return DVO_OK;
}


int dvo_tracker_set_archive(dvo_tracker *tr, int capacity, int max_matches, const int *points_capacity) {
    if (!tr) return DVO_ERR_INVALID;
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    if (capacity < 0) return tfail(tr, DVO_ERR_INVALID, "capacity must be >= 0 (0 switches the archive off)");
    if (capacity == 0) {
        DeviceGuard g(c);
        TRKHIP(stream_wait(c->stream));
        archive_release(tr);
        return DVO_OK;
    }
    if (max_matches < 1) return tfail(tr, DVO_ERR_INVALID, "max_matches must be >= 1");
    /* slots hold, and the scoring kernel reads, those forms */
    if (const int rc = check_resident_forms(tr, "the key-frame archive needs")) return rc;
    int cap[DVO_LEVELS] = {};
    for (int l = 0; l < tr->n_levels; l++) {
        const int want = points_capacity ? points_capacity[l] : 0;
        if (want < 0) return tfail(tr, DVO_ERR_INVALID, "points_capacity must be >= 0 (0: rows * cols / 8 of the level)");
        const long long v = want > 0 ? want : std::max(1LL, (long long)tr->lr[l] * tr->lc[l] / 8);
        if (v > (1LL << 30)) return tfail(tr, DVO_ERR_INVALID, "points_capacity too large");
        cap[l] = (int)v;
    }
    DeviceGuard g(c);
    TRKHIP(stream_wait(c->stream));
    archive_release(tr);                                   /* a re-configuration starts an empty ring; ids go on counting */
    A.capacity = capacity; A.max_matches = max_matches;
    auto setup = [&]() -> int {
        const size_t S = (size_t)capacity, M = (size_t)max_matches;
        size_t max_cap = 0;
        for (int l = 0; l < tr->n_levels; l++) {
            A.cap[l] = cap[l];                             /* a list of up to cap[l] points fits ... */
            const size_t alloc = ((size_t)cap[l] + 63) / 64 * 64;      /* ... slots are whole chunks of 64 */
            ArchiveLevel &L = A.view.l[l];
            L.cap = (int)alloc;
            max_cap = std::max(max_cap, alloc);
            dvo_tracker::Archive::LevelBufs &B = A.lb[l];
            TRKHIP(B.cpts.alloc(alloc * S));
            TRKHIP(B.cidx.alloc(alloc * S));
            TRKHIP(B.cpt4.alloc(alloc * S));
            TRKHIP(B.chdr.alloc(alloc / 64 * S));
            L.cpts = B.cpts.get(); L.cidx = B.cidx.get(); L.cpt4 = B.cpt4.get(); L.chdr = B.chdr.get();
        }
        A.view.n_levels = tr->n_levels; A.view.n_slots = capacity;
        TRKHIP(A.hdr.alloc(S));
        A.view.hdr = A.hdr.get();
        TRKHIP(hipMemsetAsync(A.view.hdr, 0, sizeof(ArchiveHeader) * S, c->stream));
        TRKHIP(A.d_store.alloc(2 * (size_t)tr->K));
        TRKHIP(A.h_store.alloc(2 * (size_t)tr->K));
        TRKHIP(A.d_xyz.alloc(3 * max_cap));
        TRKHIP(A.d_load.alloc(M));
        TRKHIP(A.h_load.alloc(M));
        TRKHIP(A.d_cand.alloc(M));
        TRKHIP(A.h_cand.alloc(M));
        TRKHIP(A.d_cpose.alloc(12 * M));
        TRKHIP(A.h_cpose.alloc(12 * M));
        TRKHIP(A.d_rec.alloc(M));
        TRKHIP(A.h_rec.alloc(M));
        TRKHIP(A.d_vcand.alloc(M));
        TRKHIP(A.h_vcand.alloc(M));
        TRKHIP(A.d_vfy.alloc(M));
        TRKHIP(A.h_vfy.alloc(M));
        TRKHIP(A.d_iota.alloc(M));
        A.h_iota.resize(M);
        for (size_t i = 0; i < M; i++) A.h_iota[i] = (int)i;
        TRKHIP(hipMemcpyAsync(A.d_iota, A.h_iota.data(), sizeof(int) * M, hipMemcpyHostToDevice, c->stream));
        /* the match context: max_matches pairs with the tracker's level geometry and room for any archived list */
        if (dvo_create_batch(&c->prm, max_matches, &A.mc) != DVO_OK) return tfail(tr, DVO_ERR_HIP, std::string("match context: ") + dvo_last_error(nullptr));
        dvo_ctx *mc = A.mc;
        (void)dvo_set_keep_warm2(mc, 0, 0);                /* DVO_KEEP_WARM is the tracker's context's business: no second thread and stream */
        auto MC = [&](int rc) { if (rc != DVO_OK) tr->err = mc->err; return rc; };
        for (int l = 0; l < tr->n_levels; l++) {
            int rc;
            if ((rc = MC(ensure_points(mc, l, A.view.l[l].cap)))) return rc;
            if ((rc = MC(ensure_texels(mc, l, tr->lr[l], tr->lc[l])))) return rc;
            if (native_compact_wanted(c) && (rc = MC(ensure_compact_slabs(mc, l)))) return rc;
        }
        TRKHIP(stream_wait(mc->stream));
        TRKHIP(stream_wait(c->stream));
        return DVO_OK;
    };
    const int rc = setup();
    if (rc) {
        const std::string msg = tr->err;
        archive_release(tr);
        return tfail(tr, rc, msg);
    }
    A.slot.assign((size_t)capacity, dvo_tracker::Archive::Meta());
    A.key_id.assign((size_t)tr->K, -1);
    A.on = true;
    return DVO_OK;
}

int dvo_tracker_key_frame_id(dvo_tracker *tr, int stream, long long *id) {
    if (!tr) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    if (!id) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    if (!tr->ar.on) return tfail(tr, DVO_ERR_STATE, "the key-frame archive is off (dvo_tracker_set_archive)");
    if (!tr->st[stream].started) return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream) + " has not been stepped yet");
    *id = tr->ar.key_id[stream];
    return DVO_OK;
}

int dvo_tracker_archive_info(dvo_tracker *tr, long long id, int *stream, long long *frame, int *n_points) {
    if (!tr) return DVO_ERR_INVALID;
    const dvo_tracker::Archive::Meta *M = archive_find(tr, id);
    if (!M) return tfail(tr, DVO_ERR_STATE, tr->ar.on ? "key frame " + std::to_string(id) + " is not in the archive (unknown or evicted)"
                                                       : std::string("the key-frame archive is off (dvo_tracker_set_archive)"));
    if (stream) *stream = M->stream;
    if (frame) *frame = M->frame;
    for (int l = 0; n_points && l < tr->n_levels; l++) n_points[l] = M->N[l];
    return DVO_OK;
}

int dvo_tracker_archive_get_points(dvo_tracker *tr, long long id, int level, float *xyz_out, int capacity, int *N_out) {
    if (!tr) return DVO_ERR_INVALID;
    if (level < 0 || level >= tr->n_levels) return tfail(tr, DVO_ERR_INVALID, "level out of range");
    int slot = 0;
    const dvo_tracker::Archive::Meta *M = archive_find(tr, id, &slot);
    if (!M) return tfail(tr, DVO_ERR_STATE, tr->ar.on ? "key frame " + std::to_string(id) + " is not in the archive (unknown or evicted)"
                                                       : std::string("the key-frame archive is off (dvo_tracker_set_archive)"));
    const int N = M->N[level];
    if (N_out) *N_out = N;
    const int ncopy = std::min(N, capacity);
    if (xyz_out && ncopy > 0) {
        dvo_ctx *c = tr->ctx;
        DeviceGuard g(c);
        TRKHIP(launch_archive_decode(tr->ar.view, slot, level, tr->ar.d_xyz, tr->ar.view.l[level].cap, c->stream));
        TRKHIP(hipMemcpyAsync(xyz_out, tr->ar.d_xyz, sizeof(float) * 3 * (size_t)ncopy, hipMemcpyDeviceToHost, c->stream));
        TRKHIP(stream_wait(c->stream));
    }
    return DVO_OK;
}

int dvo_tracker_archive_stats(dvo_tracker *tr, long long *archived, long long *refused, long long *evicted, int *last_launches, int *last_syncs) {
    if (!tr) return DVO_ERR_INVALID;
    if (archived) *archived = tr->ar.n_archived;
    if (refused) *refused = tr->ar.n_refused;
    if (evicted) *evicted = tr->ar.n_evicted;
    if (last_launches) *last_launches = tr->ar.last_launches;
    if (last_syncs) *last_syncs = tr->ar.last_syncs;
    return DVO_OK;
}

int dvo_archive_blob_info(const void *blob, size_t bytes, struct dvo_archive_blob_info *info) {
    static_assert(DVO_LEVELS == dvo_blob::kMaxLevels, "one number of levels");
    if (!blob || !info) return fail(nullptr, DVO_ERR_INVALID, "NULL argument");
    dvo_blob::Info I;
    const std::string defect = dvo_blob::validate(blob, bytes, &I);
    if (!defect.empty()) return fail(nullptr, DVO_ERR_INVALID, "archive blob: " + defect);
    info->version = (int)dvo_blob::kVersion;
    info->rows = I.rows; info->cols = I.cols; info->n_levels = I.n_levels; info->first_shift = I.first_shift;
    info->places_level = I.places_level; info->D = I.D; info->n_key_frames = I.n_key_frames;
    info->total_bytes = I.total_bytes;
    return DVO_OK;
}

int dvo_tracker_archive_export_size(dvo_tracker *tr, int n, const long long *key_id, size_t *bytes) {
    if (!tr) return DVO_ERR_INVALID;
    if (!bytes) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    std::vector<int> slots;
    size_t total = 0;
    const int rc = export_plan(tr, n, key_id, slots, total);
    if (rc) return rc;
    *bytes = total;
    return DVO_OK;
}

int dvo_tracker_archive_export(dvo_tracker *tr, int n, const long long *key_id, void *blob, size_t capacity, size_t *bytes) {
    if (!tr) return DVO_ERR_INVALID;
    if (!blob || !bytes) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    std::vector<int> slots;
    size_t total = 0;
    int rc = export_plan(tr, n, key_id, slots, total);
    if (rc) return rc;
    *bytes = total;
    if (capacity < total)
        return tfail(tr, DVO_ERR_INVALID, "the blob needs " + std::to_string(total) + " bytes, capacity is " + std::to_string(capacity));
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    const int count = (int)slots.size();
    const size_t table_end = sizeof(dvo_blob::Header) + sizeof(dvo_blob::Record) * (size_t)count;
    DeviceGuard g(c);
    if (count > 0 && (rc = blob_buffers(tr, total, (size_t)count))) return rc;
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    if (count > 0) {
        uint64_t off = table_end;
        for (int i = 0; i < count; i++) {
            const dvo_tracker::Archive::Meta &M = A.slot[slots[i]];
            BlobEntry &e = A.h_bent[i];
            e = BlobEntry{};
            e.origin_id = M.origin_id; e.origin_stream = M.origin_stream; e.origin_frame = M.origin_frame;
            e.slot = slots[i]; e.record = i;
            e.has_desc = (A.pl.on && M.has_desc) ? 1 : 0;
            for (int l = 0; l < tr->n_levels; l++) e.N[l] = M.N[l];
            e.payload_offset = off;
            e.payload_bytes = dvo_blob::payload_bytes(M.N, tr->n_levels, e.has_desc, A.pl.view.D);
            off += e.payload_bytes;
        }
        /* the table starts as zeros: the kernel ADDS the payload checksums into it and writes every other field */
        TRKHIP(hipMemsetAsync(A.d_blob, 0, table_end, c->stream));
        TRKHIP(hipMemcpyAsync(A.d_bent, A.h_bent, sizeof(BlobEntry) * (size_t)count, hipMemcpyHostToDevice, c->stream));
        TRKHIP(launch_archive_export(A.d_bent, count, A.view, A.pl.view, A.d_blob, c->stream));
        TRKHIP(hipMemcpyAsync(blob, A.d_blob, total, hipMemcpyDeviceToHost, c->stream));
        TRKHIP(stream_wait(c->stream));
    }
    dvo_blob::write_header(blob, count, total, tr->tp.rows, tr->tp.cols, tr->n_levels, tr->tp.first_shift, A.pl.on ? A.pl.level : -1,
                           A.pl.on ? A.pl.view.D : 0);
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_archive_import(dvo_tracker *tr, const void *blob, size_t bytes, long long *ids_out, int ids_capacity, int *n_in_blob) {
    if (!tr) return DVO_ERR_INVALID;
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    if (!A.on) return tfail(tr, DVO_ERR_STATE, kArchiveOff);
    if (!blob || (!ids_out && ids_capacity > 0) || ids_capacity < 0) return tfail(tr, DVO_ERR_INVALID, "NULL argument or negative ids_capacity");
    dvo_blob::Info I;
    std::vector<dvo_blob::Record> table;
    const std::string defect = dvo_blob::validate(blob, bytes, &I, &table);
    if (!defect.empty()) return tfail(tr, DVO_ERR_INVALID, "archive blob: " + defect);
    if (I.rows != tr->tp.rows || I.cols != tr->tp.cols || I.n_levels != tr->n_levels || I.first_shift != tr->tp.first_shift)
        return tfail(tr, DVO_ERR_INVALID, "archive blob: made by a tracker of " + std::to_string(I.rows) + " x " + std::to_string(I.cols) + ", " +
                                              std::to_string(I.n_levels) + " levels, first_shift " + std::to_string(I.first_shift) +
                                              ": not this tracker's geometry");
    const int n = I.n_key_frames;
    if (n_in_blob) *n_in_blob = n;
    if (n == 0) { A.last_launches = A.last_syncs = 0; return DVO_OK; }
    /* descriptors travel only into the same descriptor geometry */
    const bool take_desc = A.pl.on && A.pl.level == I.places_level && A.pl.view.D == I.D;
    DeviceGuard g(c);
    int rc = blob_buffers(tr, bytes, (size_t)n);
    if (rc) return rc;
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    /* the plan: ids and slots under the ring rule, as the step's store gives them.  Nothing of the tracker changes before the payload
     * checksums have come back */
    std::vector<long long> ids((size_t)n, -1);
    long long next = A.next_id;
    for (int i = 0; i < n; i++) {
        const dvo_blob::Record &r = table[(size_t)i];
        BlobEntry &e = A.h_bent[i];
        e = BlobEntry{};
        e.origin_id = r.origin_id; e.origin_stream = r.origin_stream; e.origin_frame = r.origin_frame;
        e.payload_offset = r.payload_offset; e.payload_bytes = r.payload_bytes;
        e.record = i; e.has_desc = (take_desc && r.has_desc) ? 1 : 0;
        bool fits = true;
        for (int l = 0; l < DVO_LEVELS; l++) { e.N[l] = r.N[l]; fits = fits && (l >= tr->n_levels || r.N[l] <= A.cap[l]); }
        e.slot = -1;
        if (fits) { ids[(size_t)i] = next; e.slot = (int)(next % A.capacity); next++; }
    }
    /* more key frames than the ring has slots: the blob's earliest are evicted by its later ones and need not be copied */
    for (int i = 0; i < n; i++)
        if (ids[(size_t)i] >= 0 && ids[(size_t)i] + A.capacity < next) A.h_bent[i].slot = -1;
    TRKHIP(hipMemsetAsync(A.d_bsum, 0, sizeof(unsigned long long) * (size_t)n, c->stream));
    TRKHIP(hipMemcpyAsync(A.d_blob, blob, bytes, hipMemcpyHostToDevice, c->stream));
    TRKHIP(hipMemcpyAsync(A.d_bent, A.h_bent, sizeof(BlobEntry) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_archive_blob_sums(A.d_bent, n, A.d_blob, A.d_bsum, c->stream));
    TRKHIP(hipMemcpyAsync(A.h_bsum, A.d_bsum, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    for (int i = 0; i < n; i++)
        if (A.h_bsum[i] != table[(size_t)i].payload_checksum)
            return tfail(tr, DVO_ERR_INVALID, "archive blob: key frame " + std::to_string(i) + ": the payload checksum does not match");
    /* every check passed: the host's side of the ring, then the scatter (ordered on the stream, no wait) */
    for (int i = 0; i < n; i++) {
        const dvo_blob::Record &r = table[(size_t)i];
        const long long id = ids[(size_t)i];
        if (id < 0) { A.n_refused++; continue; }
        dvo_tracker::Archive::Meta &M = A.slot[(size_t)(id % A.capacity)];
        if (M.id >= 0) {
            A.n_evicted++;
            for (long long &k : A.key_id) if (k == M.id) k = -1;
        }
        M = dvo_tracker::Archive::Meta();
        M.id = id; M.stream = -1; M.frame = (long)r.origin_frame;
        M.K = make_float4(r.K[0], r.K[1], r.K[2], r.K[3]);
        for (int l = 0; l < DVO_LEVELS; l++) M.N[l] = r.N[l];
        M.has_desc = A.h_bent[i].has_desc != 0;
        M.origin_id = r.origin_id; M.origin_stream = r.origin_stream; M.origin_frame = r.origin_frame;
        A.n_archived++;
    }
    A.next_id = next;
    TRKHIP(launch_archive_import(A.d_bent, n, A.d_blob, A.view, A.pl.view, c->stream));
    for (int i = 0; i < std::min(n, ids_capacity); i++) ids_out[i] = ids[(size_t)i];
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_archive_origin(dvo_tracker *tr, long long id, long long *origin_id, int *origin_stream, long long *origin_frame) {
    if (!tr) return DVO_ERR_INVALID;
    const dvo_tracker::Archive::Meta *M = archive_find(tr, id);
    if (!M) return tfail(tr, DVO_ERR_STATE, tr->ar.on ? "key frame " + std::to_string(id) + " is not in the archive (unknown or evicted)"
                                                       : std::string(kArchiveOff));
    if (origin_id) *origin_id = M->origin_id;
    if (origin_stream) *origin_stream = M->origin_stream;
    if (origin_frame) *origin_frame = M->origin_frame;
    return DVO_OK;
}

int dvo_tracker_score(dvo_tracker *tr, int n, const int *stream, const long long *key_id, int level, const double *R, const double *t,
                      dvo_tracker_score_record *records) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = check_candidates(tr, n, stream, key_id, R, t, records);
    if (rc) return rc;
    if (level < 0 || level >= tr->n_levels) return tfail(tr, DVO_ERR_INVALID, "level out of range");
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    for (int i = 0; i < n; i++) {
        int slot = 0;
        (void)archive_find(tr, key_id[i], &slot);
        A.h_cand[i] = ScoreCand{slot, stream[i], i, 0};
        std::memcpy(A.h_cpose + 12 * (size_t)i, R + 9 * (size_t)i, sizeof(double) * 9);
        std::memcpy(A.h_cpose + 12 * (size_t)i + 9, t + 3 * (size_t)i, sizeof(double) * 3);
    }
    TRKHIP(hipMemcpyAsync(A.d_cand, A.h_cand, sizeof(ScoreCand) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(hipMemcpyAsync(A.d_cpose, A.h_cpose, sizeof(double) * 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_archive_score(A.d_cand, n, A.d_cpose, A.view, slab_of(c, level), level, c->K, native_compact_wanted(c), A.d_rec, c->stream));
    TRKHIP(hipMemcpyAsync(A.h_rec, A.d_rec, sizeof(ScoreRecord) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    for (int i = 0; i < n; i++) expand_record(A.h_rec[i], records[i]);
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_match(dvo_tracker *tr, int n, const int *stream, const long long *key_id, const double *R0, const double *t0, double *R,
                      double *t, dvo_tracker_score_record *records) {
    if (!tr) return DVO_ERR_INVALID;
    int rc = check_candidates(tr, n, stream, key_id, R0, t0, records);
    if (rc) return rc;
    if (!R || !t) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    dvo_ctx *mc = A.mc;
    if (!c->have_K) return tfail(tr, DVO_ERR_STATE, "intrinsics not set (dvo_tracker_set_intrinsics)");
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    auto MC = [&](int r) { if (r != DVO_OK) tr->err = mc->err; return r; };
    /* which 16-byte texels travel, decided before anything is written: tex_mask bit l = the host knows they are the image's real form;
     * bit 8 + l = the host does not know yet (a compact form it has not looked at) and the match slab is sparse: the destination gets
     * memory and the load kernel decides from the device's pal_n.  No read-back, and the tracker's context is only read */
    for (int i = 0; i < n; i++) {
        int mask = 0;
        for (int l = 0; l < tr->n_levels; l++) {
            const Level &S = c->lv[l], &D = mc->lv[l];
            const int p = stream[i];
            const bool tex_real = S.now[p].texels_real();
            const bool unknown = !tex_real && D.tex_sparse && S.now[p].host_unknown();
            if (tex_real) mask |= 1 << l;
            else if (unknown) mask |= 1 << (8 + l);
            if ((tex_real || unknown) && (rc = MC(map_texels(mc, l, i, 1, c->stream)))) return rc;
        }
        A.h_load[i].tex_mask = mask;
    }
    /* the match context follows the tracker's: its stream (one order for the copies, the alignment and the scoring) and its camera models */
    mc->stream = c->stream;
    if (c->d_pair_K && !mc->d_pair_K) {                    /* per-stream models appeared: the table is made once (one wait of its own) */
        mc->K = Intrinsics{c->K.fx, c->K.fy, c->K.cx, c->K.cy, c->K.interp, 0, nullptr};
        mc->have_K = true;
        if ((rc = MC(pair_intrinsics_set(mc, 0, true, c->K.fx, c->K.fy, c->K.cx, c->K.cy)))) return rc;
    }
    mc->K = Intrinsics{c->K.fx, c->K.fy, c->K.cx, c->K.cy, c->K.interp, 0, mc->d_pair_K};
    mc->have_K = true;
    mc->host_changed();
    ArchiveDst dst{};
    LevelSet now;
    for (int l = 0; l < DVO_LEVELS; l++) now.l[l] = slab_of(c, l);
    for (int i = 0; i < n; i++) {
        int slot = 0;
        const dvo_tracker::Archive::Meta *M = archive_find(tr, key_id[i], &slot);
        ArchiveLoad &ld = A.h_load[i];
        ld.slot = slot; ld.now_pair = stream[i]; ld.dst = i;
        std::memcpy(ld.pose, R0 + 9 * (size_t)i, sizeof(double) * 9);
        std::memcpy(ld.pose + 9, t0 + 3 * (size_t)i, sizeof(double) * 3);
        if (mc->d_pair_K) { mc->h_pair_K[i] = M->K; mc->pair_K_own[i] = 1; }      /* the device's entry is written by the load launch */
        for (int l = 0; l < tr->n_levels; l++) {
            const Level &S = c->lv[l];
            Level &D = mc->lv[l];
            const int p = stream[i];
            const bool tex_real = (ld.tex_mask >> l) & 1;
            /* the pair's host state: the slot's list, the stream's now level in the form(s) it has */
            D.hN.w(i) = M->N[l];
            D.compact_ok.w(i) = 1;
            ref_list_written(mc, l, i, 1, tr->lr[l]);
            D.now.w(i).adopt_for_match(S.now[p], tex_real, D.p4 != nullptr);
        }
    }
    for (int l = 0; l < tr->n_levels; l++) {
        const Level &D = mc->lv[l];
        ArchiveDst::Lv &o = dst.l[l];
        o.cpts = D.cpts; o.cidx = D.cidx; o.cpt4 = D.cpt4; o.chdr = D.chdr; o.pt4_ok = D.d_pt4_ok; o.N = D.dN; o.pt_cap = D.pt_cap;
        o.tex_dense = D.tex_sparse ? 0 : 1;
        o.tex = D.tex; o.p4 = D.p4; o.pal = D.pal; o.pal_n = D.d_pal_n;
    }
    dst.poses = mc->d_poses; dst.pair_K = mc->d_pair_K;
    TRKHIP(hipMemcpyAsync(A.d_load, A.h_load, sizeof(ArchiveLoad) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_archive_load(A.d_load, n, A.view, now, dst, c->stream));
    /* the tracker's level schedule for every candidate: ONE launch through the index list 0 .. n - 1 */
    if ((rc = MC(enqueue_pair_list(mc, A.h_iota.data(), A.d_iota, n, tr->n_levels, tr->tp.iters, 0)))) return rc;
    /* the records at the resulting poses, on the finest level that ran, against the streams' now levels where they are */
    for (int i = 0; i < n; i++) A.h_cand[i] = ScoreCand{A.h_load[i].slot, stream[i], i, 0};
    TRKHIP(hipMemcpyAsync(A.d_cand, A.h_cand, sizeof(ScoreCand) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_archive_score(A.d_cand, n, mc->d_poses, A.view, slab_of(c, tr->last_level), tr->last_level, c->K, native_compact_wanted(c), A.d_rec,
                                c->stream));
    TRKHIP(hipMemcpyAsync(A.h_cpose, mc->d_poses, sizeof(double) * 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(hipMemcpyAsync(A.h_rec, A.d_rec, sizeof(ScoreRecord) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    for (int i = 0; i < n; i++) {
        std::memcpy(R + 9 * (size_t)i, A.h_cpose + 12 * (size_t)i, sizeof(double) * 9);
        std::memcpy(t + 3 * (size_t)i, A.h_cpose + 12 * (size_t)i + 9, sizeof(double) * 3);
        expand_record(A.h_rec[i], records[i]);
    }
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_verify_params_default(dvo_tracker_verify_params *vp) {
    if (!vp) return DVO_ERR_INVALID;
    /* parameters for a structured-light sensor (depth noise grows with range), not measured values */
    vp->tol_mm = 25.0f; vp->tol_rel = 0.02f; vp->min_depth_mm = 1.0f; vp->max_depth_mm = 65535.0f;
    return DVO_OK;
}

int dvo_tracker_verify(dvo_tracker *tr, int n, const int *stream, const long long *key_id, int level, const double *R, const double *t,
                       const dvo_tracker_verify_params *vpp, dvo_tracker_verify_record *records) {
    if (!tr) return DVO_ERR_INVALID;
    static_assert(sizeof(VerifyRecord) == sizeof(dvo_tracker_verify_record) && sizeof(VerifyTol) == sizeof(dvo_tracker_verify_params),
                  "the verification kernel reads dvo_tracker_verify_params and writes dvo_tracker_verify_record");
    int rc = check_candidates(tr, n, stream, key_id, R, t, records);
    if (rc) return rc;
    if (level < 0 || level >= tr->n_levels) return tfail(tr, DVO_ERR_INVALID, "level out of range");
    dvo_tracker_verify_params vp;
    if (vpp) vp = *vpp; else dvo_tracker_verify_params_default(&vp);
    /* written so that a NaN fails each test */
    if (!(vp.tol_mm >= 0.0f) || !(vp.tol_rel >= 0.0f) || !(vp.min_depth_mm < vp.max_depth_mm))
        return tfail(tr, DVO_ERR_INVALID, "bad verification parameters: tol_mm >= 0, tol_rel >= 0 and min_depth_mm < max_depth_mm are needed, no NaN");
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    const FrameLevel &F = c->fs.lv[level];
    for (int i = 0; i < n; i++) {
        const dvo_tracker::Stream &S = tr->st[stream[i]];
        const int fs = S.bank * tr->K + stream[i];
        if (S.bank < 0 || level >= c->fs.n_levels || !F.depth.get() || (size_t)fs >= c->fs.valid.size() || !c->fs.valid[fs] || !c->fs.has_depth[fs])
            return tfail(tr, DVO_ERR_STATE, "the current frame of stream " + std::to_string(stream[i]) + " has no depth plane in the frame store");
    }
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    for (int i = 0; i < n; i++) {
        int slot = 0;
        (void)archive_find(tr, key_id[i], &slot);
        A.h_vcand[i] = VerifyCand{slot, tr->st[stream[i]].bank * tr->K + stream[i], i, 0};
        std::memcpy(A.h_cpose + 12 * (size_t)i, R + 9 * (size_t)i, sizeof(double) * 9);
        std::memcpy(A.h_cpose + 12 * (size_t)i + 9, t + 3 * (size_t)i, sizeof(double) * 3);
    }
    const VerifyDepth D{F.depth.get(), F.npx, c->fs.n_slots, F.rows, F.cols, 0};
    const VerifyTol T{vp.tol_mm, vp.tol_rel, vp.min_depth_mm, vp.max_depth_mm};
    TRKHIP(hipMemcpyAsync(A.d_vcand, A.h_vcand, sizeof(VerifyCand) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(hipMemcpyAsync(A.d_cpose, A.h_cpose, sizeof(double) * 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_archive_verify(A.d_vcand, n, A.d_cpose, A.view, D, level, c->K, T, A.d_vfy, c->stream));
    TRKHIP(hipMemcpyAsync(A.h_vfy, A.d_vfy, sizeof(VerifyRecord) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    std::memcpy(records, A.h_vfy, sizeof(VerifyRecord) * (size_t)n);
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_set_places(dvo_tracker *tr, int level) {
    if (!tr) return DVO_ERR_INVALID;
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    if (!A.on) return tfail(tr, DVO_ERR_STATE, "the key-frame archive is off (dvo_tracker_set_archive)");
    if (level < -1 || level >= tr->n_levels) return tfail(tr, DVO_ERR_INVALID, "level out of range (-1 switches places off)");
    const long long D = level >= 0 ? (long long)tr->lr[level] * tr->lc[level] : 0;
    if (D > DVO_PLACE_MAX_D)
        return tfail(tr, DVO_ERR_INVALID, "the descriptor level has " + std::to_string(D) + " pixels, more than " + std::to_string(DVO_PLACE_MAX_D) +
                                              " (120 x 160): choose a coarser level");
    DeviceGuard g(c);
    TRKHIP(stream_wait(c->stream));
    places_release(tr);                                    /* switching on again starts without descriptors */
    if (level < 0) return DVO_OK;
    dvo_tracker::Archive::Places &P = A.pl;
    auto setup = [&]() -> int {
        const size_t S = (size_t)A.capacity, K = (size_t)tr->K;
        P.level = level;
        P.view.n_slots = A.capacity; P.view.D = (int)D; P.view.stride = (int)((D + 15) / 16 * 16);
        TRKHIP(P.desc.alloc(S * (size_t)P.view.stride));
        TRKHIP(P.mark.alloc(S));
        P.view.desc = P.desc.get(); P.view.mark = P.mark.get();
        TRKHIP(hipMemsetAsync(P.view.mark, 0, sizeof(int) * S, c->stream));
        TRKHIP(P.d_ent.alloc(2 * K));
        TRKHIP(P.h_ent.alloc(2 * K));
        TRKHIP(P.d_query.alloc(K));
        TRKHIP(P.h_query.alloc(K));
        TRKHIP(P.d_dist.alloc(K * S));
        const size_t out_bytes = (sizeof(PlaceOut) * DVO_TRACKER_PLACES_MAX_K + sizeof(int)) * K;
        TRKHIP(P.d_out.alloc(out_bytes));
        TRKHIP(P.h_out.alloc(out_bytes));
        TRKHIP(P.d_scand.alloc(K * DVO_TRACKER_PLACES_MAX_K));
        TRKHIP(P.h_scand.alloc(K * DVO_TRACKER_PLACES_MAX_K));
        TRKHIP(P.d_shift.alloc(K * DVO_TRACKER_PLACES_MAX_K));
        TRKHIP(P.h_shift.alloc(K * DVO_TRACKER_PLACES_MAX_K));
        TRKHIP(stream_wait(c->stream));
        return DVO_OK;
    };
    const int rc = setup();
    if (rc) {
        const std::string msg = tr->err;
        places_release(tr);
        return tfail(tr, rc, msg);
    }
    P.on = true;
    return DVO_OK;
}

int dvo_tracker_archive_get_descriptor(dvo_tracker *tr, long long id, unsigned char *out, int capacity, int *D_out) {
    if (!tr) return DVO_ERR_INVALID;
    const dvo_tracker::Archive::Places &P = tr->ar.pl;
    if (!P.on) return tfail(tr, DVO_ERR_STATE, "place descriptors are off (dvo_tracker_set_places)");
    int slot = 0;
    const dvo_tracker::Archive::Meta *M = archive_find(tr, id, &slot);
    if (!M) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(id) + " is not in the archive (unknown or evicted)");
    if (!M->has_desc) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(id) + " was archived while place descriptors were off");
    if (D_out) *D_out = P.view.D;
    const int ncopy = std::min(P.view.D, capacity);
    if (out && ncopy > 0) {
        dvo_ctx *c = tr->ctx;
        DeviceGuard g(c);
        TRKHIP(hipMemcpyAsync(out, P.view.desc + (size_t)slot * P.view.stride, (size_t)ncopy, hipMemcpyDeviceToHost, c->stream));
        TRKHIP(stream_wait(c->stream));
    }
    return DVO_OK;
}

int dvo_tracker_query_places(dvo_tracker *tr, int n, const int *streams, int k, long long min_frame_gap, dvo_tracker_place *out,
                             int *n_found) {
    if (!tr) return DVO_ERR_INVALID;
    static_assert(sizeof(PlaceOut) == sizeof(dvo_tracker_place), "the selection kernel writes dvo_tracker_place records");
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    dvo_tracker::Archive::Places &P = A.pl;
    if (!P.on) return tfail(tr, DVO_ERR_STATE, "place descriptors are off (dvo_tracker_set_places)");
    if (n < 1 || n > tr->K) return tfail(tr, DVO_ERR_INVALID, "n must be in [1, max_streams]");
    if (k < 1 || k > DVO_TRACKER_PLACES_MAX_K) return tfail(tr, DVO_ERR_INVALID, "k must be in [1, DVO_TRACKER_PLACES_MAX_K]");
    if (min_frame_gap < 0) return tfail(tr, DVO_ERR_INVALID, "min_frame_gap must be >= 0");
    if (!streams || !out) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    std::vector<char> seen(tr->K, 0);
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        if (s < 0 || s >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(s) + " out of range");
        if (seen[s]) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(s) + " listed twice");
        seen[s] = 1;
    }
    for (int i = 0; i < n; i++) {
        const dvo_tracker::Stream &S = tr->st[streams[i]];
        if (!S.started || S.bank < 0 || (size_t)(S.bank * tr->K + streams[i]) >= c->fs.valid.size() || !c->fs.valid[S.bank * tr->K + streams[i]])
            return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(streams[i]) + " has not been stepped yet: it has no current frame");
    }
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        const dvo_tracker::Stream &S = tr->st[s];
        const Intrinsics Ks = intrinsics_of(c, s);
        int own = -1;
        if (!archive_find(tr, A.key_id[s], &own)) own = -1;
        P.h_query[i] = PlaceQuery{S.bank * tr->K + s, s, own, 0, (long long)S.n_frame - 1, make_float4(Ks.fx, Ks.fy, Ks.cx, Ks.cy)};
    }
    PlaceOut *d_rows = reinterpret_cast<PlaceOut *>(P.d_out.get());
    int *d_found = reinterpret_cast<int *>(P.d_out + sizeof(PlaceOut) * (size_t)n * k);
    const size_t out_bytes = sizeof(PlaceOut) * (size_t)n * k + sizeof(int) * (size_t)n;
    TRKHIP(hipMemcpyAsync(P.d_query, P.h_query, sizeof(PlaceQuery) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_place_query(P.d_query, n, k, min_frame_gap, A.next_id - A.capacity, place_grey(tr), P.view, A.view.hdr, P.d_dist, d_rows,
                              d_found, c->stream));
    TRKHIP(hipMemcpyAsync(P.h_out, P.d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    std::memcpy(out, P.h_out, sizeof(PlaceOut) * (size_t)n * k);
    if (n_found) std::memcpy(n_found, P.h_out + sizeof(PlaceOut) * (size_t)n * k, sizeof(int) * (size_t)n);
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_place_shifts(dvo_tracker *tr, int n, const int *stream, const long long *key_id, int radius,
                             dvo_tracker_place_shift *records) {
    if (!tr) return DVO_ERR_INVALID;
    static_assert(sizeof(PlaceShiftOut) == sizeof(dvo_tracker_place_shift), "the shift kernel writes dvo_tracker_place_shift records");
    static_assert(DVO_PLACE_SHIFT_MAX_R == DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS, "one maximum radius");
    dvo_ctx *c = tr->ctx;
    dvo_tracker::Archive &A = tr->ar;
    dvo_tracker::Archive::Places &P = A.pl;
    if (!P.on) return tfail(tr, DVO_ERR_STATE, "place descriptors are off (dvo_tracker_set_places)");
    if (n < 1 || n > tr->K * DVO_TRACKER_PLACES_MAX_K) return tfail(tr, DVO_ERR_INVALID, "n must be in [1, max_streams * DVO_TRACKER_PLACES_MAX_K]");
    if (!stream || !key_id || !records) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    const int rows = tr->lr[P.level], cols = tr->lc[P.level];
    if (radius < 0 || radius > DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS)
        return tfail(tr, DVO_ERR_INVALID, "radius must be in [0, DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS]");
    if (rows - 2 * radius < 1 || cols - 2 * radius < 1)
        return tfail(tr, DVO_ERR_INVALID, "radius " + std::to_string(radius) + " leaves no window in the " + std::to_string(rows) + " x " +
                                              std::to_string(cols) + " descriptor level");
    for (int i = 0; i < n; i++)
        if (stream[i] < 0 || stream[i] >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(stream[i]) + " out of range");
    for (int i = 0; i < n; i++) {
        const int s = stream[i];
        const dvo_tracker::Stream &S = tr->st[s];
        if (!S.started || S.bank < 0 || (size_t)(S.bank * tr->K + s) >= c->fs.valid.size() || !c->fs.valid[S.bank * tr->K + s])
            return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(s) + " has not been stepped yet: it has no current frame");
        const dvo_tracker::Archive::Meta *M = archive_find(tr, key_id[i]);
        if (!M) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " is not in the archive (unknown or evicted)");
        if (!M->has_desc) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " was archived while place descriptors were off");
    }
    for (int i = 0; i < n; i++) {
        const Intrinsics Ks = intrinsics_of(c, stream[i]);
        const float4 k = make_float4(Ks.fx, Ks.fy, Ks.cx, Ks.cy);
        if (std::memcmp(&k, &archive_find(tr, key_id[i])->K, sizeof(float4)) != 0)
            return tfail(tr, DVO_ERR_INVALID, "key frame " + std::to_string(key_id[i]) + " was enlisted under another camera model than stream " +
                                                  std::to_string(stream[i]) + "'s");
    }
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    for (int i = 0; i < n; i++) {
        int slot = 0;
        (void)archive_find(tr, key_id[i], &slot);
        P.h_scand[i] = PlaceShiftCand{slot, tr->st[stream[i]].bank * tr->K + stream[i]};
    }
    TRKHIP(hipMemcpyAsync(P.d_scand, P.h_scand, sizeof(PlaceShiftCand) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_place_shifts(P.d_scand, n, rows, cols, radius, place_grey(tr), P.view, P.d_shift, c->stream));
    TRKHIP(hipMemcpyAsync(P.h_shift, P.d_shift, sizeof(PlaceShiftOut) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TRKHIP(stream_wait(c->stream));
    std::memcpy(records, P.h_shift, sizeof(PlaceShiftOut) * (size_t)n);
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_place_guess(dvo_tracker *tr, int stream, int dy, int dx, double *R0, double *t0) {
    if (!tr) return DVO_ERR_INVALID;
    const dvo_tracker::Archive::Places &P = tr->ar.pl;
    if (!P.on) return tfail(tr, DVO_ERR_STATE, "place descriptors are off (dvo_tracker_set_places)");
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(stream) + " out of range");
    if (!R0 || !t0) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    const int mr = DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS;
    if (dy < -mr || dy > mr || dx < -mr || dx > mr)
        return tfail(tr, DVO_ERR_INVALID, "|dy| and |dx| must be at most DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS");
    if (!tr->ctx->have_K) return tfail(tr, DVO_ERR_STATE, "intrinsics not set (dvo_tracker_set_intrinsics)");
    const Intrinsics Ks = intrinsics_of(tr->ctx, stream);
    place_guess(Ks.fx, Ks.fy, tr->tp.first_shift + P.level, dy, dx, R0, t0);
    return DVO_OK;
}

int dvo_tracker_get_stats(dvo_tracker *tr, int *kernel_launches, int *host_syncs, int *runs, int *key_frames, int *slab_growths) {
    if (!tr) return DVO_ERR_INVALID;
    if (kernel_launches) *kernel_launches = tr->s_launches;
    if (host_syncs) *host_syncs = tr->s_syncs;
    if (runs) *runs = tr->s_runs;
    if (key_frames) *key_frames = tr->s_keys;
    if (slab_growths) *slab_growths = tr->s_growths;
    return DVO_OK;
}

dvo_ctx *dvo_tracker_context(dvo_tracker *tr) { return tr ? tr->ctx : nullptr; }

}  // extern "C"
