/*
 * dvo_capi_tracker.cpp -- the multi-stream tracker of the C ABI (include/dvo_amd.h, "many camera streams"): K camera streams,
 * each following SolveDVO::loop (SolveDVO.cpp:1970-2241) as dvo_amd::SolveDVO does for one camera, advanced together by
 * batched calls of the frame store and the fused alignment.  Host side only; the key-frame rule and the pose gather run in
 * dvo_tracker.hip.  Creation, the stream set-up, the steps, signals, information, views and stats; the state and the shared helpers
 * are dvo_tracker_host.h, the archive dvo_capi_tracker_archive.cpp, the places dvo_capi_tracker_places.cpp.
 */
#include "dvo_depth_register.h"
#include "dvo_tracker_host.h"

using namespace dvo;
using namespace dvo_host;

static_assert(PLAN_TRK_FORCED == DVO_TRK_FORCED && PLAN_TRK_MAY_SWITCH == DVO_TRK_MAY_SWITCH, "dvo_tracker_plan.h restates DVO_TRK_* of dvo_launch.h");

namespace {

int level_size(int n, int shift) {                     /* cv::resize(Size(), s, s): cvRound(n * 2^-shift), half to even */
    return (int)std::nearbyint(std::ldexp((double)n, -shift));
}

using Uploader = std::function<int(const std::vector<int> &idx, int slot0, int pair0)>;

/* one step on its way through the stages below */
struct StepRun {
    dvo_tracker *tr;
    dvo_ctx *c;
    StepPlan plan;                                         /* dvo_tracker_plan.h: banks, first / align, upload runs, flags */
    int nA, nF;                                            /* aligned streams, streams on their first frame */
    bool team;                                             /* a team launch ran since the last wait */
};

/* frames: upload + pyramid + Canny, installed as the streams' now frames -- one call per run */
int upload_runs(StepRun &r, const Uploader &upload) {
    dvo_tracker *tr = r.tr;
    const StepPlan &P = r.plan;
    for (const std::pair<size_t, size_t> &run : P.upload_runs) {
        tr->s_runs++;
        const std::vector<int> idx(P.order.begin() + run.first, P.order.begin() + run.second);
        TRK(upload(idx, P.bank_of[idx[0]] * tr->K + P.stream_of[idx[0]], P.stream_of[idx[0]]));
    }
    return DVO_OK;
}

/* reference extraction of any set of streams (entries `set`, frames in bank bank[i]): ONE call of the index-list form, whose
 * launches cover the whole set; its one host synchronisation reads the point counts */
int extract(StepRun &r, const std::vector<int> &set, const std::vector<int> &bank, int map_off) {
    dvo_tracker *tr = r.tr;
    if (set.empty()) return DVO_OK;
    tr->s_runs++;
    const int n = (int)set.size();
    std::vector<int> slots(n), pairs(n);
    for (int k = 0; k < n; k++) {
        pairs[k] = r.plan.stream_of[set[k]];
        slots[k] = bank[set[k]] * tr->K + pairs[k];
        tr->h_map[map_off + k] = make_int2(slots[k], pairs[k]);
    }
    TRKHIP(hipMemcpyAsync(tr->d_map + map_off, tr->h_map + map_off, sizeof(int2) * (size_t)n, hipMemcpyHostToDevice, r.c->stream));
    return tchk(tr, frames_as_ref_list(r.c, slots.data(), pairs.data(), tr->d_map + map_off, n, nullptr));
}

/* the key-frame archive (dvo_tracker_archive.hip): the lists `extract` has just written for `set` go to the next slots of the ring
 * (dvo_key_ring.h; planned and committed at once) -- ONE launch, ordered on the stream, no wait; the host knows the counts from the
 * extraction's own synchronisation.  Key frames that a later one of the same set overwrites are not written */
int archive_store(StepRun &r, const std::vector<int> &set, const std::vector<int> &bank, int off, bool is_first) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    dvo_tracker::Archive &A = tr->ar;
    if (!A.on || set.empty()) return DVO_OK;
    std::vector<char> fits(set.size(), 1);
    std::vector<KeyRing::Meta> meta(set.size());
    for (size_t j = 0; j < set.size(); j++) {
        const int p = r.plan.stream_of[set[j]];
        const Intrinsics Ks = intrinsics_of(c, p);
        KeyRing::Meta &M = meta[j];
        M.stream = M.origin_stream = p;                    /* a native key frame is its own origin */
        M.frame = is_first ? 0 : tr->st[p].n_frame - 1;
        M.origin_frame = M.frame;
        M.K[0] = Ks.fx; M.K[1] = Ks.fy; M.K[2] = Ks.cx; M.K[3] = Ks.cy;
        M.has_desc = A.pl.on;
        for (int l = 0; l < tr->n_levels; l++) {
            M.N[l] = c->lv[l].hN[p];
            fits[j] = fits[j] && M.N[l] <= A.cap[l];
        }
    }
    const KeyRing::Plan plan = A.ring.plan(fits.data(), (int)set.size());
    int n = 0;
    for (size_t j = 0; j < set.size(); j++) {
        const KeyRing::Planned &k = plan.item[j];
        meta[j].origin_id = k.id;
        if (!k.written) continue;
        const KeyRing::Meta &M = meta[j];
        if (A.pl.on) A.pl.h_ent[off + n] = PlaceEntry{bank[set[j]] * tr->K + M.stream, k.slot};      /* the frame that has just become the reference */
        A.h_store[off + n++] = ArchiveStore{M.stream, k.slot, (long long)M.frame, make_float4(M.K[0], M.K[1], M.K[2], M.K[3])};
    }
    A.ring.commit(plan, meta.data());
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
}

/* the level schedule for any set of streams: ONE fused launch through its index list (the packed kernel's launch order), or, for
 * the one-point-per-lane kernel (dvo_params.engine_variant = 1 / interpolate_dt), one launch per run of consecutive streams */
int align_set(StepRun &r, const std::vector<int> &set, int list_off, int aflags) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    if (set.empty()) return DVO_OK;
    const int n = (int)set.size();
    if (fused_uses_compact(c->prm.points_in_flight, c->prm.interpolate_dt) && c->prm.engine_variant != 1) {
        tr->s_runs++;
        for (int k = 0; k < n; k++) tr->h_pairs[list_off + k] = r.plan.stream_of[set[k]];
        TRKHIP(hipMemcpyAsync(tr->d_pairs + list_off, tr->h_pairs + list_off, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        const int rc = enqueue_pair_list(c, tr->h_pairs + list_off, tr->d_pairs + list_off, n, tr->n_levels, tr->tp.iters, aflags);
        r.team = r.team || c->team_used;
        return tchk(tr, rc);
    }
    return tchk(tr, for_runs(set, r.plan.stream_of, r.plan.bank_of, false, [&](size_t a, size_t b) {
        tr->s_runs++;
        const int rc = dvo_align_batch_enqueue(c, r.plan.stream_of[set[a]], (int)(b - a), tr->n_levels, tr->tp.iters, aflags);
        r.team = r.team || c->team_used;
        return rc;
    }));
}

/* the step's entry list (aligned streams with the host's part of the key-frame rule, then first frames), the identity poses of the
 * first frames (processFirstFrame) and, for the views, the frame-store slot of every listed stream */
int entry_lists(StepRun &r) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    const StepPlan &P = r.plan;
    const int nA = r.nA, nF = r.nF;
    for (int k = 0; k < nA; k++) tr->h_list[k] = TrackerEntry{P.stream_of[P.align[k]], P.flags[k]};
    for (int k = 0; k < nF; k++) tr->h_list[nA + k] = TrackerEntry{P.stream_of[P.first[k]], 0};
    TRKHIP(hipMemcpyAsync(tr->d_list, tr->h_list, sizeof(TrackerEntry) * (size_t)(nA + nF), hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_tracker_reset_listed(tr->d_list + nA, nF, c->d_poses, c->stream));
    if (!tr->views_on) return DVO_OK;
    for (int k = 0; k < nA + nF; k++) {
        const int i = k < nA ? P.align[k] : P.first[k - nA];
        tr->h_vslot[k] = P.bank_of[i] * tr->K + P.stream_of[i];
    }
    TRKHIP(hipMemcpyAsync(tr->d_vslot, tr->h_vslot, sizeof(int) * (size_t)(nA + nF), hipMemcpyHostToDevice, c->stream));
    return DVO_OK;
}

/* signals + key-frame rule + poses of every aligned stream: one launch, one read */
int signals(StepRun &r) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    const Level &Lf = c->lv[tr->last_level];
    const bool with_eps = tr->tp.adaptive != 0;
    const bool blk = with_eps && c->sched.final_blk;
    if (blk && (size_t)r.nA * c->final_cap > tr->d_scratch.size()) {
        TRKHIP(stream_wait(c->stream));
        TRKHIP(tr->d_scratch.alloc((size_t)tr->K * c->final_cap));
    }
    const TrackerRule rule{tr->tp.adaptive, tr->tp.laplacian_b_thresh, tr->tp.visible_ratio_thresh, tr->tp.min_points};
    TRKHIP(launch_tracker_signals(tr->d_list, r.nA, c->d_poses, c->d_ratio, tr->last_level, with_eps ? c->d_final_N : Lf.dN,
                                  with_eps ? c->d_final_eps : nullptr, blk ? Lf.cidx : nullptr, c->final_cap, Lf.pt_cap,
                                  tr->d_scratch, c->final_cap, rule, tr->d_out, c->stream));
    TRKHIP(hipMemcpyAsync(tr->h_out, tr->d_out, sizeof(TrackerOut) * (size_t)r.nA, hipMemcpyDeviceToHost, c->stream));
    return DVO_OK;
}

/* the pose information of the aligned streams (dvo_tracker_info.hip), if it is on: ONE launch over the list -- of the entries that did
 * not switch key frame (switched = 0, after the signals kernel wrote their events) or of those that did (1, after their re-run) -- and
 * the records' copy, which the step's next wait covers */
int information(StepRun &r, int switched) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    if (!tr->info_on) return DVO_OK;
    TRKHIP(launch_tracker_information(tr->d_list, tr->d_out, switched, r.nA, c->d_poses, slab_of(c, tr->last_level), tr->last_level, c->K,
                                      native_compact_wanted(c), tr->d_info, c->stream));
    TRKHIP(hipMemcpyAsync(tr->h_info, tr->d_info, sizeof(TrackerInfo) * (size_t)r.nA, hipMemcpyDeviceToHost, c->stream));
    return DVO_OK;
}

/* the debug views of the listed streams (dvo_tracker_views.hip), if they are on: one rendering = TWO launches over the list, with the
 * filter of information() -- switched = 0 also covers the streams on their first frame (backgrounds only) -- and the histogram
 * records' copy */
int views(StepRun &r, int switched) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    if (!tr->views_on) return DVO_OK;
    const int nA = r.nA, nF = r.nF;
    const FrameLevel &F = c->fs.lv[tr->last_level];
    TRKHIP(launch_tracker_views(tr->d_list, tr->d_out, tr->d_vslot, nA, switched ? nA : nA + nF, switched, c->d_poses,
                                slab_of(c, tr->last_level), tr->last_level, c->K, native_compact_wanted(c), F.grey, F.npx, tr->d_views, tr->view_stride,
                                tr->view_stride * (size_t)tr->K, tr->d_vrec, c->stream));
    TRKHIP(hipMemcpyAsync(tr->h_vrec, tr->d_vrec, sizeof(TrackerViewRecord) * (size_t)(nA + nF), hipMemcpyDeviceToHost, c->stream));
    return DVO_OK;
}

/* key-frame switches (:2198-2232): the previous frame becomes the reference, the estimate the identity, the alignment re-runs; pose
 * information and views of the streams that switched, at the re-run's pose against their new reference; the step's second wait */
int switch_pass(StepRun &r) {
    dvo_tracker *tr = r.tr;
    dvo_ctx *c = r.c;
    const int K = tr->K, nA = r.nA;
    std::vector<int> sw;                                   /* sorted by stream */
    std::vector<int> old_bank(r.plan.stream_of.size());
    for (int k = 0; k < nA; k++) {
        const int i = r.plan.align[k];
        old_bank[i] = tr->st[r.plan.stream_of[i]].bank;
        if (tr->h_out[k].event >= 2) sw.push_back(i);
    }
    if (sw.empty()) return DVO_OK;
    tr->s_keys = (int)sw.size();
    int rc = extract(r, sw, old_bank, K);
    if (rc) return rc;
    if ((rc = archive_store(r, sw, old_bank, K, false))) return rc;
    TRKHIP(launch_tracker_reset_switched(tr->d_list, tr->d_out, nA, c->d_poses, c->stream));
    r.team = false;
    if ((rc = align_set(r, sw, K, 0))) return rc;
    TRKHIP(launch_tracker_gather_switched(tr->d_list, nA, c->d_poses, tr->d_out, c->stream));
    TRKHIP(hipMemcpyAsync(tr->h_out, tr->d_out, sizeof(TrackerOut) * (size_t)nA, hipMemcpyDeviceToHost, c->stream));
    if ((rc = information(r, 1))) return rc;
    if ((rc = views(r, 1))) return rc;
    return wait_team_checked(tr, r.team);
}

/* outputs, the streams' records and their clocks */
void commit_outputs(StepRun &r, double *R_rel, double *t_rel, int *event) {
    dvo_tracker *tr = r.tr;
    for (int k = 0; k < r.nA; k++) {
        const int i = r.plan.align[k];
        const TrackerOut &o = tr->h_out[k];
        std::memcpy(R_rel + 9 * (size_t)i, o.pose, sizeof(double) * 9);
        std::memcpy(t_rel + 3 * (size_t)i, o.pose + 9, sizeof(double) * 3);
        event[i] = o.event;
        dvo_tracker::Stream &S = tr->st[r.plan.stream_of[i]];
        S.have_signals = true;
        S.b_cap = o.b_cap; S.ratio = o.ratio; S.n_points = o.n_points;
        S.have_info = tr->info_on;
        if (tr->info_on) S.info = tr->h_info[k];
        S.have_views = tr->views_on;
        if (tr->views_on) S.vrec = tr->h_vrec[k];
        S.aligned_frame(o.event, r.plan.bank_of[i]);
    }
    for (int i : r.plan.first) {
        for (int k = 0; k < 9; k++) R_rel[9 * (size_t)i + k] = (k % 4 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 3; k++) t_rel[3 * (size_t)i + k] = 0.0;
        event[i] = 1;
        dvo_tracker::Stream &S = tr->st[r.plan.stream_of[i]];
        S = dvo_tracker::Stream();
        S.first_frame(r.plan.bank_of[i]);
        S.have_info = tr->info_on;                         /* no alignment happened: the zero record */
        S.info.level = -1;
        S.have_views = tr->views_on;                       /* plain backgrounds, the zero histogram */
        S.vrec.level = -1;
    }
}

int step_impl(dvo_tracker *tr, int count, const int *streams, const Uploader &upload, double *R_rel, double *t_rel, int *event) {
    dvo_ctx *c = tr->ctx;
    if (!c->have_K) return tfail(tr, DVO_ERR_STATE, "intrinsics not set (dvo_tracker_set_intrinsics)");
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    int cap0[DVO_LEVELS];
    for (int l = 0; l < tr->n_levels; l++) cap0[l] = c->lv[l].pt_cap;
    tr->s_runs = tr->s_keys = tr->s_growths = 0;
    StepRun r{tr, c, plan_step(tr->st, count, streams, tr->tp.key_frame_every), 0, 0, false};
    r.nA = (int)r.plan.align.size();
    r.nF = (int)r.plan.first.size();
    int rc;
    /* 1. frames */
    if ((rc = upload_runs(r, upload))) return rc;
    /* 2. first frames: reference frame + first key frame (processFirstFrame, SolveDVO.cpp:1972-2021) */
    if ((rc = extract(r, r.plan.first, r.plan.bank_of, 0))) return rc;
    if ((rc = archive_store(r, r.plan.first, r.plan.bank_of, 0, true))) return rc;
    if ((rc = entry_lists(r))) return rc;
    /* 3. the other streams: the level schedule from their last estimate (:2097-2104) */
    if ((rc = align_set(r, r.plan.align, 0, tr->tp.adaptive ? DVO_FLAG_FINAL_OUTPUTS : 0))) return rc;
    /* 4. signals of the aligned streams; pose information of those that keep their key frame; their views and those of the first
     * frames: everything rides on one wait */
    if (r.nA > 0) {
        if ((rc = signals(r))) return rc;
        if ((rc = information(r, 0))) return rc;
    }
    if ((rc = views(r, 0))) return rc;
    if ((rc = wait_team_checked(tr, r.team))) return rc;
    /* 5. key-frame switches, with a wait of their own */
    if ((rc = switch_pass(r))) return rc;
    /* 6. outputs and the streams' counters */
    commit_outputs(r, R_rel, t_rel, event);
    for (int l = 0; l < tr->n_levels; l++) tr->s_growths += (c->lv[l].pt_cap != cap0[l]);
    tr->s_launches = (int)(g_kernel_launches - launches0);
    tr->s_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

/* the camera frames of dvo_tracker_step_fmt and dvo_tracker_step_raw_depth */
struct StepFrames {
    const void *const *image, *const *depth;
    int image_format, depth_format, rows, cols;
    const char *flags_refusal;                             /* the call's flags are not among those it takes: the message, else NULL */
};

/* the refusals of the step forms; nothing is changed before they pass */
int check_step(dvo_tracker *tr, int count, const int *streams, const void *R_rel, const void *t_rel, const int *event, const StepFrames *f) {
    if (count < 1 || count > tr->K) return tfail(tr, DVO_ERR_INVALID, "count must be in [1, max_streams]");
    if (!streams || !R_rel || !t_rel || !event) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    if (const int rc = check_stream_list(tr, count, streams)) return rc;
    if (!f) return DVO_OK;
    if (f->image_format < DVO_CAM_BGR8 || f->image_format > DVO_CAM_MONO8 || f->depth_format < DVO_DEPTH_F32 || f->depth_format > DVO_DEPTH_U16)
        return tfail(tr, DVO_ERR_INVALID, "unknown image or depth format (DVO_CAM_* / DVO_DEPTH_*)");
    if (f->rows != tr->tp.rows || f->cols != tr->tp.cols)
        return tfail(tr, DVO_ERR_INVALID, "frame geometry differs from the tracker's (dvo_tracker_params.rows / cols)");
    if (f->flags_refusal) return tfail(tr, DVO_ERR_INVALID, f->flags_refusal);
    if (!f->image || !f->depth) return tfail(tr, DVO_ERR_INVALID, "colour and depth frames are both needed (every frame can become a reference)");
    for (int i = 0; i < count; i++)
        if (!f->image[i] || !f->depth[i]) return tfail(tr, DVO_ERR_INVALID, "NULL camera image");
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
    const StepFrames f{bgr8, depth_m, image_format, depth_format, rows, cols, nullptr};
    const int rc = check_step(tr, count, streams, R_rel, t_rel, event, &f);
    if (rc) return rc;
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
    const StepFrames f{image, depth, image_format, depth_format, rows, cols,
                       (flags & ~DVO_UPLOAD_DEVICE) ? "raw-depth steps take host frames (0) or DVO_UPLOAD_DEVICE" : nullptr};
    int rc = check_step(tr, count, streams, R_rel, t_rel, event, &f);
    if (rc) return rc;
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
    const int rc = check_step(tr, count, streams, R_rel, t_rel, event, nullptr);
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