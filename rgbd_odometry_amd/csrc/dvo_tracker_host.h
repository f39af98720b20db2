/*
 * dvo_tracker_host.h -- the multi-stream tracker's host state (struct dvo_tracker) and what its three host files share: the failure
 * helpers, the step's checked wait and the refusals common to several calls.  dvo_capi_tracker.cpp holds creation, the stream set-up
 * and the steps; dvo_capi_tracker_archive.cpp the key-frame archive, its blobs, score, match and verify; dvo_capi_tracker_places.cpp
 * the place descriptors.  What a tick does with its streams is decided in dvo_tracker_plan.h, the ring rule in dvo_key_ring.h.
 * Internal; not installed.
 */
#ifndef DVO_TRACKER_HOST_H_
#define DVO_TRACKER_HOST_H_

#include "dvo_ctx.h"
#include "dvo_key_ring.h"
#include "dvo_tracker_plan.h"

struct dvo_tracker {
    template <class T> using DevBuf = dvo_host::DevBuf<T>;
    template <class T> using PinnedBuf = dvo_host::PinnedBuf<T>;
    dvo_ctx *ctx = nullptr;
    int K = 0;
    dvo_tracker_params tp{};
    int n_levels = 0, last_level = 0;
    int lr[DVO_LEVELS] = {}, lc[DVO_LEVELS] = {};         /* level geometry */
    struct Stream : dvo_host::StreamClock {
        bool have_signals = false;
        float b_cap = 0.0f, ratio = 0.0f;
        int n_points = 0;
        bool have_info = false;                            /* info describes the pose the stream's last step returned */
        dvo::TrackerInfo info{};
        bool have_views = false;                           /* the stream's images and vrec show the pose its last step returned */
        dvo::TrackerViewRecord vrec{};
    };
    std::vector<Stream> st;
    DevBuf<dvo::TrackerEntry> d_list; PinnedBuf<dvo::TrackerEntry> h_list;
    DevBuf<dvo::TrackerOut> d_out; PinnedBuf<dvo::TrackerOut> h_out;       /* K entries + one slot for the team-mode error word */
    DevBuf<int> d_pairs; PinnedBuf<int> h_pairs;           /* index lists of the alignment launches: aligned streams, then switching ones */
    DevBuf<int2> d_map; PinnedBuf<int2> h_map;             /* {slot, pair} of the reference extractions: first frames, then switches */
    DevBuf<float> d_scratch;
    bool info_on = false;                                  /* dvo_tracker_set_information */
    DevBuf<dvo::TrackerInfo> d_info; PinnedBuf<dvo::TrackerInfo> h_info;   /* one record per listed stream, beside d_out / h_out; allocated when first switched on */
    bool views_on = false;                                 /* dvo_tracker_set_views; everything below is allocated when first switched on */
    DevBuf<unsigned char> d_views;                         /* 2 planes of K images: view v of stream p at d_views + (v * K + p) * view_stride */
    size_t view_stride = 0;                                /* rows * cols * 3 of the finest running level, rounded up to 256 bytes */
    DevBuf<dvo::TrackerViewRecord> d_vrec; PinnedBuf<dvo::TrackerViewRecord> h_vrec;   /* one record per listed stream, like d_info / h_info */
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
     * Everything below but the ring's next id is allocated when the archive is switched on */
    struct Archive {
        bool on = false;
        int max_matches = 0;
        int cap[DVO_LEVELS] = {};                          /* points per slot and level, multiples of 64 */
        dvo_host::KeyRing ring;                            /* ids, slots, evictions, counters: the host's side of the ring */
        dvo::ArchiveView view{};                           /* the kernels' argument: filled once from the buffers below */
        struct LevelBufs { DevBuf<uint2> cpts; DevBuf<unsigned> cidx, cpt4, chdr; } lb[DVO_LEVELS];
        DevBuf<dvo::ArchiveHeader> hdr;
        DevBuf<dvo::ArchiveStore> d_store; PinnedBuf<dvo::ArchiveStore> h_store;    /* 2 K entries: first frames, then switches */
        DevBuf<float> d_xyz;                               /* dvo_tracker_archive_get_points: one decoded list */
        dvo_ctx *mc = nullptr;                             /* max_matches pairs */
        DevBuf<dvo::ArchiveLoad> d_load; PinnedBuf<dvo::ArchiveLoad> h_load;
        DevBuf<dvo::ScoreCand> d_cand; PinnedBuf<dvo::ScoreCand> h_cand;
        DevBuf<double> d_cpose; PinnedBuf<double> h_cpose;   /* dvo_tracker_score: the candidates' poses; dvo_tracker_match: the poses read back */
        DevBuf<dvo::ScoreRecord> d_rec; PinnedBuf<dvo::ScoreRecord> h_rec;
        DevBuf<dvo::VerifyCand> d_vcand; PinnedBuf<dvo::VerifyCand> h_vcand;      /* dvo_tracker_verify: its candidates and records (the poses go through d_cpose) */
        DevBuf<dvo::VerifyRecord> d_vfy; PinnedBuf<dvo::VerifyRecord> h_vfy;
        DevBuf<int> d_iota;
        std::vector<int> h_iota;
        int last_launches = 0, last_syncs = 0;
        /* dvo_tracker_archive_export / _import: the blob's device staging buffer, the entry list and the recomputed payload checksums.
         * Allocated and grown inside those calls, never in a step */
        DevBuf<unsigned char> d_blob;
        DevBuf<dvo::BlobEntry> d_bent; PinnedBuf<dvo::BlobEntry> h_bent;
        DevBuf<unsigned long long> d_bsum; PinnedBuf<unsigned long long> h_bsum;
        /* dvo_tracker_set_places: one descriptor row per slot beside the ring (dvo_tracker_places.hip).  Allocated when switched on */
        struct Places {
            bool on = false;
            int level = -1;
            dvo::PlaceView view{};                                 /* the kernels' argument: desc and mark point into the two buffers below */
            DevBuf<unsigned char> desc;
            DevBuf<int> mark;
            DevBuf<dvo::PlaceEntry> d_ent; PinnedBuf<dvo::PlaceEntry> h_ent;       /* 2 K entries, beside d_store / h_store */
            DevBuf<dvo::PlaceQuery> d_query; PinnedBuf<dvo::PlaceQuery> h_query;   /* K queries */
            DevBuf<unsigned> d_dist;                               /* K x capacity distances */
            DevBuf<unsigned char> d_out; PinnedBuf<unsigned char> h_out;   /* n * k PlaceOut, then n counts: one copy */
            DevBuf<dvo::PlaceShiftCand> d_scand; PinnedBuf<dvo::PlaceShiftCand> h_scand;   /* dvo_tracker_place_shifts: K * DVO_TRACKER_PLACES_MAX_K candidates */
            DevBuf<dvo::PlaceShiftOut> d_shift; PinnedBuf<dvo::PlaceShiftOut> h_shift;     /* ... and their records */
        } pl;
    } ar;
    std::string err;
};

namespace dvo_host {

inline int tfail(dvo_tracker *tr, int code, const std::string &msg) {
    tr->err = msg;
    return code;
}
/* an engine call failed: its message becomes the tracker's */
inline int tchk(dvo_tracker *tr, int rc) {
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

constexpr const char *kArchiveOff = "the key-frame archive is off (dvo_tracker_set_archive)";

/* the end of a step's launch sequence: the error word of its team launches (if any ran) rides on the step's wait */
inline int wait_team_checked(dvo_tracker *tr, bool team) {
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

/* the grey image of the descriptor level as the frame store holds it (dvo_tracker_set_places) */
inline dvo::PlaceGrey place_grey(const dvo_tracker *tr) {
    const FrameLevel &F = tr->ctx->fs.lv[tr->ar.pl.level];
    return dvo::PlaceGrey{F.grey, F.npx, tr->ctx->fs.n_slots, 0};
}

inline float4 k4_of(const dvo::Intrinsics &Ks) { return make_float4(Ks.fx, Ks.fy, Ks.cx, Ks.cy); }

/* places off: the descriptors go, and no slot has one any more */
inline void places_release(dvo_tracker *tr) {
    tr->ar.pl = dvo_tracker::Archive::Places();
    for (KeyRing::Meta &M : tr->ar.ring.slot) M.has_desc = false;
}

/* the archive off: everything of it goes but the ring's next id */
inline void archive_release(dvo_tracker *tr) {
    dvo_tracker::Archive &A = tr->ar;
    places_release(tr);
    if (A.mc) { A.mc->stream = A.mc->own_stream; dvo_destroy(A.mc); }
    A.ring.configure(0, 0);
    const KeyRing ring = A.ring;
    A = dvo_tracker::Archive();
    A.ring = ring;
}

/* n streams of the tracker, none of them twice (the steps, dvo_tracker_query_places) */
inline int check_stream_list(dvo_tracker *tr, int n, const int *streams) {
    std::vector<char> seen(tr->K, 0);
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        if (s < 0 || s >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(s) + " out of range");
        if (seen[s]) return tfail(tr, DVO_ERR_INVALID, "stream " + std::to_string(s) + " listed twice");
        seen[s] = 1;
    }
    return DVO_OK;
}

/* the refusals of dvo_tracker_score, dvo_tracker_match and dvo_tracker_verify; nothing is changed before they pass */
inline int check_candidates(dvo_tracker *tr, int n, const int *stream, const long long *key_id, const void *R, const void *t, const void *records) {
    const dvo_tracker::Archive &A = tr->ar;
    if (!A.on) return tfail(tr, DVO_ERR_STATE, kArchiveOff);
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
        if (!A.ring.find(key_id[i]))
            return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " is not in the archive (unknown or evicted)");
    }
    for (int i = 0; i < n; i++) {
        const float4 k = k4_of(intrinsics_of(tr->ctx, stream[i]));
        if (std::memcmp(&k, A.ring.find(key_id[i])->K, sizeof(float4)) != 0)
            return tfail(tr, DVO_ERR_INVALID, "key frame " + std::to_string(key_id[i]) + " was enlisted under another camera model than stream " +
                                                  std::to_string(stream[i]) + "'s: a pair is decoded and projected under one model");
    }
    return DVO_OK;
}

/* information, views and the archive read the packed engine's resident forms (the compact point lists of the index-list alignment;
 * the one-point-per-lane engine keeps other forms): the refusal of whatever `what_needs` them */
inline int check_resident_forms(dvo_tracker *tr, const char *what_needs) {
    const dvo_params &prm = tr->ctx->prm;
    if (prm.interpolate_dt || prm.engine_variant == 1 || !dvo::fused_uses_compact(prm.points_in_flight, prm.interpolate_dt) || prm.debug_alias_mod > 0)
        return tfail(tr, DVO_ERR_INVALID, std::string(what_needs) + " the packed engine's resident forms: not available with "
                                                                    "dvo_params.interpolate_dt, engine_variant = 1 or debug_alias_mod");
    return DVO_OK;
}

/* the 21 upper-triangle entries of a symmetric 6x6 matrix, row by row -> all 36 */
inline void expand_sym6(const double *H21, double *H36) {
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { H36[i * 6 + j] = H21[k]; H36[j * 6 + i] = H21[k]; k++; }
}

inline void expand_record(const dvo::ScoreRecord &r, dvo_tracker_score_record &o) {
    expand_sym6(r.H, o.H36);
    std::memcpy(o.g6, r.g, sizeof(double) * 6);
    o.sum_eps2 = r.sum_eps2;
    o.n_points = r.n_points;
    o.n_visible = r.n_visible;
}

}  // namespace dvo_host

#endif  // DVO_TRACKER_HOST_H_
