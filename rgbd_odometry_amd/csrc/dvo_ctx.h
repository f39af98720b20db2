/*
 * dvo_ctx.h -- the engine context (struct dvo_ctx) and the host helpers shared by the two halves of the C-ABI
 * implementation: dvo_capi.cpp (lifecycle, inputs, hot path, inspection) and dvo_capi_frames.cpp (frame store,
 * rows f1 + f2).  Internal; not installed.
 */
#ifndef DVO_CTX_H_
#define DVO_CTX_H_

#include "../../include/dvo_amd.h"
#include "dvo_buffers.h"
#include "dvo_handle.h"
#include "dvo_launch.h"
#include "dvo_launch_memo.h"
#include "dvo_launch_plan.h"
#include "dvo_now_state.h"
#include "dvo_upload_ring.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace dvo_host {

/* A per-pair host vector that enqueue()'s stages read (dvo_capi.cpp).  enqueue() remembers what a full pass decided
 * (dvo_launch_memo.h) and trusts it for as long as the context's host generation stands still, so every write has to move that
 * generation: the vector itself is private, reading is const, and each writing access goes through w() / assign() / fill(),
 * which bump the counter the vector was bound to (dvo_ctx's constructor).  Use what w() returns at once; do not keep it. */
struct Level;
template <class T>
class Tracked {
    std::vector<T> v_;
    unsigned long long *gen_ = nullptr;
    void bump() { if (gen_) ++*gen_; }
    friend struct Level;
public:
    void bind(unsigned long long *gen) { gen_ = gen; }
    bool empty() const { return v_.empty(); }
    size_t size() const { return v_.size(); }
    const T &operator[](size_t i) const { return v_[i]; }
    T &w(size_t i) { bump(); return v_[i]; }
    void assign(size_t n, const T &x) { bump(); v_.assign(n, x); }
    void fill(const T &x) { bump(); std::fill(v_.begin(), v_.end(), x); }
};

struct Level {
    int rows = 0, cols = 0;
    float4 *tex = nullptr;
    size_t tex_stride = 0;
    /* SPARSE texel slab (round 4): the 16-byte texels of all pairs are one virtual address range (hipMemAddressReserve) of which
     * only the chunks that some pair's texels were ever asked for are backed by memory (map_texels).  The engine's own now levels
     * exist in the compact form only, so a large resident batch never maps any: 6.5 of the 9.7 MB a 640x480x4 pair used to hold.
     * Kernels keep addressing base + pair * stride.  Dense (one hipMalloc, everything backed) for small slabs. */
    bool tex_sparse = false;
    size_t tex_chunk = 0, tex_va_bytes = 0;
    std::vector<hipMemGenericAllocationHandle_t> tex_handles;   /* per chunk; tex_mapped says which are live */
    std::vector<char> tex_mapped;
    DevBuf<float> pts;
    DevBuf<uint2> cpts;             /* compact twin of pts (8 B / point), same capacity; valid where compact_ok */
    DevBuf<unsigned> cidx;          /* per compact point: its index in the 3 x N list (the compact twin is in block order) */
    DevBuf<unsigned> cpt4;          /* the compact twin again in 4 bytes per point (dvo_device_math.h: pt4_decode), same capacity */
    DevBuf<unsigned> chdr;          /* per chunk of 64 points: linear block index of its first point; pt_cap / 64 per pair */
    DevBuf<int> d_pt4_ok;           /* per pair: the 4-byte list decodes to the 8-byte one bit for bit (written by the builder) */
    Tracked<char> compact_ok;       /* per pair: the list came from the engine's enlist kernels */
    /* per pair: a stamp that changes whenever the pair's reference list is rewritten (ref_list_written).  The packed kernel stores
     * its final outputs in the order of the compact list; the getter permutes them with cidx and must not do so with the index of a
     * list written after the launch */
    Tracked<unsigned long long> list_gen;
    Tracked<int> pt4_rows;          /* per pair: image rows the 4-byte twin of the list was encoded against (pt4_decode needs the same) */
    int pt_cap = 0;
    DevBuf<int> dN;
    Tracked<int> hN;                /* 0 = not set */
    Tracked<NowState> now;         /* per pair: the forms its now level exists in (dvo_now_state.h); n_pairs records from dvo_create_batch on */
    /* compact form of the now levels (dvo_palette.h), allocated at the first build */
    DevBuf<unsigned> p4;            /* n_pairs x p4_stride rank words */
    DevBuf<float2> pal;             /* n_pairs x DVO_PAL_MAX {DT value, weight} */
    DevBuf<int> d_pal_n;            /* n_pairs: > 0 palette size, <= 0 no compact form (kept 0 while the form is stale) */
    size_t p4_stride = 0;

    void bind(unsigned long long *gen) { hN.bind(gen); compact_ok.bind(gen); pt4_rows.bind(gen); list_gen.bind(gen); now.bind(gen); }
    /* one more alignment of `pair` enqueued.  The one write that leaves the generation alone: `uses` is read only by wants_build
     * of a form that is not built, and a pass over such a pair is never remembered (dvo_launch_memo.h: build_possible) */
    void now_used(int pair) { now.v_[(size_t)pair].used(); }
};

/* frame store (rows f1/f2): per level one slab per plane for all slots, slot s at base + s*npx */
struct FrameLevel {
    int rows = 0, cols = 0;
    size_t npx = 0;
    DevBuf<unsigned char> grey, edge;
    DevBuf<float> depth;
};
struct FrameStore {
    int n_slots = 0, n_levels = 0;
    FrameLevel lv[DVO_LEVELS];
    std::vector<char> valid, has_depth;
};
/* diagnostics / tests: DVO_COMPACT_NOW=eager builds the compact form of a now level (dvo_palette.h) at its FIRST alignment
 * (so that every test of the suite runs through it), =off never builds it; default: after DVO_COMPACT_NOW_AFTER alignments */
inline int compact_now_policy() {
    static const int pol = [] {
        const char *e = std::getenv("DVO_COMPACT_NOW");
        return (e && std::strcmp(e, "eager") == 0) ? 1 : ((e && std::strcmp(e, "off") == 0) ? 2 : 0);
    }();
    return pol;
}
}  // namespace dvo_host

struct dvo_ctx {
    dvo_params prm;
    dvo::DevParams dprm;
    int n_pairs = 0;
    int device = 0;                 /* HIP device the context was created on: every entry point makes it current (DeviceGuard) */
    int n_cu = 256;                 /* compute units of the device (auto tuning of launch shapes) */
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    dvo::Intrinsics K{0, 0, 0, 0, 0};
    bool have_K = false;
    dvo_host::Level lv[DVO_LEVELS];
    dvo_host::DevBuf<float> staging;    /* 3 planes (or one point list) of the largest upload so far */
    dvo_host::DevBuf<double> d_poses;
    dvo_host::DevBuf<float> d_energy;
    dvo_host::DevBuf<int> d_best;
    dvo_host::DevBuf<float> d_ratio;
    dvo_host::DevBuf<float> d_final_eps, d_final_reproj;
    dvo_host::DevBuf<int> d_final_N;
    dvo_host::DevBuf<double> d_H;       /* DVO_FLAG_NORMAL_MATRIX output, n_pairs x e_stride x 21 */
    dvo_host::DevBuf<int> d_tex_mode;
    /* team mode of the packed kernel (G workgroups per pair for small batches): exchange slots, arrival counters, error flag */
    dvo_host::DevBuf<double> d_team_buf;
    dvo_host::DevBuf<unsigned> d_team_cnt;     /* n_pairs counters followed by one int error flag */
    int last_block = 0, last_team = 0, last_packed = 0;   /* shape of the last fused launch (dvo_get_last_launch_shape) */
    unsigned team_epoch = 0;             /* team mode: exchanges every launch so far may have run (Schedule.team_epoch0 of the next launch) */
    bool team_legacy = false;            /* a team launch was captured into a caller's graph once: zero the records before every launch again */
    bool team_err_dirty = false;         /* the device's error word is set (reported by the getters): the next team launch clears it */
    bool team_used = false;              /* the last enqueue ran in team mode: dvo_get_poses checks the error flag */      /* n_pairs x DVO_LEVELS, written by the packed fused kernel */
    int final_cap = 0;
    dvo_host::DevBuf<double> d_scratch;   /* partials (1024 x 32) + acc (32) + misc doubles */
    /* dvo_align_pyramid_wide as a replayable hipGraph (the schedule is ~2 dependent launches per iteration) */
    hipGraphExec_t wide_exec = nullptr;
    unsigned long long wide_sig = 0;
    int step_solo_mask = 0;              /* ... and those that ran as one launch of one workgroup (tiled_level_solo_kernel) */
    int step_pk_mask = 0;                /* levels of the last enqueued step schedule that ran tiled_step_pk_kernel (inspection) */
    dvo_host::PinnedBuf<double> h_pose;     /* pinned: in/out pose of the graph's copy nodes */
    int wide_team_mask = 0;         /* levels the last dvo_align_pyramid_wide handed to the fused team kernel (round 6) */
    int direct_compact = -1;        /* dvo_set_direct_compact: float now levels go to the compact form at installation (-1: auto, by batch size) */
    dvo_host::PinnedBuf<double> h_poses;     /* pinned: dvo_get_poses / dvo_set_poses staging, 12 doubles per pair */
    dvo_host::DevBuf<char> d_states;     /* n_pairs x pose_state_bytes(): host-driven iteration state */
    /* one-launch-per-iteration schedule (dvo_align_pyramid_wide / _tiled, round 4): two optimiser states (double-buffered), two
     * rows of 32 reduced sums (alternating), the arrival ticket of the partial rows */
    dvo_host::DevBuf<char> d_step_state;
    dvo_host::DevBuf<double> d_step_acc;
    dvo_host::DevBuf<unsigned> d_step_ticket;
    hipGraphExec_t tiled_exec = nullptr;     /* the tiled schedule (incl. its ncclAllReduce calls) as a replayable graph */
    unsigned long long tiled_sig = 0;
    bool tiled_graph_used = false;           /* inspection: the last dvo_align_pyramid_tiled replayed its graph */
    dvo_host::DevBuf<float> d_iter_energy; /* n_pairs x iter_energy_cap */
    int iter_energy_cap = 0;
    std::vector<int> iter_max;      /* per pair: max_iters of the running dvo_iter_begin (0 = none) */
    dvo_host::DevBuf<int> d_colcounts;
    dvo_host::DevBuf<int> d_order;       /* launch order of the pairs of a large batch (longest first) */
    std::vector<int> h_order;
    unsigned long long points_gen = 1;   /* bumped whenever a reference list changes (its length is the launch-order key) */
    unsigned long long order_key[4] = {0, 0, 0, 0};   /* points_gen, first_pair, n_pairs, hash of the schedule the resident order was made for */
    dvo_host::DevBuf<unsigned> pal_work; /* scratch of the compact-now-form builder (dvo_palette.hip) */
    dvo_host::FrameStore fs;
    /* cv::undistort of the publisher: fixed-point map of the camera's full resolution (dvo_frames_set_undistort) */
    dvo_host::DevBuf<short2> d_umap_xy;
    dvo_host::DevBuf<unsigned short> d_umap_frac;
    int umap_rows = 0, umap_cols = 0;
    /* per-pair calibration (the multi-stream tracker's per-stream camera models; a plain context never has any).
     * Intrinsics: d_pair_K (n_pairs entries, K.pair_K points at it) exists once some pair has its own; every other entry holds K.
     * Undistortion: pair_umap[p] = -1 the context's map above, 0 none, m > 0 umaps[m - 1] (shared by every pair with the same
     * calibration, freed with its last user); d_umap_*_tab resolve them per pair for the camera-level launches */
    dvo_host::DevBuf<float4> d_pair_K;
    std::vector<float4> h_pair_K;
    std::vector<char> pair_K_own;
    struct UMap {
        double key[9];                  /* K4 | D5 */
        int rows = 0, cols = 0, users = 0;
        dvo_host::DevBuf<short2> xy;
        dvo_host::DevBuf<unsigned short> frac;
    };
    std::vector<UMap> umaps;
    std::vector<int> pair_umap;
    dvo_host::DevBuf<short2 *> d_umap_xy_tab;
    dvo_host::DevBuf<unsigned short *> d_umap_frac_tab;
    /* per-pair ignore masks (dvo_frames_set_pair_mask; a context that never set one has none of this).  pair_mask[p] = 0 none,
     * m > 0 masks[m - 1]: the keep planes of every level in one allocation, shared by the pairs that were given it in one call and
     * freed with its last user.  d_mask_tab resolves them per pair and level (p * DVO_LEVELS + l, NULL = no mask) for the one launch
     * of the upload paths; it is uploaded by the setter, never by an upload */
    struct MaskSet {
        int users = 0, n_levels = 0;
        int rows[DVO_LEVELS] = {0}, cols[DVO_LEVELS] = {0};
        size_t off[DVO_LEVELS] = {0};
        dvo_host::DevBuf<unsigned char> keep;
    };
    std::vector<MaskSet> masks;
    std::vector<int> pair_mask;
    dvo_host::DevBuf<const unsigned char *> d_mask_tab;
    dvo_host::DevBuf<int> work;       /* preprocessing scratch (Canny / distance transform / point counts) */
    /* frame uploads (dvo_upload_ring.h): two landing buffers filled by copy streams while the context stream preprocesses the other;
     * camera frames that already sit in HBM are read where they are, through a table of their addresses */
    dvo_host::UploadRing upload;
    dvo_host::SourceTable src_tab;
    struct dvo_photo_state *photo = nullptr;     /* dvo_capi_photo.cpp: the photometric engine's reference data */
    struct dvo_depth_state *depth_reg = nullptr; /* dvo_capi_depth.cpp: depth rigs, z-buffer and registered images; NULL until a rig is set */
    struct dvo_keep_warm_state *warm = nullptr;  /* dvo_set_keep_warm: the thread that keeps the GPU at its active clocks */
    dvo::Schedule sched{};
    bool have_sched = false;
    /* which pairs the per-pair outputs (energies, final outputs) currently describe: the output buffers are laid out by
     * the schedule of the enqueue that wrote them, so a pair aligned under an older, differently shaped schedule (or before
     * the buffers were re-allocated) has nothing valid to report */
    int sched_gen = 0;
    std::vector<int> pair_gen;      /* per pair: sched_gen of the enqueue that last aligned it (0 = never) */
    std::vector<unsigned long long> final_list_gen;   /* per pair: list_gen of the finest level's list the last enqueue aligned */
    std::string err;
    /* enqueue()'s memo (dvo_launch_memo.h).  host_gen: bumped by every write of the host state enqueue()'s stages read -- the
     * Tracked vectors of the levels by themselves, everything else by host_changed() at the place of the write */
    unsigned long long host_gen = 1;
    dvo_host::MemoMode memo_mode = dvo_host::MEMO_ON;      /* DVO_LAUNCH_MEMO, read when the context is made */
    dvo_host::LaunchMemo memo;
    dvo::Schedule memo_sched{};          /* what the remembered pass decided */
    dvo_host::LaunchPlan memo_plan;
    bool memo_order = false;             /* ... and that it launched through d_order */
    void host_changed() { host_gen++; }

    dvo_ctx() { for (dvo_host::Level &L : lv) L.bind(&host_gen); }
    dvo_ctx(const dvo_ctx &) = delete;
    dvo_ctx &operator=(const dvo_ctx &) = delete;
};


namespace dvo_host {

/* the context's device is current for an entry point (dvo_handle.h: OnDevice); a NULL context does nothing */
struct DeviceGuard : OnDevice {
    explicit DeviceGuard(const dvo_ctx *c) : OnDevice(c ? c->device : -1, false) {}
};
#define DVO_ENTER(c)                         \
    if (!(c)) return DVO_ERR_INVALID;        \
    dvo_host::DeviceGuard dvo_device_guard_(c)

int fail(dvo_ctx *c, int code, const std::string &msg);
/* Wait for a stream WITHOUT going to sleep on an interrupt first: poll its completion (hipStreamQuery reads the queue's
 * signal) for up to two milliseconds, only then block in hipStreamSynchronize.  On this pool a process can find the wake-up
 * from a blocking wait delayed by 14-33 ms (measured on the single-camera-stream path, profiles/r03_single_stream: kernels of
 * 0.2 ms, waits of 24 ms, intermittently per process); a single stream's frame is over in well under a millisecond, so the
 * poll costs one busy host thread for that long.  DVO_WAIT=block in the environment restores the plain blocking wait. */
hipError_t stream_wait(hipStream_t s);
inline thread_local unsigned long long g_host_waits = 0;     /* stream_wait calls of this host thread (dvo_tracker_get_stats) */
#define HIPCHK(c, expr)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return dvo_host::fail((c), DVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

/* room for n elements in a buffer whose contents need not survive: free BEFORE allocate (peak memory), after a wait for the
 * context stream, which may still use the old block.  A failed allocation leaves the buffer empty. */
template <class Buf>
int regrow(dvo_ctx *c, Buf &buf, size_t n) {
    if (n <= buf.size()) return DVO_OK;
    if (buf.size()) { HIPCHK(c, stream_wait(c->stream)); buf.reset(); }
    HIPCHK(c, buf.alloc(n));
    return DVO_OK;
}
int ensure_staging(dvo_ctx *c, size_t bytes);
int ensure_work(dvo_ctx *c, size_t bytes);
bool pair_ok(const dvo_ctx *c, int pair);
bool level_ok(int level);
int ensure_points(dvo_ctx *c, int level, int N);                 /* room for N points per pair at `level` (keeps contents) */
int ensure_texels(dvo_ctx *c, int level, int rows, int cols);
/* the now level of `pair` at `level` was (re)written: mark it present and its compact form stale */
int now_written(dvo_ctx *c, int level, int first_pair, int count);
/* the slabs of the compact form of `level` (allocated at first use) */
int ensure_compact_slabs(dvo_ctx *c, int level);
/* the now level of these pairs was (re)written in its compact form only (launch_edges_to_now with p4 != NULL) */
int now_written_compact(dvo_ctx *c, int level, int first_pair, int count);
/* make the 16-byte texels of these pairs' now level valid (decoded from the compact form where that is all there is): for
 * every path that reads texels -- everything except the packed fused kernel on the compact form */
int ensure_tex16(dvo_ctx *c, int level, int first_pair, int count);
/* true if now levels written by the engine's own distance-transform stage should be compact (false: DVO_COMPACT_NOW=off or
 * dvo_params.engine_variant = 4 -- plain 16-byte texels) */
bool native_compact_wanted(const dvo_ctx *c);
/* build the compact form of the stale now levels among [first_pair, first_pair+count) at `level`; with only_reused, only
 * of those that have been aligned DVO_COMPACT_NOW_AFTER times (the build costs about 4.4 alignments) */
int build_compact_now(dvo_ctx *c, int level, int first_pair, int count, bool only_reused);
/* schedule / readiness / output bookkeeping of the align entry points (dvo_capi.cpp) */
dvo::LevelSlab slab_of(const dvo_ctx *c, int level);
int check_ready(dvo_ctx *c, int pair, int level);
int build_schedule(dvo_ctx *c, int n_levels, const int *iters, int flags, dvo::Schedule &sc);
int ensure_outputs(dvo_ctx *c, const dvo::Schedule &sc);
void stamp_outputs(dvo_ctx *c, const dvo::Schedule &sc, int first, int n);
/* backs the texels of pairs [first, first + count) of a level with memory (no-op for a dense slab) */
int map_texels(dvo_ctx *c, int level, int first, int count, hipStream_t stream = nullptr);
void free_texels(dvo_ctx *c, Level &L);
/* sparse slabs, after a distance-transform launch over pairs [first, first + count) that ran WITHOUT texel output: waits for it,
 * reads the palette sizes back and maps the texels of the images the compact form could not hold; *n_failed = how many */
int sparse_map_compact_failures(dvo_ctx *c, int level, int first, int count, hipStream_t stream, int *n_failed);
int refresh_compact_known(dvo_ctx *c, int level, int first, int count, bool skip_native = false);      /* reads pal_n back where the host does not know it yet (skip_native: only where a refusal is possible) */
/* enqueues the level schedule of one pair as ONE launch per iteration on c->stream (dvo_kernels.hip: tiled_step_kernel): this
 * rank's contiguous share of every level's points (rank / world: dvo_tiled_shard's decomposition), `all_reduce` (may be empty:
 * one GPU) called on the 32 sums between two launches.  Pose in / out through d_pose (12 doubles on the device). */
hipError_t enqueue_step_schedule(dvo_ctx *c, const dvo::Schedule &sc, int pair, int flags, double *d_pose, int rank, int world,
                                 const std::function<hipError_t(double *)> &all_reduce);
int ensure_step_buffers(dvo_ctx *c);
hipError_t team_err_fetch(dvo_ctx *c, int *pinned_slot);      /* the error word of the last team launch -> a pinned slot, on the stream (no wait) */
int team_err_result(dvo_ctx *c, const int *pinned_slot);       /* after the caller's wait: DVO_ERR_HIP if it was set */
int team_err_check(dvo_ctx *c);       /* after a wait: DVO_ERR_HIP if a member of the last team launch gave up waiting for its team */
/* the wide / tiled schedule's coarse levels as one team launch of the fused kernel (dvo_capi.cpp) */
int wide_coarse_levels_as_team(dvo_ctx *c, int pair, int n_levels, const int *iters, int flags, dvo::Schedule &sc, const double *h_pose_in,
                               double *d_pose, unsigned &coarse_mask, bool &coarse_team, bool allow_finest);
/* after the wait of a wide / tiled alignment: the outputs of `pair` follow the whole schedule `iters` (sc: what was left for the step launches) */
int stamp_step_alignment(dvo_ctx *c, dvo::Schedule &sc, int pair, int n_levels, const int *iters, int flags, unsigned coarse_mask, bool coarse_team);
int check_step_lost(dvo_ctx *c);    /* after the wait of a wide / tiled alignment: DVO_ERR_HIP if a step launch lost a workgroup's rows */
unsigned long long step_schedule_signature(dvo_ctx *c, const dvo::Schedule &sc, int pair, int n_levels, int flags, int rank, int world);
/* the reference lists of pairs [first, first + n) of a level were (re)written: bumps points_gen and the pairs' list stamps;
 * rows > 0: the rows of the image their 4-byte twins were encoded against (0: no valid 4-byte twin) */
void ref_list_written(dvo_ctx *c, int level, int first, int n, int rows);
/* index-list forms (the multi-stream tracker, dvo_capi_tracker.cpp): one launch sequence for any set of pairs.
 * enqueue_pair_list: the fused alignment of pairs h_pairs[0 .. n) (d_pairs: the same on the device) -- dvo_align_batch_enqueue for a set.
 * frames_as_ref_list: dvo_frames_as_ref for slot h_slots[i] -> pair h_pairs[i] (d_map[i] = {slot, pair} on the device); N_out[i * levels + l]. */
int enqueue_pair_list(dvo_ctx *c, const int *h_pairs, const int *d_pairs, int n, int n_levels, const int *iters, int flags);
int frames_as_ref_list(dvo_ctx *c, const int *h_slots, const int *h_pairs, const int2 *d_map, int count, int *N_out);
/* per-pair calibration (dvo_capi.cpp, dvo_capi_frames.cpp).  pair_intrinsics_set: own = false gives the pair the context's K again.
 * pair_undistort_set: mode -1 the context's map, 0 none, 1 the map of (K4, D5) at rows x cols.  Both wait for the stream and upload
 * their tables at once (never per launch). */
int pair_intrinsics_set(dvo_ctx *c, int pair, bool own, float fx, float fy, float cx, float cy);
int pair_undistort_set(dvo_ctx *c, int pair, int mode, int rows, int cols, const double *K4, const double *D5);
int pair_umap_tables_upload(dvo_ctx *c);
void tiled_forget(dvo_ctx *c);
void depth_forget(dvo_ctx *c);           /* dvo_capi_depth.cpp: frees the depth registration state; the caller has waited for the stream (dvo_destroy) */
/* makes stream s wait for the last depth registration's resolve launch (no-op in a context that never registered): for copy streams
 * that gather device sources, which may be the registered images */
hipError_t depth_registered_ready(dvo_ctx *c, hipStream_t s);
void photo_forget(dvo_ctx *c);           /* dvo_capi_photo.cpp */         /* dvo_capi_tiled.cpp: drop the RCCL attachment of a context */

/* the camera model of one pair for the launches that run one pair (no table) */
inline dvo::Intrinsics intrinsics_of(const dvo_ctx *c, int pair) {
    dvo::Intrinsics k = c->K;
    k.pair_K = nullptr;
    if (c->d_pair_K && pair >= 0 && pair < (int)c->h_pair_K.size()) {
        const float4 v = c->h_pair_K[pair];
        k.fx = v.x; k.fy = v.y; k.cx = v.z; k.cy = v.w;
    }
    return k;
}

}  // namespace dvo_host
#endif
