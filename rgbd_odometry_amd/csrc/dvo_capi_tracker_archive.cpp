/*
 * dvo_capi_tracker_archive.cpp -- the key-frame archive of the multi-stream tracker (include/dvo_amd.h, "key-frame archive"): the ring's
 * set-up and inspection, export and import of its blobs, score, match and verify.  Host side of dvo_tracker_archive.hip,
 * dvo_tracker_archive_blob.hip and dvo_tracker_verify.hip; the ring rule is dvo_key_ring.h, the step's store dvo_capi_tracker.cpp.
 */
#include "dvo_archive_blob.h"
#include "dvo_tracker_host.h"

using namespace dvo;
using namespace dvo_host;

namespace {

/* the slots an export lists, in its order, and the size of its blob; nothing is changed */
int export_plan(dvo_tracker *tr, int n, const long long *key_id, std::vector<int> &slots, size_t &total) {
    const dvo_tracker::Archive &A = tr->ar;
    if (!A.on) return tfail(tr, DVO_ERR_STATE, kArchiveOff);
    if (n < 0) return tfail(tr, DVO_ERR_INVALID, "n must be >= 0");
    slots.clear();
    if (!key_id) {                                         /* every live key frame, ascending id */
        for (long long id = std::max(0LL, A.ring.next_id - A.ring.capacity); id < A.ring.next_id; id++) {
            int slot = 0;
            if (tr->ar.ring.find(id, &slot)) slots.push_back(slot);
        }
    } else {
        for (int i = 0; i < n; i++) {
            int slot = 0;
            if (!tr->ar.ring.find(key_id[i], &slot))
                return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " is not in the archive (unknown, refused or evicted)");
            slots.push_back(slot);
        }
    }
    if (slots.size() > (size_t)INT32_MAX) return tfail(tr, DVO_ERR_INVALID, "too many key frames for one blob");
    uint64_t bytes = sizeof(dvo_blob::Header) + sizeof(dvo_blob::Record) * (uint64_t)slots.size();
    for (int slot : slots) {
        const KeyRing::Meta &M = A.ring.slot[slot];
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
    A.max_matches = max_matches;
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
    A.ring.configure(capacity, tr->K);
    A.on = true;
    return DVO_OK;
}

int dvo_tracker_key_frame_id(dvo_tracker *tr, int stream, long long *id) {
    if (!tr) return DVO_ERR_INVALID;
    if (stream < 0 || stream >= tr->K) return tfail(tr, DVO_ERR_INVALID, "stream out of range");
    if (!id) return tfail(tr, DVO_ERR_INVALID, "NULL argument");
    if (!tr->ar.on) return tfail(tr, DVO_ERR_STATE, "the key-frame archive is off (dvo_tracker_set_archive)");
    if (!tr->st[stream].started) return tfail(tr, DVO_ERR_STATE, "stream " + std::to_string(stream) + " has not been stepped yet");
    *id = tr->ar.ring.key_id[stream];
    return DVO_OK;
}

int dvo_tracker_archive_info(dvo_tracker *tr, long long id, int *stream, long long *frame, int *n_points) {
    if (!tr) return DVO_ERR_INVALID;
    const KeyRing::Meta *M = tr->ar.ring.find(id);
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
    const KeyRing::Meta *M = tr->ar.ring.find(id, &slot);
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
    if (archived) *archived = tr->ar.ring.n_archived;
    if (refused) *refused = tr->ar.ring.n_refused;
    if (evicted) *evicted = tr->ar.ring.n_evicted;
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
            const KeyRing::Meta &M = A.ring.slot[slots[i]];
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
    /* the plan: ids and slots under the ring rule (dvo_key_ring.h), as the step's store gives them; key frames that a later one of
     * the blob overwrites need not be copied (slot -1).  Nothing of the tracker changes before the payload checksums have come back */
    std::vector<char> fits((size_t)n, 1);
    std::vector<KeyRing::Meta> meta((size_t)n);
    for (int i = 0; i < n; i++) {
        const dvo_blob::Record &r = table[(size_t)i];
        BlobEntry &e = A.h_bent[i];
        e = BlobEntry{};
        e.origin_id = r.origin_id; e.origin_stream = r.origin_stream; e.origin_frame = r.origin_frame;
        e.payload_offset = r.payload_offset; e.payload_bytes = r.payload_bytes;
        e.record = i; e.has_desc = (take_desc && r.has_desc) ? 1 : 0;
        KeyRing::Meta &M = meta[(size_t)i];
        M.frame = (long)r.origin_frame;
        std::memcpy(M.K, r.K, sizeof(M.K));
        M.has_desc = e.has_desc != 0;
        M.origin_id = r.origin_id; M.origin_stream = r.origin_stream; M.origin_frame = r.origin_frame;
        for (int l = 0; l < DVO_LEVELS; l++) {
            e.N[l] = M.N[l] = r.N[l];
            fits[(size_t)i] = fits[(size_t)i] && (l >= tr->n_levels || r.N[l] <= A.cap[l]);
        }
    }
    const KeyRing::Plan plan = A.ring.plan(fits.data(), n);
    for (int i = 0; i < n; i++) A.h_bent[i].slot = plan.item[(size_t)i].written ? plan.item[(size_t)i].slot : -1;
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
    A.ring.commit(plan, meta.data());
    TRKHIP(launch_archive_import(A.d_bent, n, A.d_blob, A.view, A.pl.view, c->stream));
    for (int i = 0; i < std::min(n, ids_capacity); i++) ids_out[i] = plan.item[(size_t)i].id;
    A.last_launches = (int)(g_kernel_launches - launches0);
    A.last_syncs = (int)(g_host_waits - waits0);
    return DVO_OK;
}

int dvo_tracker_archive_origin(dvo_tracker *tr, long long id, long long *origin_id, int *origin_stream, long long *origin_frame) {
    if (!tr) return DVO_ERR_INVALID;
    const KeyRing::Meta *M = tr->ar.ring.find(id);
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
        (void)tr->ar.ring.find(key_id[i], &slot);
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
        const KeyRing::Meta *M = tr->ar.ring.find(key_id[i], &slot);
        ArchiveLoad &ld = A.h_load[i];
        ld.slot = slot; ld.now_pair = stream[i]; ld.dst = i;
        std::memcpy(ld.pose, R0 + 9 * (size_t)i, sizeof(double) * 9);
        std::memcpy(ld.pose + 9, t0 + 3 * (size_t)i, sizeof(double) * 3);
        if (mc->d_pair_K) { mc->h_pair_K[i] = make_float4(M->K[0], M->K[1], M->K[2], M->K[3]); mc->pair_K_own[i] = 1; }      /* the device's entry is written by the load launch */
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
        (void)tr->ar.ring.find(key_id[i], &slot);
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

}  // extern "C"
