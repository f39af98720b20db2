/*
 * dvo_capi_tracker_places.cpp -- place descriptors of the archived key frames of the multi-stream tracker (include/dvo_amd.h,
 * dvo_tracker_set_places ...): top-k retrieval, the shift search and the pose guess.  Host side of dvo_tracker_places.hip; the step's
 * descriptor store is in dvo_capi_tracker.cpp.
 */
#include "dvo_place_guess.h"
#include "dvo_tracker_host.h"

using namespace dvo;
using namespace dvo_host;

extern "C" {

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
        const size_t S = (size_t)A.ring.capacity, K = (size_t)tr->K;
        P.level = level;
        P.view.n_slots = A.ring.capacity; P.view.D = (int)D; P.view.stride = (int)((D + 15) / 16 * 16);
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
    const KeyRing::Meta *M = tr->ar.ring.find(id, &slot);
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
    if (const int rc = check_stream_list(tr, n, streams)) return rc;
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
        int own = -1;
        if (!A.ring.find(A.ring.key_id[s], &own)) own = -1;
        P.h_query[i] = PlaceQuery{S.bank * tr->K + s, s, own, 0, (long long)S.n_frame - 1, k4_of(intrinsics_of(c, s))};
    }
    PlaceOut *d_rows = reinterpret_cast<PlaceOut *>(P.d_out.get());
    int *d_found = reinterpret_cast<int *>(P.d_out + sizeof(PlaceOut) * (size_t)n * k);
    const size_t out_bytes = sizeof(PlaceOut) * (size_t)n * k + sizeof(int) * (size_t)n;
    TRKHIP(hipMemcpyAsync(P.d_query, P.h_query, sizeof(PlaceQuery) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TRKHIP(launch_place_query(P.d_query, n, k, min_frame_gap, A.ring.next_id - A.ring.capacity, place_grey(tr), P.view, A.view.hdr, P.d_dist, d_rows,
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
        const KeyRing::Meta *M = tr->ar.ring.find(key_id[i]);
        if (!M) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " is not in the archive (unknown or evicted)");
        if (!M->has_desc) return tfail(tr, DVO_ERR_STATE, "key frame " + std::to_string(key_id[i]) + " was archived while place descriptors were off");
    }
    for (int i = 0; i < n; i++) {
        const float4 k = k4_of(intrinsics_of(c, stream[i]));
        if (std::memcmp(&k, A.ring.find(key_id[i])->K, sizeof(float4)) != 0)
            return tfail(tr, DVO_ERR_INVALID, "key frame " + std::to_string(key_id[i]) + " was enlisted under another camera model than stream " +
                                                  std::to_string(stream[i]) + "'s");
    }
    DeviceGuard g(c);
    const unsigned long long launches0 = g_kernel_launches, waits0 = g_host_waits;
    for (int i = 0; i < n; i++) {
        int slot = 0;
        (void)tr->ar.ring.find(key_id[i], &slot);
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

}  // extern "C"
