/*
 * dvo_capi_depth.cpp -- depth registration of the frame stage (include/dvo_amd.h, "depth registration"): the host builder's entry
 * point (dvo_depth_register.h is the definition), the per-pair rigs, and the registration itself -- two launches of
 * dvo_depth_register.hip per call.  Host side only; no CPU compute path behind the context's entry points.
 */
#include "dvo_ctx.h"
#include "dvo_depth_register.h"

using namespace dvo;
using namespace dvo_host;

/* A context that never set a rig has none of this.  The rig table (one entry per pair) goes up in the setter; a registration uploads
 * only the table of its source addresses.  z: the 32-bit z-buffers, 0xFFFFFFFF everywhere between two calls (the resolve launch
 * re-arms what the scatter touched; z_armed is false only after an allocation or a call that failed between its two launches).
 * out: the registered images of the last call, image i of pair first_pair + i at i * stride */
struct dvo_depth_state {
    std::vector<char> has;
    std::vector<dvo_depth_rig> rig;
    std::vector<int> rows, cols;                    /* per pair: the colour geometry its rig was set for */
    DevBuf<dvo_depth_rig> d_rig;
    DevBuf<unsigned> z;
    bool z_armed = false;
    DevBuf<unsigned short> out;
    DevBuf<unsigned char> land;                     /* host sources: where the raw images land, image i at i * (its call's) image stride */
    DevBuf<const void *> d_src;
    /* pinned staging, two slots used in turn: a call fills the slot whose copies were queued two calls ago, so that the runs of one
     * step never wait for one another's copies */
    struct Stage {
        PinnedBuf<unsigned char> mirror;            /* host sources are gathered here */
        PinnedBuf<const void *> h_src;
        hipEvent_t ev = nullptr;                    /* the copies out of this slot have left */
        bool pending = false;
    } stage[2];
    int next_stage = 0;
    hipEvent_t ev_resolved = nullptr;               /* the last registration's resolve launch has finished: `out` is complete */
    bool resolved_pending = false;
    int first_pair = -1, count = 0, img_rows = 0, img_cols = 0;     /* what `out` holds */
    size_t stride = 0;
};

namespace dvo_host {
void depth_forget(dvo_ctx *c) {
    dvo_depth_state *S = c->depth_reg;
    if (!S) return;
    for (dvo_depth_state::Stage &T : S->stage)
        if (T.ev) (void)hipEventDestroy(T.ev);
    if (S->ev_resolved) (void)hipEventDestroy(S->ev_resolved);
    delete S;
    c->depth_reg = nullptr;
}
/* Work on stream `s` that follows reads the registered images only after the resolve launch that writes them.  The registration runs
 * on the context stream; an upload that cannot read device sources in place gathers them on its copy streams, which nothing else
 * orders behind it */
hipError_t depth_registered_ready(dvo_ctx *c, hipStream_t s) {
    const dvo_depth_state *S = c->depth_reg;
    if (!S || !S->resolved_pending) return hipSuccess;
    return hipStreamWaitEvent(s, S->ev_resolved, 0);
}
}  // namespace dvo_host

namespace {
/* room for n elements, contents not kept; *grown: the old block (if any) was replaced, after a wait for the context stream */
template <class Buf>
int grow(dvo_ctx *c, Buf &buf, size_t n, bool *grown) {
    if (n <= buf.size()) return DVO_OK;
    *grown = true;
    return regrow(c, buf, n);
}
}  // namespace

extern "C" {

int dvo_depth_register_host(const dvo_depth_rig *rig, const void *depth, int depth_format, int rows, int cols, unsigned short *out) {
    return dvo_depth::build(rig, depth, depth_format, rows, cols, out) ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_frames_set_pair_depth_rig(dvo_ctx *c, int pair, const dvo_depth_rig *rig, int rows, int cols) {
    DVO_ENTER(c);
    /* refusals first: a refused call leaves every rig in force as it was */
    if (pair < -1 || pair >= c->n_pairs) return fail(c, DVO_ERR_INVALID, "pair out of range (-1: every pair)");
    if (rig && (!dvo_depth::rig_ok(rig) || rows < 1 || cols < 1))
        return fail(c, DVO_ERR_INVALID, "bad depth rig (sizes >= 1, focal lengths positive, every number finite, has_Dc5 0 or 1)");
    if (!rig && !c->depth_reg) return DVO_OK;                        /* no pair has a rig already */
    if (!c->depth_reg) {
        dvo_depth_state *N = new dvo_depth_state();
        N->has.assign(c->n_pairs, 0);
        N->rig.assign(c->n_pairs, dvo_depth_rig());
        N->rows.assign(c->n_pairs, 0);
        N->cols.assign(c->n_pairs, 0);
        c->depth_reg = N;
    }
    dvo_depth_state &S = *c->depth_reg;
    if (!S.d_rig) HIPCHK(c, S.d_rig.alloc((size_t)c->n_pairs));
    HIPCHK(c, stream_wait(c->stream));                               /* no launch in flight reads the old table */
    for (int p = (pair < 0 ? 0 : pair); p < (pair < 0 ? c->n_pairs : pair + 1); p++) {
        S.has[p] = rig ? 1 : 0;
        S.rig[p] = rig ? *rig : dvo_depth_rig();
        S.rows[p] = rig ? rows : 0;
        S.cols[p] = rig ? cols : 0;
    }
    HIPCHK(c, hipMemcpy(S.d_rig, S.rig.data(), sizeof(dvo_depth_rig) * (size_t)c->n_pairs, hipMemcpyHostToDevice));
    return DVO_OK;
}

int dvo_frames_register_depth(dvo_ctx *c, int first_pair, int count, const void *const *depth, int depth_format, int flags,
                              const unsigned short **d_out) {
    DVO_ENTER(c);
    if (flags & ~(DVO_UPLOAD_ASYNC | DVO_UPLOAD_DEVICE))
        return fail(c, DVO_ERR_INVALID, "depth registration takes host sources (0) or DVO_UPLOAD_DEVICE, with or without DVO_UPLOAD_ASYNC");
    if (depth_format != DVO_DEPTH_F32 && depth_format != DVO_DEPTH_U16)
        return fail(c, DVO_ERR_INVALID, "unknown depth format (DVO_DEPTH_F32 / DVO_DEPTH_U16)");
    if (!depth || count < 1 || !pair_ok(c, first_pair) || count > c->n_pairs - first_pair)
        return fail(c, DVO_ERR_INVALID, "bad depth registration arguments (pair range, image list)");
    for (int i = 0; i < count; i++)
        if (!depth[i]) return fail(c, DVO_ERR_INVALID, "NULL depth image");
    dvo_depth_state *Sp = c->depth_reg;
    for (int p = first_pair; p < first_pair + count; p++)
        if (!Sp || !Sp->has[p]) return fail(c, DVO_ERR_STATE, "pair " + std::to_string(p) + " has no depth rig (dvo_frames_set_pair_depth_rig)");
    dvo_depth_state &S = *Sp;
    const int rows = S.rows[first_pair], cols = S.cols[first_pair];
    size_t max_px = 0;
    for (int p = first_pair; p < first_pair + count; p++) {
        if (S.rows[p] != rows || S.cols[p] != cols)
            return fail(c, DVO_ERR_INVALID, "the listed pairs' rigs were set for different colour geometries");
        max_px = std::max(max_px, (size_t)S.rig[p].depth_rows * (size_t)S.rig[p].depth_cols);
    }
    const bool dev_src = (flags & DVO_UPLOAD_DEVICE) != 0;
    const size_t stride = depth_register_stride(rows, cols), bpp = depth_format == DVO_DEPTH_U16 ? 2 : 4;
    const size_t img_bytes = (max_px * bpp + 15) / 16 * 16;
    /* the pools: a growth waits for the context stream (the old block may be in use) and is the only host synchronisation here */
    bool z_grown = false, out_grown = false;
    const size_t out_was = S.out.size();
    int rc;
    if ((rc = grow(c, S.z, stride * count, &z_grown))) { S.z_armed = false; return rc; }
    if (z_grown) S.z_armed = false;
    if ((rc = grow(c, S.out, stride * count, &out_grown))) { S.count = 0; return rc; }
    if (out_grown && out_was) S.count = 0;                           /* the previous call's images went with the old block */
    dvo_depth_state::Stage &T = S.stage[S.next_stage];
    if (!T.ev) HIPCHK(c, hipEventCreateWithFlags(&T.ev, hipEventDisableTiming));
    if (!S.ev_resolved) HIPCHK(c, hipEventCreateWithFlags(&S.ev_resolved, hipEventDisableTiming));
    if (T.pending) {                                                 /* the slot's copies of two calls ago: gone, unless the host ran far ahead */
        if (hipEventQuery(T.ev) != hipSuccess) HIPCHK(c, hipEventSynchronize(T.ev));
        T.pending = false;
    }
    if ((size_t)count > S.d_src.size()) {
        if (S.d_src.size()) HIPCHK(c, stream_wait(c->stream));
        HIPCHK(c, S.d_src.alloc((size_t)count));
    }
    if ((size_t)count > T.h_src.size()) HIPCHK(c, T.h_src.alloc((size_t)count));
    if (!dev_src) {
        if ((rc = regrow(c, S.land, img_bytes * count))) return rc;
        if (img_bytes * count > T.mirror.size()) HIPCHK(c, T.mirror.alloc(img_bytes * count));
    }
    if (!S.z_armed) HIPCHK(c, hipMemsetAsync(S.z, 0xFF, sizeof(unsigned) * S.z.size(), c->stream));
    S.z_armed = true;
    for (int i = 0; i < count; i++) {
        if (dev_src) { T.h_src[i] = depth[i]; continue; }
        const dvo_depth_rig &g = S.rig[first_pair + i];
        std::memcpy(T.mirror + img_bytes * i, depth[i], (size_t)g.depth_rows * (size_t)g.depth_cols * bpp);
        T.h_src[i] = S.land + img_bytes * i;
    }
    if (!dev_src) HIPCHK(c, hipMemcpyAsync(S.land, T.mirror, img_bytes * (size_t)count, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.d_src, T.h_src, sizeof(const void *) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(T.ev, c->stream));
    T.pending = true;
    S.next_stage ^= 1;
    /* from here on `out` is being rewritten, and the z-buffer is dirty until the resolve launch is in the queue */
    S.count = 0;
    S.z_armed = false;
    HIPCHK(c, launch_depth_register(S.d_rig + first_pair, S.d_src, depth_format, count, max_px, rows, cols, S.z, S.out, c->stream));
    S.z_armed = true;
    HIPCHK(c, hipEventRecord(S.ev_resolved, c->stream));
    S.resolved_pending = true;
    S.first_pair = first_pair; S.count = count; S.img_rows = rows; S.img_cols = cols; S.stride = stride;
    if (d_out)
        for (int i = 0; i < count; i++) d_out[i] = S.out + stride * i;
    return DVO_OK;
}

int dvo_frames_get_registered_depth(dvo_ctx *c, int pair, unsigned short *out, int capacity, int *rows, int *cols) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    const dvo_depth_state *S = c->depth_reg;
    if (!S || pair < S->first_pair || pair >= S->first_pair + S->count)
        return fail(c, DVO_ERR_STATE, "pair " + std::to_string(pair) + " has no registered depth image (dvo_frames_register_depth)");
    if (rows) *rows = S->img_rows;
    if (cols) *cols = S->img_cols;
    if (!out) return DVO_OK;
    const size_t npx = (size_t)S->img_rows * S->img_cols;
    if (capacity < 0 || (size_t)capacity < npx) return fail(c, DVO_ERR_INVALID, "capacity is smaller than the image (rows * cols pixels)");
    HIPCHK(c, hipMemcpyAsync(out, S->out + S->stride * (size_t)(pair - S->first_pair), sizeof(unsigned short) * npx, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

}  // extern "C"
