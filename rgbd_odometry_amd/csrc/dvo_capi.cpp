/*
 * dvo_capi.cpp -- implementation of the C ABI declared in include/dvo_amd.h: lifecycle, inputs, hot path, inspection
 * (the frame store -- rows f1 + f2 -- is dvo_capi_frames.cpp; both share dvo_ctx.h).
 *
 * Host side only: context + HBM slab management, uploads, kernel launches.
 * There is deliberately no CPU compute path in this file: every compute entry
 * point needs a HIP device and fails with DVO_ERR_NO_DEVICE / DVO_ERR_HIP
 * otherwise.
 *
 * HBM layout ("slabs", sized for batch mode): per pyramid level ONE allocation
 * for the texels of all pairs and ONE for the points of all pairs (see
 * dvo_launch.h::LevelSlab), so a 256-pair 640x480x4 batch is 8 large
 * allocations (~1.7 GB of texels) instead of 2048 small ones.
 */
#include "dvo_ctx.h"
#include "dvo_launch_plan.h"
#include "dvo_palette.h"

#include <atomic>
#include <chrono>
#include <thread>

using namespace dvo;


namespace { thread_local std::string g_create_error; }

namespace dvo_host {

int fail(dvo_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

hipError_t stream_wait(hipStream_t s) {
    ++g_host_waits;
    static const bool block = [] { const char *e = std::getenv("DVO_WAIT"); return e && std::strcmp(e, "block") == 0; }();
    if (!block) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int n = 0;; n++) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) return e;                /* hipSuccess: everything enqueued so far has completed */
            if ((n & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    return hipStreamSynchronize(s);
}

int ensure_staging(dvo_ctx *c, size_t bytes) { return regrow(c, c->staging, (bytes + sizeof(float) - 1) / sizeof(float)); }
int ensure_work(dvo_ctx *c, size_t bytes) { return regrow(c, c->work, (bytes + sizeof(int) - 1) / sizeof(int)); }

bool pair_ok(const dvo_ctx *c, int pair) { return pair >= 0 && pair < c->n_pairs; }
bool level_ok(int level) { return level >= 0 && level < DVO_LEVELS; }

/* make room for N points per pair at `level` (keeps existing contents) */
int ensure_points(dvo_ctx *c, int level, int N) {
    Level &L = c->lv[level];
    if (L.hN.empty()) { L.hN.assign(c->n_pairs, 0); }
    if (L.compact_ok.empty()) L.compact_ok.assign(c->n_pairs, 0);
    if (!L.dN) {
        HIPCHK(c, L.dN.alloc(c->n_pairs));
        HIPCHK(c, hipMemsetAsync(L.dN, 0, sizeof(int) * c->n_pairs, c->stream));
    }
    if (N <= L.pt_cap) return DVO_OK;
    int new_cap = std::max(N, L.pt_cap + L.pt_cap / 4);
    new_cap = (new_cap + 255) / 256 * 256;
    /* all five or none: locals that an early return frees, moved over the old ones once they hold the contents */
    DevBuf<float> np;
    DevBuf<uint2> ncp;
    DevBuf<unsigned> nci, nc4, nch;
    HIPCHK(c, np.alloc(3 * (size_t)new_cap * c->n_pairs));
    HIPCHK(c, ncp.alloc((size_t)new_cap * c->n_pairs));
    HIPCHK(c, nci.alloc((size_t)new_cap * c->n_pairs));
    HIPCHK(c, nc4.alloc((size_t)new_cap * c->n_pairs));
    HIPCHK(c, nch.alloc((size_t)(new_cap / 64) * c->n_pairs));      /* new_cap % 256 == 0 */
    if (!L.d_pt4_ok) {
        HIPCHK(c, L.d_pt4_ok.alloc(c->n_pairs));
        HIPCHK(c, hipMemsetAsync(L.d_pt4_ok, 0, sizeof(int) * (size_t)c->n_pairs, c->stream));
    }
    if (L.pts) {
        HIPCHK(c, hipMemcpy2DAsync(np, sizeof(float) * 3 * (size_t)new_cap, L.pts,
                                   sizeof(float) * 3 * (size_t)L.pt_cap,
                                   sizeof(float) * 3 * (size_t)L.pt_cap, c->n_pairs,
                                   hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(ncp, sizeof(uint2) * (size_t)new_cap, L.cpts, sizeof(uint2) * (size_t)L.pt_cap,
                                   sizeof(uint2) * (size_t)L.pt_cap, c->n_pairs, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(nci, sizeof(unsigned) * (size_t)new_cap, L.cidx, sizeof(unsigned) * (size_t)L.pt_cap,
                                   sizeof(unsigned) * (size_t)L.pt_cap, c->n_pairs, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(nc4, sizeof(unsigned) * (size_t)new_cap, L.cpt4, sizeof(unsigned) * (size_t)L.pt_cap,
                                   sizeof(unsigned) * (size_t)L.pt_cap, c->n_pairs, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(nch, sizeof(unsigned) * (size_t)(new_cap / 64), L.chdr, sizeof(unsigned) * (size_t)(L.pt_cap / 64),
                                   sizeof(unsigned) * (size_t)(L.pt_cap / 64), c->n_pairs, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, stream_wait(c->stream));
    }
    L.pts = std::move(np);
    L.cpts = std::move(ncp);
    L.cidx = std::move(nci);
    L.cpt4 = std::move(nc4);
    L.chdr = std::move(nch);
    L.pt_cap = new_cap;
    c->host_changed();
    return DVO_OK;
}

/* ---- the 16-byte texel slab: dense (hipMalloc) or sparse (virtual range, chunks mapped on demand) --------------------------- */
static bool tex_sparse_wanted(size_t bytes) {
    static const int pol = [] { const char *e = std::getenv("DVO_TEX_SLAB"); return e ? (!std::strcmp(e, "sparse") ? 1 : (!std::strcmp(e, "dense") ? 2 : 0)) : 0; }();
    return pol == 1 || (pol == 0 && bytes >= ((size_t)2 << 30));      /* default: from 2 GiB per level on */
}
void free_texels(dvo_ctx *c, Level &L) {
    if (!L.tex) return;
    if (L.tex_sparse) {
        for (size_t i = 0; i < L.tex_mapped.size(); i++)
            if (L.tex_mapped[i]) {
                (void)hipMemUnmap(reinterpret_cast<char *>(L.tex) + i * L.tex_chunk, L.tex_chunk);
                (void)hipMemRelease(L.tex_handles[i]);
            }
        (void)hipMemAddressFree(L.tex, L.tex_va_bytes);
    } else {
        (void)hipFree(L.tex);
    }
    L.tex = nullptr; L.tex_sparse = false; L.tex_mapped.clear(); L.tex_handles.clear(); L.tex_va_bytes = 0;
    (void)c;
}
/* `stream`: the stream whose work will write the texels next (the zero fill of a fresh chunk must be ordered before that work);
 * nullptr = the context stream */
int map_texels(dvo_ctx *c, int level, int first, int count, hipStream_t stream) {
    Level &L = c->lv[level];
    if (!stream) stream = c->stream;
    if (!L.tex_sparse || count <= 0) return DVO_OK;
    const size_t pair_bytes = sizeof(float4) * L.tex_stride;
    const size_t lo = (size_t)first * pair_bytes / L.tex_chunk, hi = ((size_t)(first + count) * pair_bytes - 1) / L.tex_chunk;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = c->device;
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    for (size_t i = lo; i <= hi; i++) {
        if (L.tex_mapped[i]) continue;
        char *addr = reinterpret_cast<char *>(L.tex) + i * L.tex_chunk;
        hipMemGenericAllocationHandle_t h;
        hipError_t e = hipMemCreate(&h, L.tex_chunk, &prop, 0);
        if (e == hipSuccess) {
            e = hipMemMap(addr, L.tex_chunk, 0, h, 0);
            if (e == hipSuccess) e = hipMemSetAccess(addr, L.tex_chunk, &acc, 1);
            if (e != hipSuccess) { (void)hipMemUnmap(addr, L.tex_chunk); (void)hipMemRelease(h); }
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, DVO_ERR_NOMEM, "cannot back the 16-byte texels of pairs " + std::to_string(first) + ".." + std::to_string(first + count - 1) +
                                              " of level " + std::to_string(level) + " with memory: " + hipGetErrorString(e));
        }
        L.tex_handles[i] = h; L.tex_mapped[i] = 1;
        HIPCHK(c, hipMemsetAsync(addr, 0, L.tex_chunk, stream));      /* tile padding is never read, but keep it defined */
    }
    return DVO_OK;
}
int sparse_map_compact_failures(dvo_ctx *c, int level, int first, int count, hipStream_t stream, int *n_failed) {
    Level &L = c->lv[level];
    std::vector<int> pn((size_t)count);
    HIPCHK(c, hipMemcpyAsync(pn.data(), L.d_pal_n + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, stream_wait(stream));
    std::vector<char> needs_tex((size_t)count);      /* refused, or a partial form: 16-byte texels are (also) its form */
    for (int i = 0; i < count; i++) needs_tex[i] = L.now.w(first + i).learned(pn[i], true);
    int n = 0;
    for (int i = 0; i < count; ) {
        if (!needs_tex[i]) { i++; continue; }
        int j = i;
        while (j < count && needs_tex[j]) j++;
        const int rc = map_texels(c, level, first + i, j - i, stream);
        if (rc) return rc;
        n += j - i;
        i = j;
    }
    *n_failed = n;
    return DVO_OK;
}
/* pal_n of the pairs whose compact form the host has not looked at yet (one copy + one wait per run of such pairs) */
int refresh_compact_known(dvo_ctx *c, int level, int first, int count, bool skip_native) {
    Level &L = c->lv[level];
    if (!L.d_pal_n) return DVO_OK;
    auto unknown = [&](int p) { return L.now[p].needs_readback(skip_native); };
    for (int p = first; p < first + count; ) {
        if (!unknown(p)) { p++; continue; }
        int q = p;
        while (q < first + count && unknown(q)) q++;
        std::vector<int> pn((size_t)(q - p));
        HIPCHK(c, hipMemcpyAsync(pn.data(), L.d_pal_n + p, sizeof(int) * (size_t)(q - p), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_wait(c->stream));
        for (int i = p; i < q; i++) L.now.w(i).learned(pn[i - p], false);
        p = q;
    }
    return DVO_OK;
}

int ensure_texels(dvo_ctx *c, int level, int rows, int cols) {
    Level &L = c->lv[level];
    if (L.tex && L.rows == rows && L.cols == cols) return DVO_OK;
    if (L.tex) {
        HIPCHK(c, stream_wait(c->stream));
        free_texels(c, L);
        L.now.assign(L.now.size(), NowState());
        L.p4.reset(); L.pal.reset(); L.d_pal_n.reset();
    }

    L.rows = rows; L.cols = cols;
    c->host_changed();
    L.tex_stride = texel_count(rows, cols);
    const size_t bytes = sizeof(float4) * L.tex_stride * c->n_pairs;
    if (tex_sparse_wanted(bytes)) {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = c->device;
        size_t gran = 0;
        void *va = nullptr;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) == hipSuccess && gran > 0) {
            const size_t chunk = ((((size_t)16 << 20) + gran - 1) / gran) * gran;         /* ~16 MiB: a few 640x480 pairs per mapping */
            const size_t va_bytes = (bytes + chunk - 1) / chunk * chunk;
            if (hipMemAddressReserve(&va, va_bytes, chunk, nullptr, 0) == hipSuccess && va) {
                L.tex = reinterpret_cast<float4 *>(va);
                L.tex_sparse = true; L.tex_chunk = chunk; L.tex_va_bytes = va_bytes;
                L.tex_handles.assign(va_bytes / chunk, hipMemGenericAllocationHandle_t{});
                L.tex_mapped.assign(va_bytes / chunk, 0);
                return DVO_OK;
            }
        }
        (void)hipGetLastError();                /* no virtual memory management on this runtime: the dense slab */
    }
    HIPCHK(c, hipMalloc((void **)&L.tex, bytes));
    if (L.tex_stride != (size_t)rows * cols)      /* tile padding is never read, but keep it defined */
        HIPCHK(c, hipMemsetAsync(L.tex, 0, bytes, c->stream));
    return DVO_OK;
}

bool native_compact_wanted(const dvo_ctx *c) { return c->prm.engine_variant != 4 && compact_now_policy() != 2; }
/* float images straight to the compact form at dvo_set_now_level: dvo_set_direct_compact, or DVO_DIRECT_COMPACT=on / off in the
 * environment (which wins) */
static bool direct_compact_wanted(const dvo_ctx *c) {
    const char *e = getenv("DVO_DIRECT_COMPACT");
    /* default (round 6): on for batch contexts (64 pairs and more: throughput is what they are for, and the packed kernel on the compact
     * form is 1.7 x the 16-byte route), off for a single stream, whose alignment is latency-bound either way and whose frame would pay
     * 0.16 ms more per installed pair; dvo_set_direct_compact(0 / 1) overrides */
    const bool on = e ? !strcmp(e, "on") : (c->direct_compact < 0 ? c->n_pairs >= 64 : c->direct_compact != 0);
    return native_compact_wanted(c) && on;
}
/* the kernel addresses a pair's rank words with 32-bit byte offsets built from 24-bit multiplies (dvo_palette.h, p4_line_offset) */
static_assert(NowState::PAL_PARTIAL_BIT == DVO_PAL_PARTIAL, "dvo_now_state.h classifies pal_n without dvo_palette.h");
static bool p4_addressable(int rows, int cols) {
    return !(p4_count(rows, cols) * sizeof(unsigned) >= ((size_t)1 << 32) || rows >= (1 << 16) || ((cols + 3) >> 2) >= (1 << 24) ||
             (size_t)p4_tiles_per_col(rows) * 128 >= ((size_t)1 << 24));
}

int ensure_compact_slabs(dvo_ctx *c, int level) {
    Level &L = c->lv[level];
    if (L.p4) return DVO_OK;
    L.p4_stride = p4_count(L.rows, L.cols);
    HIPCHK(c, L.pal.alloc(DVO_PAL_MAX * (size_t)c->n_pairs));
    HIPCHK(c, L.d_pal_n.alloc(c->n_pairs));
    HIPCHK(c, L.p4.alloc(L.p4_stride * c->n_pairs));          /* last: `if (L.p4)` is the test for all three */
    c->host_changed();
    /* complete before anything can write a palette size */
    HIPCHK(c, hipMemsetAsync(L.d_pal_n, 0, sizeof(int) * (size_t)c->n_pairs, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

int now_written_compact(dvo_ctx *c, int level, int first_pair, int count) {
    Level &L = c->lv[level];
    for (int p = first_pair; p < first_pair + count; p++) L.now.w(p).written_compact();
    return DVO_OK;
}

int ensure_tex16(dvo_ctx *c, int level, int first_pair, int count) {
    Level &L = c->lv[level];
    if (!L.p4) return DVO_OK;
    for (int p = first_pair; p < first_pair + count; ) {
        if (L.now[p].texels_real()) { p++; continue; }
        int q = p;
        while (q < first_pair + count && !L.now[q].texels_real()) q++;
        { const int mrc = map_texels(c, level, p, q - p); if (mrc) return mrc; }
        HIPCHK(c, launch_p4_decode_texels(L.p4, L.p4_stride, L.pal, L.d_pal_n, L.tex, L.tex_stride, L.rows, L.cols, p, q - p, c->stream));
        for (int i = p; i < q; i++) L.now.w(i).texels_decoded();
        p = q;
    }
    return DVO_OK;
}

int now_written(dvo_ctx *c, int level, int first_pair, int count) {
    Level &L = c->lv[level];
    const int end = first_pair + count;
    for (int p = first_pair, run = -1; p <= end; p++) {     /* run: first of a run of pairs whose compact form just went stale: the kernel must not read it */
        const bool went_stale = p < end && L.now.w(p).written_texels();
        if (went_stale && run < 0) run = p;
        if (!went_stale && run >= 0) {
            HIPCHK(c, hipMemsetAsync(L.d_pal_n + run, 0, sizeof(int) * (size_t)(p - run), c->stream));
            run = -1;
        }
    }
    return DVO_OK;
}

int build_compact_now(dvo_ctx *c, int level, int first_pair, int count, bool only_reused) {
    Level &L = c->lv[level];
    /* a level beyond the compact form's addressing (> ~800 M pixels) simply keeps the 16-byte form */
    if (!L.tex || !p4_addressable(L.rows, L.cols)) return DVO_OK;
    for (int p = first_pair; p < first_pair + count; ) {
        auto wanted = [&](int i) { return L.now[i].wants_build(only_reused); };
        if (!wanted(p)) { p++; continue; }
        int q = p;
        while (q < first_pair + count && wanted(q)) q++;
        { const int rc = ensure_compact_slabs(c, level); if (rc) return rc; }
        for (int b = p; b < q; b += 1024) {                 /* scratch: 32 KiB per image of a launch */
            const int nb = std::min(1024, q - b);
            { const int rc = regrow(c, c->pal_work, palette_work_ints(nb)); if (rc) return rc; }
            HIPCHK(c, launch_palette_build(L.tex, L.tex_stride, L.rows, L.cols, L.p4, L.p4_stride, L.pal, L.d_pal_n, b, nb, c->pal_work, c->stream));
        }
        for (int i = p; i < q; i++) L.now.w(i).built_compact();      /* the builder may have refused (pal_n < 0) */
        p = q;
    }
    return DVO_OK;
}

}  // namespace dvo_host

using namespace dvo_host;

namespace dvo_host {       /* shared with dvo_capi_tiled.cpp (declared in dvo_ctx.h) */

LevelSlab slab_of(const dvo_ctx *c, int level) {
    const Level &L = c->lv[level];
    LevelSlab s;
    s.tex = L.tex; s.pts = L.pts; s.cpts = L.cpts; s.cidx = L.cidx; s.N = L.dN;
    s.cpt4 = L.cpt4; s.chdr = L.chdr; s.pt4_ok = L.d_pt4_ok;
    s.tex_stride = L.tex_stride; s.pt_cap = L.pt_cap; s.rows = L.rows; s.cols = L.cols;
    s.p4 = L.p4; s.pal = L.pal; s.pal_n = L.d_pal_n; s.p4_stride = L.p4_stride;
    return s;
}

int check_ready(dvo_ctx *c, int pair, int level) {
    if (!c->have_K) return fail(c, DVO_ERR_STATE, "intrinsics not set (dvo_set_intrinsics)");
    const Level &L = c->lv[level];
    if (L.hN.empty() || L.hN[pair] <= 0)
        return fail(c, DVO_ERR_STATE, "reference points of pair " + std::to_string(pair) + " level " +
                                          std::to_string(level) + " not set");
    if (!L.now[pair].ready())
        return fail(c, DVO_ERR_STATE, "now level " + std::to_string(level) + " of pair " +
                                          std::to_string(pair) + " not set");
    return DVO_OK;
}

int build_schedule(dvo_ctx *c, int n_levels, const int *iters, int flags, Schedule &sc) {
    if (n_levels < 1 || n_levels > DVO_LEVELS || !iters) return fail(c, DVO_ERR_INVALID, "bad level schedule");
    std::memset(&sc, 0, sizeof(sc));
    sc.n_levels = n_levels;
    sc.flags = flags;
    sc.last_level = -1;
    int off = 0;
    for (int l = 0; l < n_levels; l++) {
        sc.iters[l] = iters[l] > 0 ? iters[l] : 0;
        sc.e_off[l] = off;
        off += sc.iters[l];
    }
    for (int l = n_levels - 1; l >= 0; l--) if (sc.iters[l] > 0) sc.last_level = l;
    if (sc.last_level < 0) return fail(c, DVO_ERR_INVALID, "schedule has no iterations");
    sc.e_stride = off;
    return DVO_OK;
}

int ensure_outputs(dvo_ctx *c, const Schedule &sc) {
    const size_t need = (size_t)sc.e_stride * c->n_pairs;
    int rc;
    if (need > c->d_energy.size()) {
        c->sched_gen++;              /* earlier energies are gone */
        if ((rc = regrow(c, c->d_energy, need))) return rc;
    }
    if (sc.flags & DVO_FLAG_NORMAL_MATRIX) {
        const size_t needH = need * 21;
        if (needH > c->d_H.size()) {
            c->sched_gen++;
            if ((rc = regrow(c, c->d_H, needH))) return rc;
        }
    }
    if (sc.flags & DVO_FLAG_FINAL_OUTPUTS) {
        const int cap = c->lv[sc.last_level].pt_cap;
        if (cap > c->final_cap) {
            c->sched_gen++;          /* earlier final outputs are gone */
            c->final_cap = 0;        /* the capacity of BOTH buffers: stays 0 unless both grow */
            if (c->d_final_eps) HIPCHK(c, stream_wait(c->stream));
            c->d_final_eps.reset(); c->d_final_reproj.reset();
            HIPCHK(c, c->d_final_eps.alloc((size_t)cap * c->n_pairs));
            HIPCHK(c, c->d_final_reproj.alloc(3 * (size_t)cap * c->n_pairs));
            c->final_cap = cap;
        }
    }
    return DVO_OK;
}

/* the outputs of pairs [first, first+n) now follow schedule `sc`; a schedule with another layout invalidates what
 * other pairs reported before (their energies sit at other offsets) */
void stamp_outputs(dvo_ctx *c, const Schedule &sc, int first, int n) {
    const bool same_layout = c->have_sched && c->sched.n_levels == sc.n_levels && c->sched.e_stride == sc.e_stride &&
                             std::memcmp(c->sched.iters, sc.iters, sizeof(sc.iters)) == 0 &&
                             ((c->sched.flags ^ sc.flags) & (DVO_FLAG_FINAL_OUTPUTS | DVO_FLAG_NORMAL_MATRIX)) == 0 &&
                             c->sched.last_level == sc.last_level && c->sched.final_blk == sc.final_blk;
    if (!same_layout || c->sched_gen == 0) c->sched_gen++;
    c->host_changed();           /* enqueue()'s memo skips these loops only while nothing else has stamped */
    if (c->pair_gen.empty()) c->pair_gen.assign(c->n_pairs, 0);
    for (int p = first; p < first + n; p++) c->pair_gen[p] = c->sched_gen;
    if (c->final_list_gen.empty()) c->final_list_gen.assign(c->n_pairs, 0);
    const Level &Lf = c->lv[sc.last_level];
    for (int p = first; p < first + n; p++) {
        const int dp = (sc.alias_mod > 0) ? p % sc.alias_mod : p;
        c->final_list_gen[p] = Lf.list_gen.empty() ? 0 : Lf.list_gen[dp];
    }
}
void ref_list_written(dvo_ctx *c, int level, int first, int n, int rows) {
    Level &L = c->lv[level];
    if (L.list_gen.empty()) { L.list_gen.assign(c->n_pairs, 0); L.pt4_rows.assign(c->n_pairs, 0); }
    c->points_gen++;
    for (int p = first; p < first + n; p++) { L.list_gen.w(p) = c->points_gen; L.pt4_rows.w(p) = rows; }
}
bool outputs_valid(const dvo_ctx *c, int pair) {
    return c->have_sched && !c->pair_gen.empty() && c->pair_gen[pair] == c->sched_gen;
}

Outputs outputs_of(const dvo_ctx *c) {
    Outputs o;
    o.poses = c->d_poses; o.energy = c->d_energy; o.best_idx = c->d_best; o.ratio = c->d_ratio;
    o.final_eps = c->d_final_eps; o.final_reproj = c->d_final_reproj; o.final_N = c->d_final_N;
    o.final_cap = c->final_cap;
    o.tex_mode = c->d_tex_mode;
    o.H = c->d_H;
    o.team_buf = c->d_team_buf;
    o.team_cnt = c->d_team_cnt;
    o.team_err = reinterpret_cast<int *>(c->d_team_cnt ? c->d_team_cnt + c->n_pairs : nullptr);
    o.order = nullptr;
    return o;
}

void cast_pose(const double *R, const double *t, float *Rf, float *tf) {
    for (int k = 0; k < 9; k++) Rf[k] = (float)R[k];       /* cR.cast<float>()  SolveDVO.cpp:673 */
    for (int k = 0; k < 3; k++) tf[k] = (float)t[k];       /* :674 */
}

/* the tiers of team launches for the coarse levels of the wide / tiled schedule (dvo_launch_plan.h: plan_wide_tiers), with the
 * limits DVO_WIDE_TEAM_MAX=a,b asks for (0 switches the team launches off; tests) */
static const TeamTiers &team_tiers() {
    static const TeamTiers t = [] {
        TeamTiers v;
        if (const char *e = std::getenv("DVO_WIDE_TEAM_MAX")) { int a = 0, b = -1; const int n = std::sscanf(e, "%d,%d", &a, &b); v.lim[0] = a; v.lim[1] = n > 1 ? b : a; }
        return v;
    }();
    return t;
}
static bool team_tiers_possible(const dvo_ctx *c, int flags) {
    return team_tiers().lim[1] > 0 && !(flags & DVO_FLAG_NORMAL_MATRIX) && !c->prm.interpolate_dt && c->prm.engine_variant != 1 && c->prm.team_size == 0 &&
           c->n_cu >= 64 && c->stream != nullptr;
}

/* ---- one fused alignment launch: enqueue() and its stages.  WHAT to launch is decided by dvo_launch_plan.h from the facts gathered
 * here; the stages below carry it out.  A full pass over a resident batch walks every pair at every level several times; what it
 * decided is remembered (dvo_launch_memo.h) and a repeated request on unchanged host state goes straight to the launch --------- */
static_assert(PLAN_NACC_PAD == DVO_NACC_PAD && PLAN_PALETTE_BYTES == sizeof(float2) * DVO_PAL_MAX && PLAN_SOLO_MAX == DVO_TILED_SOLO_MAX_DEFAULT,
              "dvo_launch_plan.h restates constants of dvo_launch.h and dvo_palette.h");

struct EnqueueRequest {
    int first_pair = 0, n_pairs = 0;
    int n_levels = 0;
    const int *iters = nullptr;
    int flags = 0;
    /* the levels THIS launch runs (the energy layout stays that of the whole schedule `iters`): the wide schedule hands its
     * coarse levels to the fused team kernel and keeps the fine ones for its step launches (round 6, dvo_align_pyramid_wide) */
    unsigned level_mask = ~0u;
    /* index-list form (the multi-stream tracker): the launch aligns pairs h_list[0 .. n_pairs) -- any set, in that order --
     * through the launch-order array of the packed kernel (d_list: the same indices on the device); first_pair must be 0.  No team mode. */
    const int *h_list = nullptr, *d_list = nullptr;
    int forced_team = 0;            /* a tier of the wide / tiled schedule: this team size instead of dvo_params.team_size (0: that) */
    int pair(int i) const { return h_list ? h_list[i] : first_pair + i; }
};

static EnqueueRequest range_request(int first_pair, int n_pairs, int n_levels, const int *iters, int flags) {
    EnqueueRequest q;
    q.first_pair = first_pair; q.n_pairs = n_pairs; q.n_levels = n_levels; q.iters = iters; q.flags = flags;
    return q;
}

/* the range helpers take contiguous pairs: one call of fn(first, count) per run of consecutive pairs of the request */
template <class Fn>
static int for_each_run(const EnqueueRequest &q, Fn fn) {
    for (int a = 0; a < q.n_pairs;) {
        int b = a + 1;
        while (b < q.n_pairs && q.pair(b) == q.pair(b - 1) + 1) b++;
        const int r = fn(q.pair(a), b - a);
        if (r) return r;
        a = b;
    }
    return DVO_OK;
}

/* arguments, the schedule with the level mask applied, readiness, output buffers, which point lists are compact */
static int validate_and_schedule(dvo_ctx *c, const EnqueueRequest &q, Schedule &sc) {
    if (q.h_list) {
        if (q.first_pair != 0 || q.n_pairs < 1 || q.n_pairs > c->n_pairs || !q.d_list) return fail(c, DVO_ERR_INVALID, "bad pair list");
        for (int i = 0; i < q.n_pairs; i++) if (!pair_ok(c, q.h_list[i])) return fail(c, DVO_ERR_INVALID, "pair list entry out of bounds");
    } else if (!pair_ok(c, q.first_pair) || q.n_pairs < 1 || q.first_pair + q.n_pairs > c->n_pairs)
        return fail(c, DVO_ERR_INVALID, "pair range out of bounds");
    int rc = build_schedule(c, q.n_levels, q.iters, q.flags, sc);
    if (rc) return rc;
    if (q.level_mask != ~0u) {
        sc.last_level = -1;
        for (int l = 0; l < q.n_levels; l++) if (!((q.level_mask >> l) & 1u)) sc.iters[l] = 0;
        for (int l = q.n_levels - 1; l >= 0; l--) if (sc.iters[l] > 0) sc.last_level = l;
        if (sc.last_level < 0) return fail(c, DVO_ERR_INVALID, "schedule has no iterations");
    }
    for (int l = 0; l < q.n_levels; l++) {
        if (sc.iters[l] <= 0) continue;
        for (int i = 0; i < q.n_pairs; i++)
            if ((rc = check_ready(c, q.pair(i), l))) return rc;
    }
    if ((rc = ensure_outputs(c, sc))) return rc;
    sc.alias_mod = c->prm.debug_alias_mod > 0 ? c->prm.debug_alias_mod : 0;
    /* compact (8-byte) point lists when every list of this launch was built by the engine's own enlist kernels */
    sc.compact = fused_uses_compact(c->prm.points_in_flight, c->prm.interpolate_dt) ? 1 : 0;
    for (int l = 0; l < q.n_levels && sc.compact; l++) {
        if (sc.iters[l] <= 0) continue;
        for (int i = 0; i < q.n_pairs && sc.compact; i++) {
            const int p = q.pair(i);
            if (c->lv[l].compact_ok.empty() || !c->lv[l].compact_ok[sc.alias_mod > 0 ? p % sc.alias_mod : p]) sc.compact = 0;
        }
    }
    return DVO_OK;
}

/* what plan_launch reads (all_p4 comes from prepare_now_forms) */
static LaunchFacts gather_facts(const dvo_ctx *c, const EnqueueRequest &q, const Schedule &sc) {
    LaunchFacts f;
    f.block_threads = c->prm.block_threads; f.lds_point_bytes = c->prm.lds_point_bytes; f.points_in_flight = c->prm.points_in_flight;
    f.engine_variant = c->prm.engine_variant; f.interpolate_dt = c->prm.interpolate_dt;
    f.team_size = q.forced_team ? q.forced_team : c->prm.team_size;
    f.compact_now_policy = compact_now_policy();
    f.n_cu = c->n_cu; f.n_pairs = q.n_pairs; f.listed = q.h_list != nullptr; f.flags = sc.flags;
    f.compact = sc.compact != 0;
    f.has_pair_K = (bool)c->d_pair_K;
    const bool block_auto = plan_block_auto(f);
    for (int l = 0; l < q.n_levels && block_auto; l++) {
        if (sc.iters[l] <= 0) continue;
        for (int i = 0; i < q.n_pairs; i++) f.max_n = std::max(f.max_n, c->lv[l].hN[q.pair(i)]);
    }
    if (plan_team_by_n_fine(f))
        for (int p = q.first_pair; p < q.first_pair + q.n_pairs; p++) f.n_fine = std::max(f.n_fine, c->lv[sc.last_level].hN[p]);
    for (int l = 0; l < q.n_levels && !f.pt4_rows_mismatch; l++) {
        if (sc.iters[l] <= 0 || c->lv[l].pt4_rows.empty()) continue;
        const Level &L = c->lv[l];
        for (int i = 0; i < q.n_pairs; i++) {
            const int p = q.pair(i);
            const int dp = sc.alias_mod > 0 ? p % sc.alias_mod : p;
            if (L.pt4_rows[dp] != 0 && L.pt4_rows[dp] != L.rows) { f.pt4_rows_mismatch = true; break; }
        }
    }
    const int blocks[3] = {256, 512, 1024};
    for (int b = 0; b < 3; b++) { f.fused2_lds[b][0] = (int)fused2_static_lds(blocks[b], false); f.fused2_lds[b][1] = (int)fused2_static_lds(blocks[b], true); }
    f.pose_state_bytes = (int)pose_state_bytes();
    return f;
}

/* compact form of the now levels (dvo_palette.h): built for a level that has been aligned DVO_COMPACT_NOW_AFTER times (or
 * up front by dvo_now_prepare) -- the build costs about 4.4 alignments and saves 0.28 of one per use: a now level aligned
 * once or twice never repays it.  f.all_p4: every now level of the launch has the form */
static int prepare_now_forms(dvo_ctx *c, const EnqueueRequest &q, const Schedule &sc, LaunchFacts &f, bool &build_possible) {
    f.all_p4 = true;
    build_possible = false;
    if (!plan_reads_compact_now(f)) return DVO_OK;
    int rc;
    for (int l = 0; l < q.n_levels; l++) {
        if (sc.iters[l] <= 0) continue;
        if ((rc = for_each_run(q, [&](int first, int n) { return build_compact_now(c, l, first, n, compact_now_policy() != 1); }))) return rc;
        Level &L = c->lv[l];
        for (int i = 0; i < q.n_pairs; i++) { const int p = q.pair(i); L.now_used(p); f.all_p4 = f.all_p4 && L.now[p].built; }
    }
    build_possible = !f.all_p4;      /* a form that is not built is built once its use count says so: the memo must keep counting */
    for (int l = 0; l < q.n_levels && f.all_p4 && shape_depends_on_refusals(f); l++) {
        if (sc.iters[l] <= 0) continue;
        if ((rc = for_each_run(q, [&](int first, int n) { return refresh_compact_known(c, l, first, n, true); }))) return rc;      /* natively written forms are never refused: no read-back, no wait */
        const Level &L = c->lv[l];
        int refused = 0;
        for (int i = 0; i < q.n_pairs; i++) refused += (L.now[q.pair(i)].known == NowState::P4_REFUSED);
        if (too_many_refused(refused, q.n_pairs)) f.all_p4 = false;
    }
    return DVO_OK;
}

/* the 16-byte texels of every now level of the launch */
static int ensure_tex16_of_launch(dvo_ctx *c, const EnqueueRequest &q, const Schedule &sc) {
    int rc;
    for (int l = 0; l < q.n_levels; l++) {
        if (sc.iters[l] <= 0) continue;
        if ((rc = for_each_run(q, [&](int first, int n) { return ensure_tex16(c, l, first, n); }))) return rc;
        if (sc.alias_mod > 0 && (rc = ensure_tex16(c, l, 0, std::min(sc.alias_mod, c->n_pairs)))) return rc;
    }
    return DVO_OK;
}

/* the exchange records of a team launch (dvo_launch_plan.h: team_epoch_step); sets sc.team_epoch0.  The only place that
 * touches d_team_buf, d_team_cnt, team_epoch, team_legacy and team_err_dirty on the way to a launch */
static int team_exchange_prepare(dvo_ctx *c, Schedule &sc) {
    const size_t buf_bytes = 16 * 2 * 32 * 8 * (size_t)std::max(c->n_pairs, 9);     /* 16-byte records, [2][32][8] per pair (a team over all XCDs: 8 + 1 slots) */
    bool first_use = false;
    if (!c->d_team_buf) {
        HIPCHK(c, c->d_team_cnt.alloc((size_t)c->n_pairs + 1));
        HIPCHK(c, c->d_team_buf.alloc(buf_bytes / sizeof(double)));
        first_use = c->team_err_dirty = true;
        /* tests: start the count close to its 32-bit end, so that a few alignments cross the wrap (read when the buffer is made) */
        if (const char *e = std::getenv("DVO_TEAM_EPOCH0")) c->team_epoch = (unsigned)std::strtoul(e, nullptr, 0);
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (c->stream && hipStreamIsCapturing(c->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) c->team_legacy = true;
    const TeamEpochStep step = team_epoch_step(c->team_epoch, team_exchanges_needed(sc.iters, sc.n_levels), c->team_legacy, first_use);
    if (step.zero_records) HIPCHK(c, hipMemsetAsync(c->d_team_buf, 0, buf_bytes, c->stream));
    if (c->team_err_dirty || c->team_legacy) {
        HIPCHK(c, hipMemsetAsync(c->d_team_cnt, 0, sizeof(unsigned) * ((size_t)c->n_pairs + 1), c->stream));
        c->team_err_dirty = false;
    }
    sc.team_epoch0 = step.epoch0;
    c->team_epoch = step.next_epoch;
    return DVO_OK;
}

/* the launch order of a batch of more pairs than compute units (dvo_launch_plan.h: launch_order), made and uploaded
 * once per resident batch; *order = c->d_order */
static int resident_order(dvo_ctx *c, const EnqueueRequest &q, const Schedule &sc, const int **order) {
    unsigned long long sched_hash = 1469598103934665603ull;
    for (int l = 0; l < q.n_levels; l++) sched_hash = (sched_hash ^ (unsigned long long)(unsigned)sc.iters[l]) * 1099511628211ull;
    const unsigned long long key[4] = {c->points_gen, (unsigned long long)q.first_pair, (unsigned long long)q.n_pairs, sched_hash};
    if (!c->d_order || std::memcmp(key, c->order_key, sizeof(key)) != 0) {
        std::vector<long long> work((size_t)q.n_pairs);
        for (int p = 0; p < q.n_pairs; p++) {
            long long w = 0;
            for (int l = 0; l < q.n_levels; l++) w += (long long)sc.iters[l] * c->lv[l].hN[q.first_pair + p];
            work[p] = w;
        }
        c->h_order.resize((size_t)q.n_pairs);
        launch_order(work.data(), q.n_pairs, c->h_order.data());
        { const int rc = regrow(c, c->d_order, (size_t)c->n_pairs); if (rc) return rc; }
        HIPCHK(c, stream_wait(c->stream));          /* an earlier launch may still read the old order */
        HIPCHK(c, hipMemcpyAsync(c->d_order, c->h_order.data(), sizeof(int) * (size_t)q.n_pairs, hipMemcpyHostToDevice, c->stream));
        std::memcpy(c->order_key, key, sizeof(key));
        c->host_changed();         /* d_order now holds this request's order, and no other's */
    }
    *order = c->d_order;
    return DVO_OK;
}

/* the outputs of the launch's pairs follow `sc` now */
static void stamp_launch(dvo_ctx *c, const EnqueueRequest &q, const Schedule &sc) {
    if (!q.h_list) stamp_outputs(c, sc, q.first_pair, q.n_pairs);
    else stamp_outputs(c, sc, q.h_list[0], 1);
    c->sched = sc;
    c->have_sched = true;
    for (int i = 1; q.h_list && i < q.n_pairs; i++) stamp_outputs(c, sc, q.h_list[i], 1);     /* same layout now: no generation bump */
}

/* the stages that decide: the final Schedule (all but final_blk and team_epoch0, which the launch sets) and the LaunchPlan */
static int decide_launch(dvo_ctx *c, const EnqueueRequest &q, Schedule &sc, LaunchPlan &plan, bool &build_possible) {
    int rc = validate_and_schedule(c, q, sc);
    if (rc) return rc;
    LaunchFacts facts = gather_facts(c, q, sc);
    if ((rc = prepare_now_forms(c, q, sc, facts, build_possible))) return rc;
    plan = plan_launch(facts);
    if (plan.err) return fail(c, plan.err, plan.msg);
    sc.no_p4 = plan.no_p4; sc.no_pt4 = plan.no_pt4;
    sc.lds_bytes = plan.lds_bytes; sc.lds_points = plan.lds_points;
    sc.no_lds_tex = plan.no_lds_tex; sc.force_exact = plan.force_exact; sc.force_e2 = plan.force_e2; sc.no_pt4_direct = plan.no_pt4_direct;
    sc.team = plan.team;
    sc.n_pairs_launch = q.n_pairs;
    return DVO_OK;
}

static MemoKey memo_key_now(const dvo_ctx *c, const EnqueueRequest &q) {
    MemoKey k;
    k.q = memo_request(q.first_pair, q.n_pairs, q.n_levels, q.iters, q.flags, q.level_mask, q.forced_team, q.h_list != nullptr);
    k.host_gen = c->host_gen;
    k.sched_gen = c->sched_gen; k.final_cap = c->final_cap;
    k.energy_size = c->d_energy.size(); k.h_size = c->d_H.size();
    return k;
}

/* DVO_LAUNCH_MEMO=verify: the full stages on a hit must decide what was remembered, and change nothing on the host */
static int memo_verify(dvo_ctx *c, const EnqueueRequest &q) {
    const unsigned long long gen0 = c->host_gen;
    Schedule sc;
    LaunchPlan plan;
    bool build_possible = false;
    const int rc = decide_launch(c, q, sc, plan, build_possible);
    if (rc) return rc;
    const Schedule &ms = c->memo_sched;
    const LaunchPlan &mp = c->memo_plan;
    const char *bad = nullptr;
#define MEMO_SAME(a, b, field) if (!bad && std::memcmp(&(a).field, &(b).field, sizeof((a).field)) != 0) bad = #field
    MEMO_SAME(sc, ms, n_levels); MEMO_SAME(sc, ms, iters); MEMO_SAME(sc, ms, e_off); MEMO_SAME(sc, ms, e_stride); MEMO_SAME(sc, ms, last_level);
    MEMO_SAME(sc, ms, flags); MEMO_SAME(sc, ms, alias_mod); MEMO_SAME(sc, ms, lds_points); MEMO_SAME(sc, ms, lds_bytes); MEMO_SAME(sc, ms, no_lds_tex);
    MEMO_SAME(sc, ms, no_p4); MEMO_SAME(sc, ms, team); MEMO_SAME(sc, ms, n_pairs_launch); MEMO_SAME(sc, ms, force_e2); MEMO_SAME(sc, ms, force_exact);
    MEMO_SAME(sc, ms, compact); MEMO_SAME(sc, ms, no_pt4); MEMO_SAME(sc, ms, no_pt4_direct); MEMO_SAME(sc, ms, team_epoch0);
    if (!bad && ms.final_blk != (plan.packed ? 1 : 0)) bad = "final_blk";       /* set at the launch */
    MEMO_SAME(plan, mp, err); MEMO_SAME(plan, mp, packed); MEMO_SAME(plan, mp, block); MEMO_SAME(plan, mp, points_in_flight);
    MEMO_SAME(plan, mp, lds_bytes); MEMO_SAME(plan, mp, lds_points); MEMO_SAME(plan, mp, no_p4); MEMO_SAME(plan, mp, no_pt4);
    MEMO_SAME(plan, mp, no_lds_tex); MEMO_SAME(plan, mp, force_exact); MEMO_SAME(plan, mp, force_e2); MEMO_SAME(plan, mp, no_pt4_direct);
    MEMO_SAME(plan, mp, needs_tex16); MEMO_SAME(plan, mp, team); MEMO_SAME(plan, mp, super_team); MEMO_SAME(plan, mp, team_fallback);
#undef MEMO_SAME
    if (!bad && build_possible) bad = "build_possible";
    if (!bad && c->host_gen != gen0) bad = "host_gen (the stages wrote host state)";
    if (!bad && c->memo_order != (plan.packed && q.n_pairs > c->n_cu)) bad = "order";
    if (bad) return fail(c, DVO_ERR_STATE, std::string("DVO_LAUNCH_MEMO=verify: the remembered launch differs from a full pass in ") + bad);
    return DVO_OK;
}

/* the launch of a remembered pass: the slabs and outputs as they are now, no walk over the pairs */
static int enqueue_remembered(dvo_ctx *c, const EnqueueRequest &q) {
    const Schedule &sc = c->memo_sched;
    const LaunchPlan &plan = c->memo_plan;
    LevelSet ls;
    for (int l = 0; l < DVO_LEVELS; l++) ls.l[l] = slab_of(c, l);
    Outputs o = outputs_of(c);
    if (plan.packed) {
        if (c->memo_order) o.order = c->d_order;
        HIPCHK(c, launch_align_fused2(plan.block, ls, sc, c->K, c->dprm, o, q.first_pair, q.n_pairs, c->stream));
    }
    else
        HIPCHK(c, launch_align_fused(plan.block, plan.points_in_flight, ls, sc, c->K, c->dprm, o, q.first_pair, q.n_pairs, c->stream));
    c->team_used = false;
    c->last_block = plan.block; c->last_team = sc.team;
    c->last_packed = plan.packed ? 1 : 0;
    /* the stamp of the remembered pass covers exactly this range and nothing has stamped since (stamp_outputs moves the
     * generation of the key); should the context's schedule not be the remembered one all the same, stamp as a full pass does */
    if (!c->have_sched || std::memcmp(&c->sched, &sc, sizeof(sc)) != 0) stamp_launch(c, q, sc);
    c->memo.hits++;
    return DVO_OK;
}

int enqueue(dvo_ctx *c, const EnqueueRequest &q) {
    int rc;
    if (c->memo.valid && c->memo.matches(memo_key_now(c, q))) {
        if (c->memo_mode == MEMO_VERIFY && (rc = memo_verify(c, q))) return rc;
        return enqueue_remembered(c, q);
    }
    c->memo.forget();
    c->memo.full_passes++;
    Schedule sc;
    LaunchPlan plan;
    bool build_possible = false;
    if ((rc = decide_launch(c, q, sc, plan, build_possible))) return rc;
    if (plan.needs_tex16 && (rc = ensure_tex16_of_launch(c, q, sc))) return rc;
    c->team_used = plan.team > 1;
    if (plan.team > 1 && (rc = team_exchange_prepare(c, sc))) return rc;
    LevelSet ls;
    for (int l = 0; l < DVO_LEVELS; l++) ls.l[l] = slab_of(c, l);
    bool ordered = false;
    if (plan.packed) {
        Outputs o = outputs_of(c);
        if (q.h_list) o.order = q.d_list;             /* workgroup b aligns pair first_pair (0) + d_list[b] */
        else if (plan.team == 1 && q.n_pairs > c->n_cu) {
            if ((rc = resident_order(c, q, sc, &o.order))) return rc;
            ordered = true;
        }
        sc.final_blk = 1;            /* the packed kernel stores its final outputs in the order of the compact lists */
        hipError_t le = launch_align_fused2(plan.block, ls, sc, c->K, c->dprm, o, q.first_pair, q.n_pairs, c->stream);
        if (le != hipSuccess && sc.team > 1 && plan.team_fallback) {
            /* the runtime could not make the whole team launch resident at once (something else holds compute units or LDS):
             * the same batch without teams -- slower for a small batch, same results up to the order of the double sums */
            sc.team = 1;
            c->team_used = false;
            le = launch_align_fused2(plan.block, ls, sc, c->K, c->dprm, o, q.first_pair, q.n_pairs, c->stream);
        }
        HIPCHK(c, le);
    }
    else
        HIPCHK(c, launch_align_fused(plan.block, plan.points_in_flight, ls, sc, c->K, c->dprm, outputs_of(c),
                                     q.first_pair, q.n_pairs, c->stream));
    c->last_block = plan.block; c->last_team = sc.team;
    c->last_packed = plan.packed ? 1 : 0;
    stamp_launch(c, q, sc);
    /* remember the pass where an identical second call would be this one launch and nothing else (dvo_launch_memo.h); the
     * key is taken now, after everything the pass itself wrote.  No 16-byte texels are pending: the pass has just decoded what
     * the plan reads */
    c->memo.record(memo_key_now(c, q), c->memo_mode, plan.team, false, build_possible);
    if (c->memo.valid) { c->memo_sched = sc; c->memo_plan = plan; c->memo_order = ordered; }
    return DVO_OK;
}

}  // namespace dvo_host

extern "C" {

int dvo_params_default(dvo_params *p) {
    if (!p) return DVO_ERR_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->beta = 0.5;
    p->precond_rot = .5;
    p->reg_lambda = 0.05;
    p->step_a = 9.0;
    p->step_b = 1.0E-2;
    p->step_decay_after = 5;
    p->step_decay_offset = 4;
    p->trust_radius = 0.003;
    p->psi_norm_stop = 1.0E-7;
    p->enable_rotationize = 1;
    p->enable_l2_reg = 1;
    p->interpolate_dt = 0;
    p->block_threads = 0;
    return DVO_OK;
}

int dvo_create_batch(const dvo_params *p, int n_pairs, dvo_ctx **out) {
    if (!out) return fail(nullptr, DVO_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_pairs < 1) return fail(nullptr, DVO_ERR_INVALID, "n_pairs must be >= 1");
    dvo_params prm;
    if (p) prm = *p; else dvo_params_default(&prm);
    std::string why;
    if (const int rc = device_check(&why)) return fail(nullptr, rc, why);
    dvo_ctx *c = new dvo_ctx();
    c->prm = prm;
    c->n_pairs = n_pairs;
    c->memo_mode = memo_mode(std::getenv("DVO_LAUNCH_MEMO"));
    for (Level &L : c->lv) L.now.assign((size_t)n_pairs, NowState());
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess) c->device = dev;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0)
            c->n_cu = prop.multiProcessorCount;
    }
    c->dprm.beta = prm.beta; c->dprm.precond_rot = prm.precond_rot; c->dprm.reg_lambda = prm.reg_lambda;
    c->dprm.step_a = prm.step_a; c->dprm.step_b = prm.step_b;
    c->dprm.trust_radius = (double)prm.trust_radius;        /* widened at use, SolveDVO.cpp:835 */
    c->dprm.psi_norm_stop = (double)prm.psi_norm_stop;      /* :872 */
    c->dprm.step_decay_after = prm.step_decay_after; c->dprm.step_decay_offset = prm.step_decay_offset;
    c->dprm.enable_rotationize = prm.enable_rotationize; c->dprm.enable_l2_reg = prm.enable_l2_reg;
    c->dprm.interpolate_dt = prm.interpolate_dt ? 1 : 0;
#define CRCHK(expr)                                                                                     \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            fail(nullptr, DVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));              \
            dvo_destroy(c);                                                                             \
            return DVO_ERR_HIP;                                                                         \
        }                                                                                               \
    } while (0)
    CRCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CRCHK(c->d_poses.alloc((size_t)12 * n_pairs));
    CRCHK(c->d_best.alloc((size_t)DVO_LEVELS * n_pairs));
    CRCHK(c->d_ratio.alloc((size_t)DVO_LEVELS * n_pairs));
    CRCHK(c->d_final_N.alloc(n_pairs));
    CRCHK(c->d_tex_mode.alloc((size_t)DVO_LEVELS * n_pairs));
    CRCHK(hipMemset(c->d_tex_mode, 0xff, sizeof(int) * DVO_LEVELS * n_pairs));
    CRCHK(c->d_scratch.alloc(1024 * DVO_NACC_PAD + 64));
    CRCHK(hipMemset(c->d_best, 0xff, sizeof(int) * DVO_LEVELS * n_pairs));
    CRCHK(hipMemset(c->d_ratio, 0, sizeof(float) * DVO_LEVELS * n_pairs));
    CRCHK(hipMemset(c->d_final_N, 0, sizeof(int) * n_pairs));
    {   /* identity poses */
        std::vector<double> id((size_t)12 * n_pairs, 0.0);
        for (int p_ = 0; p_ < n_pairs; p_++) { id[12 * p_] = id[12 * p_ + 4] = id[12 * p_ + 8] = 1.0; }
        CRCHK(hipMemcpy(c->d_poses, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice));
    }
#undef CRCHK
    *out = c;
    if (const char *e = std::getenv("DVO_KEEP_WARM")) {       /* "busy_us,pause_us" */
        int busy = 0, pause = 0;
        if (std::sscanf(e, "%d,%d", &busy, &pause) >= 1 && busy > 0) (void)dvo_set_keep_warm2(c, busy, pause);
    }
    return DVO_OK;
}

int dvo_create(const dvo_params *p, dvo_ctx **out) { return dvo_create_batch(p, 1, out); }

/* ---- keep-warm: a single camera stream leaves the GPU idle ~30 ms between frames (ros::Rate(35), SolveDVO.cpp:1945).  On this
 * pool a process that only ever submits such sparse work finds the GPU parked at its lowest clocks and never raises them: every
 * 0.5 ms alignment then takes 15-30 ms (profiles/r03_single_stream: the C++ replay as the second process on a box).  A host
 * thread of the context keeps ONE wave busy -- launches of `busy_us` microseconds of real time, `pause_us` apart, on a stream of
 * its own -- which is what the power management reads as load.  Off by default (a batch workload never idles); the
 * environment variable DVO_KEEP_WARM="busy_us,pause_us" switches it on for every new context (deployment knob: no code
 * change, no privileges -- the alternative is an administrator pinning the performance level with rocm-smi). */
struct dvo_keep_warm_state {
    std::thread th;
    std::atomic<bool> stop{false};
    hipStream_t stream = nullptr;
    int busy_us = 0, pause_us = 0;
};
static void keep_warm_stop(dvo_ctx *c) {
    dvo_keep_warm_state *w = c->warm;
    if (!w) return;
    w->stop.store(true);
    if (w->th.joinable()) w->th.join();
    if (w->stream) { (void)hipStreamSynchronize(w->stream); (void)hipStreamDestroy(w->stream); }
    delete w;
    c->warm = nullptr;
}
int dvo_set_keep_warm2(dvo_ctx *c, int busy_us, int pause_us) {
    DVO_ENTER(c);
    keep_warm_stop(c);
    if (busy_us <= 0) return DVO_OK;
    dvo_keep_warm_state *w = new dvo_keep_warm_state();
    w->busy_us = busy_us; w->pause_us = pause_us < 0 ? 0 : pause_us;
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) { delete w; return fail(c, DVO_ERR_HIP, "keep-warm: cannot create a stream"); }
    const int device = c->device;
    w->th = std::thread([w, device]() {
        (void)hipSetDevice(device);
        while (!w->stop.load()) {
            (void)launch_keep_warm(w->busy_us, w->stream);
            if (w->pause_us == 0) (void)launch_keep_warm(w->busy_us, w->stream);     /* back to back: the next one is queued already */
            (void)hipStreamSynchronize(w->stream);                                    /* never more than two launches queued */
            if (w->pause_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(w->pause_us));
        }
    });
    c->warm = w;
    return DVO_OK;
}
int dvo_set_keep_warm(dvo_ctx *c, int period_us) {          /* a short launch every period_us microseconds */
    return dvo_set_keep_warm2(c, period_us > 0 ? 5 : 0, period_us);
}

int dvo_destroy(dvo_ctx *c) {
    if (!c) return DVO_OK;
    DeviceGuard guard(c);
    keep_warm_stop(c);
    if (c->stream) (void)stream_wait(c->stream);
    for (int l = 0; l < DVO_LEVELS; l++) free_texels(c, c->lv[l]);
    tiled_forget(c);
    photo_forget(c);
    depth_forget(c);
    if (c->wide_exec) (void)hipGraphExecDestroy(c->wide_exec);
    if (c->tiled_exec) (void)hipGraphExecDestroy(c->tiled_exec);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;           /* frees every buffer the context owns, and the upload ring's copy streams and events: under the guard, after the wait */
    return DVO_OK;
}

const char *dvo_last_error(const dvo_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }
int dvo_num_pairs(const dvo_ctx *c) { return c ? c->n_pairs : 0; }

int dvo_set_stream(dvo_ctx *c, void *hip_stream) {
    DVO_ENTER(c);
    HIPCHK(c, stream_wait(c->stream));
    c->stream = (hipStream_t)hip_stream;
    return DVO_OK;
}
int dvo_use_own_stream(dvo_ctx *c) {
    DVO_ENTER(c);
    HIPCHK(c, stream_wait(c->stream));
    c->stream = c->own_stream;
    return DVO_OK;
}
int dvo_synchronize(dvo_ctx *c) {
    DVO_ENTER(c);
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

int dvo_set_intrinsics(dvo_ctx *c, float fx, float fy, float cx, float cy) {
    DVO_ENTER(c);
    if (!(fx > 0.0f) || !(fy > 0.0f)) return fail(c, DVO_ERR_INVALID, "fx, fy must be positive");
    if (c->have_K && (c->K.fx != fx || c->K.fy != fy || c->K.cx != cx || c->K.cy != cy))
        for (int l = 0; l < DVO_LEVELS; l++)          /* compact lists are expanded with K at run time: those built under the old K lose the short form */
            c->lv[l].compact_ok.fill(0);
    c->K = Intrinsics{fx, fy, cx, cy, c->prm.interpolate_dt ? 1 : 0, 0, c->d_pair_K};
    c->have_K = true;
    c->host_changed();
    if (c->d_pair_K) {                                /* pairs without a camera model of their own follow K */
        for (int p = 0; p < c->n_pairs; p++)
            if (!c->pair_K_own[p]) c->h_pair_K[p] = make_float4(fx, fy, cx, cy);
        HIPCHK(c, stream_wait(c->stream));
        HIPCHK(c, hipMemcpy(c->d_pair_K, c->h_pair_K.data(), sizeof(float4) * (size_t)c->n_pairs, hipMemcpyHostToDevice));
    }
    return DVO_OK;
}

}  // extern "C"

/* a pair's own camera model (own = true), or back to the context's K.  The pair's compact lists lose their short form when its model
 * changes, as every pair's do in dvo_set_intrinsics: a list is never expanded with a K other than the one it was built under */
int dvo_host::pair_intrinsics_set(dvo_ctx *c, int pair, bool own, float fx, float fy, float cx, float cy) {
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    if (own && (!(fx > 0.0f) || !(fy > 0.0f))) return fail(c, DVO_ERR_INVALID, "fx, fy must be positive");
    if (!own && !c->d_pair_K) return DVO_OK;           /* no table: every pair uses K already */
    const float4 old = c->d_pair_K ? c->h_pair_K[pair] : make_float4(c->K.fx, c->K.fy, c->K.cx, c->K.cy);
    HIPCHK(c, stream_wait(c->stream));
    if (!c->d_pair_K) {
        HIPCHK(c, c->d_pair_K.alloc(c->n_pairs));
        c->h_pair_K.assign(c->n_pairs, make_float4(c->K.fx, c->K.fy, c->K.cx, c->K.cy));
        c->pair_K_own.assign(c->n_pairs, 0);
        c->K.pair_K = c->d_pair_K;
    }
    const float4 now = own ? make_float4(fx, fy, cx, cy) : make_float4(c->K.fx, c->K.fy, c->K.cx, c->K.cy);
    c->h_pair_K[pair] = now;
    c->pair_K_own[pair] = own ? 1 : 0;
    c->host_changed();
    HIPCHK(c, hipMemcpy(c->d_pair_K, c->h_pair_K.data(), sizeof(float4) * (size_t)c->n_pairs, hipMemcpyHostToDevice));
    if (old.x != now.x || old.y != now.y || old.z != now.z || old.w != now.w)
        for (int l = 0; l < DVO_LEVELS; l++)
            if (!c->lv[l].compact_ok.empty()) c->lv[l].compact_ok.w(pair) = 0;
    return DVO_OK;
}

extern "C" {

/* ---- reference side -------------------------------------------------------- */
static int set_ref_common(dvo_ctx *c, int pair, int level, const float *xyz, int N, bool device_src) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    if (!xyz || N < 1) return fail(c, DVO_ERR_INVALID, "need N >= 1 reference points (reference asserts nSelectedPts > 0, SolveDVO.cpp:282)");
    int rc = ensure_points(c, level, N);
    if (rc) return rc;
    Level &L = c->lv[level];
    float *dst = L.pts + (size_t)pair * L.pt_cap * 3;
    HIPCHK(c, hipMemcpyAsync(dst, xyz, sizeof(float) * 3 * (size_t)N,
                             device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    L.hN.w(pair) = N;
    ref_list_written(c, level, pair, 1, 0);
    L.compact_ok.w(pair) = 0;                                         /* arbitrary X, Y: no 8-byte form ... */
    HIPCHK(c, hipMemsetAsync(L.d_pt4_ok + pair, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemcpyAsync(L.dN + pair, &L.hN[pair], sizeof(int), hipMemcpyHostToDevice, c->stream));
    /* ... unless the list IS what enlistRefEdgePts (:224-264) makes of some edge map for these intrinsics -- the literal drop-in hands over
     * exactly that (_ref_edge_3d[level]).  Round 6: every point's pixel is recovered and put through
     * the enlist expression again; all points equal bit for bit -> the list gets its compact twin (the packed kernel then reads the caller's
     * bits), any mismatch -> the one-point-per-lane kernel as before.  Costs one launch and one 4-byte read-back per call. */
    if (c->have_K && fused_uses_compact(c->prm.points_in_flight, c->prm.interpolate_dt)) {
        if (!c->h_poses) HIPCHK(c, c->h_poses.alloc(12 * (size_t)c->n_pairs + 2));
        int *h_fail = reinterpret_cast<int *>(c->h_poses + 12 * (size_t)c->n_pairs) + 1;      /* pinned: the slot beside the team error word */
        int *d_fail = L.d_pt4_ok + pair;                            /* a scratch word: zero now, rewritten by points4_build below or left zero */
        HIPCHK(c, launch_points_recover_compact(dst, N, level, intrinsics_of(c, pair), L.cpts + (size_t)pair * L.pt_cap, L.cidx + (size_t)pair * L.pt_cap, d_fail, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_fail, d_fail, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_wait(c->stream));
        const bool ok = *h_fail == 0;
        if (!ok) HIPCHK(c, hipMemsetAsync(d_fail, 0, sizeof(int), c->stream));
        if (ok) {
            L.compact_ok.w(pair) = 1;
            /* 4-byte points need the level's row count (their row field): known once the now level of this size has been installed */
            if (L.rows > 0) {
                HIPCHK(c, launch_points4_build(L.cpts, L.dN, L.pt_cap, L.rows, L.cpt4, L.chdr, L.d_pt4_ok, pair, 1, c->stream));
                L.pt4_rows.w(pair) = L.rows;
            }
        }
        return DVO_OK;
    }
    if (!device_src) HIPCHK(c, stream_wait(c->stream));   /* host buffer is only borrowed */
    return DVO_OK;
}
int dvo_set_ref_level_pair(dvo_ctx *c, int pair, int level, const float *xyz, int N) {
    return set_ref_common(c, pair, level, xyz, N, false);
}
int dvo_set_ref_level(dvo_ctx *c, int level, const float *xyz, int N) {
    return set_ref_common(c, 0, level, xyz, N, false);
}
int dvo_set_ref_level_device(dvo_ctx *c, int pair, int level, const float *d_xyz, int N) {
    return set_ref_common(c, pair, level, d_xyz, N, true);
}

int dvo_set_ref_level_from_images(dvo_ctx *c, int pair, int level, const int32_t *edge,
                                  const float *depth_mm, int rows, int cols,
                                  float *xyz_out, float *uv_out, int capacity, int *N_out) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    if (!edge || !depth_mm || rows < 1 || cols < 1) return fail(c, DVO_ERR_INVALID, "bad image arguments");
    if (!c->have_K) return fail(c, DVO_ERR_STATE, "intrinsics not set (dvo_set_intrinsics)");
    const size_t npx = (size_t)rows * cols;
    /* staging: edge (int32) | depth (f32) | uv (2 floats per pixel worst case) */
    int rc = ensure_staging(c, npx * (4 + 4 + 8));
    if (rc) return rc;
    int32_t *d_edge = (int32_t *)c->staging.get();
    float *d_depth = c->staging + npx;
    float *d_uv = c->staging + 2 * npx;
    const size_t cc_ints = (size_t)cols + 2 + enlist_block_ints(rows, cols);      /* column counters | block-order counters */
    if ((rc = regrow(c, c->d_colcounts, cc_ints))) return rc;
    int *d_blk = c->d_colcounts + cols + 2;
    HIPCHK(c, hipMemcpyAsync(d_edge, edge, npx * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_depth, depth_mm, npx * 4, hipMemcpyHostToDevice, c->stream));
    /* pass 1: count on the device, read N, grow the slab; pass 2: write */
    const ImgBatch gb{rows, cols, 1};
    int *d_N = c->d_colcounts + cols + 1;
    HIPCHK(c, launch_enlist_count(d_edge, 0, 0, d_depth, 0, gb, c->d_colcounts, d_blk, c->stream));
    int N = 0;
    HIPCHK(c, hipMemcpyAsync(&N, d_N, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    if (N_out) *N_out = N;
    if (N < 1) return fail(c, DVO_ERR_INVALID, "no reference point selected (reference asserts nSelectedPts > 0, SolveDVO.cpp:282)");
    if ((rc = ensure_points(c, level, N))) return rc;
    Level &L = c->lv[level];
    float *dst = L.pts + (size_t)pair * L.pt_cap * 3;
    HIPCHK(c, launch_enlist_write(d_edge, 0, 0, d_depth, 0, gb, level, intrinsics_of(c, pair), c->d_colcounts, d_blk, dst, 0,
                                  L.cpts + (size_t)pair * L.pt_cap, L.cidx + (size_t)pair * L.pt_cap, d_uv, N, nullptr, c->stream));
    L.hN.w(pair) = N;
    HIPCHK(c, hipMemcpyAsync(L.dN + pair, &L.hN[pair], sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_points4_build(L.cpts, L.dN, L.pt_cap, rows, L.cpt4, L.chdr, L.d_pt4_ok, pair, 1, c->stream));
    L.compact_ok.w(pair) = 1;
    L.hN.w(pair) = N;
    ref_list_written(c, level, pair, 1, rows);
    HIPCHK(c, hipMemcpyAsync(L.dN + pair, &L.hN[pair], sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int ncopy = std::min(N, capacity);
    if (xyz_out && ncopy > 0)
        HIPCHK(c, hipMemcpyAsync(xyz_out, dst, sizeof(float) * 3 * (size_t)ncopy, hipMemcpyDeviceToHost, c->stream));
    if (uv_out && ncopy > 0)
        HIPCHK(c, hipMemcpyAsync(uv_out, d_uv, sizeof(float) * 2 * (size_t)ncopy, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* ---- now side --------------------------------------------------------------- */
static int set_now_common(dvo_ctx *c, int pair, int level, const float *dt, const float *gx,
                          const float *gy, int rows, int cols, bool device_src) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    if (!dt || !gx || !gy || rows < 1 || cols < 1) return fail(c, DVO_ERR_INVALID, "bad image arguments");
    int rc = ensure_texels(c, level, rows, cols);
    if (rc) return rc;
    Level &L = c->lv[level];
    const size_t npx = (size_t)rows * cols;
    const float *s_dt = dt, *s_gx = gx, *s_gy = gy;
    /* the compact form straight from the float images (round 3, dvo_frames.hip: launch_float_level_to_compact): for a normalised
     * exact distance transform with its imageGradient -- what the reference produces -- the pair is read in the 4-byte form from
     * its first alignment on; anything else keeps the 16-byte texels (and the generic builder's DVO_COMPACT_NOW_AFTER policy) */
    const bool direct = direct_compact_wanted(c) && (long long)rows + cols + 1 <= 46340 && p4_addressable(rows, cols);
    const size_t plane_floats = device_src ? 0 : 3 * npx;
    if (!device_src || direct)
        if ((rc = ensure_staging(c, sizeof(float) * plane_floats + (direct ? sizeof(int) * float_level_work_ints(rows, cols) : 0)))) return rc;
    if (!device_src) {
        HIPCHK(c, hipMemcpyAsync(c->staging, dt, npx * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->staging + npx, gx, npx * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->staging + 2 * npx, gy, npx * 4, hipMemcpyHostToDevice, c->stream));
        s_dt = c->staging; s_gx = c->staging + npx; s_gy = c->staging + 2 * npx;
    }
    if ((rc = map_texels(c, level, pair, 1))) return rc;
    HIPCHK(c, launch_pack_texels(s_dt, s_gx, s_gy, L.tex + (size_t)pair * L.tex_stride, rows, cols, c->stream));
    if ((rc = now_written(c, level, pair, 1))) return rc;
    if (direct) {
        if ((rc = ensure_compact_slabs(c, level))) return rc;
        HIPCHK(c, launch_float_level_to_compact(s_dt, s_gx, s_gy, rows, cols, reinterpret_cast<int *>(c->staging + plane_floats), L.p4,
                                                L.p4_stride, L.pal, L.d_pal_n, pair, c->stream));
        L.now.w(pair).direct_compact_written();        /* texels AND compact form are current; pal_n on the device says which one the kernel reads */
        if (!device_src) {
            if (!c->h_poses) HIPCHK(c, c->h_poses.alloc(12 * (size_t)c->n_pairs + 2));
            HIPCHK(c, hipMemcpyAsync(c->h_poses, L.d_pal_n + pair, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (!device_src) {
        HIPCHK(c, stream_wait(c->stream));
        /* not an exact distance transform (or its gradients are not imageGradient's): leave the pair to the generic builder's policy */
        if (direct && *reinterpret_cast<const int *>(c->h_poses.get()) <= 0) L.now.w(pair).direct_compact_refused();
    }
    return DVO_OK;
}
void *dvo_host_alloc_mapped(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void dvo_host_free_mapped(void *p) { if (p) (void)hipHostFree(p); }

int dvo_set_direct_compact(dvo_ctx *c, int on) {
    DVO_ENTER(c);
    c->direct_compact = on ? 1 : 0;
    c->host_changed();
    return DVO_OK;
}
int dvo_set_now_level_pair(dvo_ctx *c, int pair, int level, const float *dt, const float *gx,
                           const float *gy, int rows, int cols) {
    return set_now_common(c, pair, level, dt, gx, gy, rows, cols, false);
}
int dvo_set_now_level(dvo_ctx *c, int level, const float *dt, const float *gx, const float *gy,
                      int rows, int cols) {
    return set_now_common(c, 0, level, dt, gx, gy, rows, cols, false);
}
int dvo_set_now_level_device(dvo_ctx *c, int pair, int level, const float *d_dt, const float *d_gx,
                             const float *d_gy, int rows, int cols) {
    return set_now_common(c, pair, level, d_dt, d_gx, d_gy, rows, cols, true);
}

/* computeDistTransfrmOfNow after Canny (SolveDVO.cpp:1768-1795) on the device */
int dvo_set_now_level_from_edges(dvo_ctx *c, int pair, int level, const unsigned char *edge, int rows, int cols) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    if (!edge || rows < 1 || cols < 1) return fail(c, DVO_ERR_INVALID, "bad image arguments");
    if ((long long)rows + cols + 1 > 46340) return fail(c, DVO_ERR_INVALID, "image too large for the exact distance transform (rows + cols must stay below 46339)");
    int rc = ensure_texels(c, level, rows, cols);
    if (rc) return rc;
    const size_t npx = (size_t)rows * cols;
    bool any = false;
    for (size_t i = 0; i < npx && !any; i++) any = edge[i] != 0;
    if (!any) return fail(c, DVO_ERR_INVALID, "edge mask has no edge pixel: the distance transform is undefined");
    /* staging: edge bytes (rounded up to ints) | work ints */
    const size_t edge_ints = (npx + 3) / 4;
    if ((rc = ensure_staging(c, sizeof(int) * (edge_ints + edt_work_ints(rows, cols, 1) + 1)))) return rc;
    unsigned char *d_edge = (unsigned char *)c->staging.get();
    int *work = (int *)c->staging.get() + edge_ints;
    HIPCHK(c, hipMemcpyAsync(d_edge, edge, npx, hipMemcpyHostToDevice, c->stream));
    Level &L = c->lv[level];
    const bool compact = native_compact_wanted(c);
    if (compact && (rc = ensure_compact_slabs(c, level))) return rc;
    /* a sparse texel slab: the stage runs without texel output first; the (rare) image the compact form cannot hold gets its
     * texels mapped and written by a second run of the last pass */
    const bool defer = compact && L.tex_sparse;
    if (L.tex_sparse && !compact && (rc = map_texels(c, level, pair, 1))) return rc;
    HIPCHK(c, launch_edges_to_now(d_edge, 0, ImgBatch{rows, cols, 1}, work, defer ? nullptr : L.tex + (size_t)pair * L.tex_stride, L.tex_stride,
                                  compact ? L.p4 : nullptr, L.p4_stride, L.pal, L.d_pal_n, pair, c->stream));
    if (defer) {
        int n_failed = 0;
        if ((rc = sparse_map_compact_failures(c, level, pair, 1, c->stream, &n_failed))) return rc;
        if (n_failed)
            HIPCHK(c, launch_edges_to_now(d_edge, 0, ImgBatch{rows, cols, 1}, work, L.tex + (size_t)pair * L.tex_stride, L.tex_stride,
                                          L.p4, L.p4_stride, L.pal, L.d_pal_n, pair, c->stream, true));
    }
    if ((rc = compact ? now_written_compact(c, level, pair, 1) : now_written(c, level, pair, 1))) return rc;
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* the three planar images of a resident now level (inspection) */
int dvo_get_now_level(dvo_ctx *c, int pair, int level, float *dt, float *gx, float *gy) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    Level &L = c->lv[level];
    if (!L.now[pair].ready()) return fail(c, DVO_ERR_STATE, "now level not set");
    const size_t npx = (size_t)L.rows * L.cols;
    int rc = ensure_staging(c, sizeof(float) * 3 * npx);
    if (rc) return rc;
    if ((rc = ensure_tex16(c, level, pair, 1))) return rc;
    float *d = c->staging;
    HIPCHK(c, launch_unpack_texels(L.tex + (size_t)pair * L.tex_stride, L.rows, L.cols, d, d + npx, d + 2 * npx, c->stream));
    if (dt) HIPCHK(c, hipMemcpyAsync(dt, d, sizeof(float) * npx, hipMemcpyDeviceToHost, c->stream));
    if (gx) HIPCHK(c, hipMemcpyAsync(gx, d + npx, sizeof(float) * npx, hipMemcpyDeviceToHost, c->stream));
    if (gy) HIPCHK(c, hipMemcpyAsync(gy, d + 2 * npx, sizeof(float) * npx, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

int dvo_get_ref_level(dvo_ctx *c, int pair, int level, float *xyz_out, int capacity, int *N_out) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    Level &L = c->lv[level];
    if (L.hN.empty() || L.hN[pair] <= 0) return fail(c, DVO_ERR_STATE, "reference level not set");
    const int N = L.hN[pair];
    if (N_out) *N_out = N;
    const int ncopy = std::min(N, capacity);
    if (xyz_out && ncopy > 0) {
        HIPCHK(c, hipMemcpyAsync(xyz_out, L.pts + (size_t)pair * L.pt_cap * 3, sizeof(float) * 3 * (size_t)ncopy,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_wait(c->stream));
    }
    return DVO_OK;
}

/* replicate the first n_src pairs over [dst_first, dst_first+dst_count): slot p <- pair (p-dst_first) % n_src */
int dvo_replicate_pairs(dvo_ctx *c, int n_src, int dst_first, int dst_count) {
    DVO_ENTER(c);
    if (n_src < 1 || dst_first < 0 || dst_count < 0 || dst_first + dst_count > c->n_pairs || n_src > c->n_pairs)
        return fail(c, DVO_ERR_INVALID, "bad replicate arguments");
    if (dst_first != 0 && dst_first < n_src) return fail(c, DVO_ERR_INVALID, "destination range overlaps the sources");
    for (int l = 0; l < DVO_LEVELS; l++) {
        Level &L = c->lv[l];
        if (!L.tex && !L.pts) continue;
        for (int p = 0; p < n_src; p++) {
            int rc = check_ready(c, p, l);
            if (rc) return rc;
        }
        /* the now level travels in the form(s) its sources have: 16-byte texels, the compact form, or both.  A source whose image
         * the compact form could not hold HAS 16-byte texels (refresh_compact_known clears its stale mark) */
        { const int prc = refresh_compact_known(c, l, 0, n_src); if (prc) return prc; }
        bool any_tex16 = false, any_compact = false;
        for (int p = 0; p < n_src; p++) {
            any_tex16 = any_tex16 || L.now[p].texels_real();
            any_compact = any_compact || L.now[p].built;
        }
        DevBuf<unsigned char> d_has_tex;
        if (any_tex16 && L.tex) {
            /* 16-byte texels travel with the sources that have them: those destinations (and sources) need memory behind theirs */
            std::vector<unsigned char> has((size_t)n_src);
            bool all = true;
            for (int p = 0; p < n_src; p++) { has[p] = L.now[p].texels_real(); all = all && has[p]; }
            for (int p = 0; p < n_src; p++)
                if (has[p]) { const int mrc = map_texels(c, l, p, 1); if (mrc) return mrc; }
            for (int p = dst_first; p < dst_first + dst_count; ) {
                if (!has[(p - dst_first) % n_src]) { p++; continue; }
                int q = p;
                while (q < dst_first + dst_count && has[(q - dst_first) % n_src]) q++;
                const int mrc = map_texels(c, l, p, q - p);
                if (mrc) return mrc;
                p = q;
            }
            if (!all) {
                HIPCHK(c, d_has_tex.alloc((size_t)n_src));
                HIPCHK(c, hipMemcpyAsync(d_has_tex, has.data(), (size_t)n_src, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, stream_wait(c->stream));          /* `has` leaves scope */
            }
        }
        {
            const hipError_t le = launch_replicate_level(any_tex16 ? L.tex : nullptr, d_has_tex, L.tex_stride, L.pts, L.cpts, L.cidx, L.cpt4, L.chdr, L.d_pt4_ok,
                                                         L.pt_cap, L.dN, n_src, dst_first, dst_count, c->stream);
            if (d_has_tex) { (void)hipStreamSynchronize(c->stream); d_has_tex.reset(); }
            HIPCHK(c, le);
        }
        for (int p = dst_first; p < dst_first + dst_count; p++) {
            const int src = (p - dst_first) % n_src;
            if (src == p) continue;                                 /* a source inside the destination range keeps its own list */
            L.hN.w(p) = L.hN[src];
            ref_list_written(c, l, p, 1, L.pt4_rows.empty() ? 0 : L.pt4_rows[src]);
            L.compact_ok.w(p) = L.compact_ok[src];
        }
        /* the slots written: everything but the sources themselves (dst_first == 0: the range starts with them) */
        const int w_first = (dst_first == 0) ? std::min(n_src, dst_count) : dst_first;
        const int w_count = dst_first + dst_count - w_first;
        if (L.tex && w_count > 0) {
            int rc = now_written(c, l, w_first, w_count);           /* marks the destinations' compact form stale ... */
            if (rc) return rc;
            if (any_compact) {                                      /* ... and this copies the sources' over it */
                HIPCHK(c, launch_replicate_compact(L.p4, L.p4_stride, L.pal, L.d_pal_n, n_src, dst_first, dst_count, c->stream));
                for (int p = dst_first; p < dst_first + dst_count; p++) {
                    const int src = (p - dst_first) % n_src;
                    if (p != src) L.now.w(p).adopt(L.now[src]);
                }
            }
        }
    }
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* shape of the last fused launch: threads per workgroup, workgroups per pair (team), 1 = packed two-points-per-lane kernel */
int dvo_get_last_launch_shape(dvo_ctx *c, int *block_threads, int *team_size, int *packed) {
    DVO_ENTER(c);
    if (block_threads) *block_threads = c->last_block;
    if (team_size) *team_size = c->last_team;
    if (packed) *packed = c->last_packed;
    return DVO_OK;
}

/* build the compact form of the resident now levels of these pairs now (instead of at their second alignment) */
int dvo_now_prepare(dvo_ctx *c, int first_pair, int count) {
    DVO_ENTER(c);
    if (!pair_ok(c, first_pair) || count < 1 || first_pair + count > c->n_pairs) return fail(c, DVO_ERR_INVALID, "pair range out of bounds");
    c->host_changed();           /* whatever it finds to build: the next enqueue() decides anew */
    if (c->prm.engine_variant == 4 || compact_now_policy() == 2) return DVO_OK;
    for (int l = 0; l < DVO_LEVELS; l++) {
        int rc = build_compact_now(c, l, first_pair, count, false);
        if (rc) return rc;
    }
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* palette size of the compact form of (pair, level): > 0 size, 0 not built, < 0 the builder's reason for "no compact form" */
int dvo_get_now_compact_info(dvo_ctx *c, int pair, int level, int *palette_size) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !palette_size) return fail(c, DVO_ERR_INVALID, "bad arguments");
    Level &L = c->lv[level];
    *palette_size = 0;
    if (!L.d_pal_n) return DVO_OK;
    HIPCHK(c, hipMemcpyAsync(palette_size, L.d_pal_n + pair, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    if (*palette_size > 0) *palette_size = pal_count(*palette_size);      /* without the partial mark: dvo_get_now_compact_partial */
    return DVO_OK;
}
/* 1 if the compact form of (pair, level) is PARTIAL (round 5, dvo_palette.h): the image has more distinct distances than the palette
 * holds, a pixel 512 px or more from every edge or a rank step beyond +-127 -- its lowest ranks are in the compact form, the pixels
 * it cannot express are looked up in the image's 16-byte texels (which such an image also has) */
int dvo_get_now_compact_partial(dvo_ctx *c, int pair, int level, int *partial) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !partial) return fail(c, DVO_ERR_INVALID, "bad arguments");
    Level &L = c->lv[level];
    *partial = 0;
    if (!L.d_pal_n) return DVO_OK;
    int v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, L.d_pal_n + pair, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    *partial = pal_partial(v) ? 1 : 0;
    return DVO_OK;
}

/* ---- hot path ---------------------------------------------------------------- */
/* wait = false (dvo_align_batch): the launch that reads the poses follows on the same stream, and every host-side writer of the staging
 * buffer waits for the stream first -- no host round trip for the upload */
static int set_poses_impl(dvo_ctx *c, int first_pair, int n_pairs, const double *R, const double *t, bool wait) {
    if (!pair_ok(c, first_pair) || n_pairs < 1 || first_pair + n_pairs > c->n_pairs || !R || !t)
        return fail(c, DVO_ERR_INVALID, "bad pose arguments");
    if (!c->h_poses) HIPCHK(c, c->h_poses.alloc(12 * (size_t)c->n_pairs + 2));
    double *h = c->h_poses;                       /* pinned: a plain DMA, no staging thread, no blocking wait inside the copy */
    HIPCHK(c, stream_wait(c->stream));            /* an earlier dvo_get_poses may still be filling the staging buffer */
    for (int p = 0; p < n_pairs; p++) {
        std::memcpy(&h[12 * p], R + 9 * p, sizeof(double) * 9);
        std::memcpy(&h[12 * p + 9], t + 3 * p, sizeof(double) * 3);
    }
    HIPCHK(c, hipMemcpyAsync(c->d_poses + (size_t)12 * first_pair, h, sizeof(double) * 12 * (size_t)n_pairs,
                             hipMemcpyHostToDevice, c->stream));
    if (wait) HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}
int dvo_set_poses(dvo_ctx *c, int first_pair, int n_pairs, const double *R, const double *t) {
    DVO_ENTER(c);
    return set_poses_impl(c, first_pair, n_pairs, R, t, true);
}

/* team mode: a member that gave up waiting for its team leaves a flag; every result of that launch is void */
static int check_team_err(dvo_ctx *c) {
    if (!c->team_used) return DVO_OK;
    if (!c->h_poses) HIPCHK(c, c->h_poses.alloc(12 * (size_t)c->n_pairs + 2));
    int *flag = reinterpret_cast<int *>(c->h_poses + 12 * (size_t)c->n_pairs);      /* pinned slot after the poses */
    *flag = 0;
    HIPCHK(c, hipMemcpyAsync(flag, c->d_team_cnt + c->n_pairs, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    const int team_err = *flag;
    if (team_err) c->team_err_dirty = true;
    if (team_err)
        return fail(c, DVO_ERR_HIP, "team mode: a workgroup gave up waiting for its team (members were not resident together); "
                                    "the results of that launch are void -- set dvo_params.team_size = 1");
    return DVO_OK;
}

}  // extern "C"
/* dvo_get_poses / dvo_get_poses_rows: the staging copy, the wait and the team error check; then 12 doubles per pair (R column-major,
 * t) are unpacked, with R as it is stored or row by row */
template <bool kRows>
static int get_poses_impl(dvo_ctx *c, int first_pair, int n_pairs, double *R, double *t) {
    if (!pair_ok(c, first_pair) || n_pairs < 1 || first_pair + n_pairs > c->n_pairs || !R || !t)
        return fail(c, DVO_ERR_INVALID, "bad pose arguments");
    if (!c->h_poses) HIPCHK(c, c->h_poses.alloc(12 * (size_t)c->n_pairs + 2));
    double *h = c->h_poses;
    int *flag = reinterpret_cast<int *>(c->h_poses + 12 * (size_t)c->n_pairs);      /* team mode: the error word rides on the same wait */
    *flag = 0;
    if (c->team_used) HIPCHK(c, hipMemcpyAsync(flag, c->d_team_cnt + c->n_pairs, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h, c->d_poses + (size_t)12 * first_pair, sizeof(double) * 12 * (size_t)n_pairs,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    if (c->team_used && *flag) c->team_err_dirty = true;
    if (c->team_used && *flag)
        return fail(c, DVO_ERR_HIP, "team mode: a workgroup gave up waiting for its team (members were not resident together); "
                                    "the results of that launch are void -- set dvo_params.team_size = 1");
    for (int p = 0; p < n_pairs; p++) {
        const double *s = &h[12 * (size_t)p];
        double *r = R + 9 * (size_t)p;
        if (kRows) {
            r[0] = s[0]; r[1] = s[3]; r[2] = s[6];
            r[3] = s[1]; r[4] = s[4]; r[5] = s[7];
            r[6] = s[2]; r[7] = s[5]; r[8] = s[8];
        } else
            std::memcpy(r, s, sizeof(double) * 9);
        std::memcpy(t + 3 * (size_t)p, s + 9, sizeof(double) * 3);
    }
    return DVO_OK;
}
extern "C" {

int dvo_get_poses(dvo_ctx *c, int first_pair, int n_pairs, double *R, double *t) {
    DVO_ENTER(c);
    return get_poses_impl<false>(c, first_pair, n_pairs, R, t);
}

int dvo_get_poses_rows(dvo_ctx *c, int first_pair, int n_pairs, double *R_rows, double *t) {
    DVO_ENTER(c);
    return get_poses_impl<true>(c, first_pair, n_pairs, R_rows, t);
}

int dvo_get_enqueue_counts(dvo_ctx *c, unsigned long long *full_passes, unsigned long long *memo_hits) {
    DVO_ENTER(c);
    if (!full_passes || !memo_hits) return fail(c, DVO_ERR_INVALID, "NULL output");
    *full_passes = c->memo.full_passes;
    *memo_hits = c->memo.hits;
    return DVO_OK;
}

}  // extern "C"
namespace dvo_host {
int enqueue_pair_list(dvo_ctx *c, const int *h_pairs, const int *d_pairs, int n, int n_levels, const int *iters, int flags) {
    EnqueueRequest q = range_request(0, n, n_levels, iters, flags);
    q.h_list = h_pairs; q.d_list = d_pairs;
    return enqueue(c, q);
}
}  // namespace dvo_host
extern "C" {
int dvo_align_batch_enqueue(dvo_ctx *c, int first_pair, int n_pairs, int n_levels, const int *iters, int flags) {
    DVO_ENTER(c);
    return enqueue(c, range_request(first_pair, n_pairs, n_levels, iters, flags));
}

int dvo_align_batch(dvo_ctx *c, int first_pair, int n_pairs, int n_levels, const int *iters,
                    int flags, double *R, double *t) {
    DVO_ENTER(c);
    if (!pair_ok(c, first_pair) || n_pairs < 1 || first_pair + n_pairs > c->n_pairs || !R || !t)
        return fail(c, DVO_ERR_INVALID, "bad pose arguments");
    int rc = set_poses_impl(c, first_pair, n_pairs, R, t, false);
    if (rc) return rc;
    if ((rc = enqueue(c, range_request(first_pair, n_pairs, n_levels, iters, flags & ~DVO_FLAG_IDENTITY_START)))) return rc;
    return dvo_get_poses(c, first_pair, n_pairs, R, t);
}

int dvo_align_pyramid(dvo_ctx *c, int n_levels, const int *iters, int flags, double *R, double *t) {
    return dvo_align_batch(c, 0, 1, n_levels, iters, flags, R, t);
}

int dvo_get_level_report(dvo_ctx *c, int pair, int level, float *energy, int n_energy,
                         int *best_idx, float *visible_ratio) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range");
    if (!c->have_sched || level >= c->sched.n_levels) return fail(c, DVO_ERR_STATE, "no alignment has been run for this level");
    if (!outputs_valid(c, pair))
        return fail(c, DVO_ERR_STATE, "pair " + std::to_string(pair) + " was not aligned under the current schedule (its report was "
                                      "overwritten or laid out by an earlier, different schedule): align it again");
    HIPCHK(c, stream_wait(c->stream));
    { const int trc = check_team_err(c); if (trc) return trc; }
    if (energy) {
        const int n = std::min(n_energy, c->sched.iters[level]);
        if (n > 0)
            HIPCHK(c, hipMemcpy(energy, c->d_energy + (size_t)pair * c->sched.e_stride + c->sched.e_off[level],
                                sizeof(float) * n, hipMemcpyDeviceToHost));
    }
    if (best_idx) HIPCHK(c, hipMemcpy(best_idx, c->d_best + pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    if (visible_ratio) HIPCHK(c, hipMemcpy(visible_ratio, c->d_ratio + pair * DVO_LEVELS + level, sizeof(float), hipMemcpyDeviceToHost));
    return DVO_OK;
}

/* H = sum_i w_i J_i^T J_i of iterate `itr` of `level` (itr < 0: the best iterate), as the 6x6 symmetric matrix, row-major */
int dvo_get_level_normal_matrix(dvo_ctx *c, int pair, int level, int itr, double *H36) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !H36) return fail(c, DVO_ERR_INVALID, "bad arguments");
    if (!c->have_sched || level >= c->sched.n_levels || !(c->sched.flags & DVO_FLAG_NORMAL_MATRIX) || !c->d_H)
        return fail(c, DVO_ERR_STATE, "last alignment did not request DVO_FLAG_NORMAL_MATRIX");
    if (!outputs_valid(c, pair)) return fail(c, DVO_ERR_STATE, "pair was not aligned under the current schedule: align it again");
    HIPCHK(c, stream_wait(c->stream));
    if (itr < 0) HIPCHK(c, hipMemcpy(&itr, c->d_best + pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    if (itr < 0 || itr >= c->sched.iters[level]) return fail(c, DVO_ERR_STATE, "no such iterate");
    double h[21];
    HIPCHK(c, hipMemcpy(h, c->d_H + ((size_t)pair * c->sched.e_stride + c->sched.e_off[level] + itr) * 21, sizeof(h), hipMemcpyDeviceToHost));
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { H36[i * 6 + j] = h[k]; H36[j * 6 + i] = h[k]; k++; }
    return DVO_OK;
}

int dvo_get_final_outputs(dvo_ctx *c, int pair, float *final_eps, float *final_reproj, int capacity, int *N_out) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    if (!c->have_sched || !(c->sched.flags & DVO_FLAG_FINAL_OUTPUTS) || !c->d_final_eps)
        return fail(c, DVO_ERR_STATE, "last alignment did not request DVO_FLAG_FINAL_OUTPUTS");
    if (!outputs_valid(c, pair))
        return fail(c, DVO_ERR_STATE, "pair " + std::to_string(pair) + " was not aligned under the current schedule: align it again");
    HIPCHK(c, stream_wait(c->stream));
    { const int trc = check_team_err(c); if (trc) return trc; }
    int N = 0;
    HIPCHK(c, hipMemcpy(&N, c->d_final_N + pair, sizeof(int), hipMemcpyDeviceToHost));
    if (N_out) *N_out = N;
    const int n = std::min(N, capacity);
    const float *src_e = c->d_final_eps + (size_t)pair * c->final_cap, *src_r = c->d_final_reproj + (size_t)pair * c->final_cap * 3;
    if (N > 0 && c->sched.final_blk) {
        /* the packed kernel keeps them in the order of its compact point list; the reference's order (:703-704) is made here */
        const Level &L = c->lv[c->sched.last_level];
        const int dpair = (c->sched.alias_mod > 0) ? pair % c->sched.alias_mod : pair;
        /* ... with the index of THAT list: if the pair's reference list was rewritten after the alignment (a key-frame switch, a
         * replicate, a new dvo_set_ref_level*) the index now describes other points and the outputs cannot be put in order any more */
        const unsigned long long now_gen = L.list_gen.empty() ? 0 : L.list_gen[dpair];
        if (c->final_list_gen.empty() || c->final_list_gen[pair] != now_gen || N != L.hN[dpair])
            return fail(c, DVO_ERR_STATE, "the reference list of pair " + std::to_string(pair) + " was replaced after its alignment: the final "
                                          "outputs of that alignment are gone (fetch them before installing a new reference, or align again)");
        int rc = ensure_staging(c, sizeof(float) * 4 * (size_t)N);
        if (rc) return rc;
        HIPCHK(c, launch_final_permute(L.cidx + (size_t)dpair * L.pt_cap, src_e, src_r, N, c->staging, c->staging + N, c->stream));
        HIPCHK(c, stream_wait(c->stream));
        src_e = c->staging; src_r = c->staging + N;
    }
    if (n > 0 && final_eps) HIPCHK(c, hipMemcpy(final_eps, src_e, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (n > 0 && final_reproj) HIPCHK(c, hipMemcpy(final_reproj, src_r, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_run_iterations_pair(dvo_ctx *c, int pair, int level, int max_iters, double *R, double *t,
                            float *energy, float *final_eps, float *final_reproj,
                            int *best_idx, float *visible_ratio) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level)) return fail(c, DVO_ERR_INVALID, "pair/level out of range (reference: assert level>=0, SolveDVO.cpp:625)");
    if (max_iters < 1) return fail(c, DVO_ERR_INVALID, "maxIterations must be > 0 (SolveDVO.cpp:626)");
    if (!R || !t) return fail(c, DVO_ERR_INVALID, "R/t are NULL");
    int iters[DVO_LEVELS] = {0};
    iters[level] = max_iters;
    const int flags = (final_eps || final_reproj) ? DVO_FLAG_FINAL_OUTPUTS : 0;
    int rc = dvo_align_batch(c, pair, 1, level + 1, iters, flags, R, t);
    if (rc) return rc;
    if ((rc = dvo_get_level_report(c, pair, level, energy, max_iters, best_idx, visible_ratio))) return rc;
    if (flags) {
        const int N = c->lv[level].hN[pair];
        if ((rc = dvo_get_final_outputs(c, pair, final_eps, final_reproj, N, nullptr))) return rc;
    }
    return DVO_OK;
}

int dvo_run_iterations(dvo_ctx *c, int level, int max_iters, double *R, double *t,
                       float *energy, float *final_eps, float *final_reproj,
                       int *best_idx, float *visible_ratio) {
    return dvo_run_iterations_pair(c, 0, level, max_iters, R, t, energy, final_eps, final_reproj,
                                   best_idx, visible_ratio);
}

/* ---- host-driven iteration ------------------------------------------------------ */
int dvo_iter_begin(dvo_ctx *c, int pair, int level, int max_iters, const double *R, const double *t) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || max_iters < 1 || !R || !t) return fail(c, DVO_ERR_INVALID, "bad arguments");
    int rc = check_ready(c, pair, level);
    if (rc) return rc;
    if ((rc = ensure_tex16(c, level, pair, 1))) return rc;       /* the host-driven kernels read 16-byte texels */
    if (!c->d_states) {
        HIPCHK(c, c->d_states.alloc(pose_state_bytes() * c->n_pairs));
        c->iter_max.assign(c->n_pairs, 0);
    }
    if (max_iters > c->iter_energy_cap) {
        const int cap = std::max(max_iters, 64);
        c->iter_energy_cap = 0;
        if ((rc = regrow(c, c->d_iter_energy, (size_t)cap * c->n_pairs))) return rc;
        c->iter_energy_cap = cap;
    }
    double h[12];
    std::memcpy(h, R, sizeof(double) * 9);
    std::memcpy(h + 9, t, sizeof(double) * 3);
    double *d_pose = c->d_poses + (size_t)12 * pair;
    HIPCHK(c, hipMemcpyAsync(d_pose, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_iter_begin(c->d_states + pose_state_bytes() * pair, c->dprm, d_pose,
                                c->d_iter_energy + (size_t)c->iter_energy_cap * pair, max_iters, c->stream));
    HIPCHK(c, stream_wait(c->stream));     /* h is a stack buffer */
    c->iter_max[pair] = max_iters;
    return DVO_OK;
}

int dvo_iter_accumulate(dvo_ctx *c, int pair, int level, int first_point, int n_points, double *d_acc32) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !d_acc32) return fail(c, DVO_ERR_INVALID, "bad arguments");
    if (!c->d_states || c->iter_max[pair] == 0) return fail(c, DVO_ERR_STATE, "dvo_iter_begin has not been called for this pair");
    const int N = c->lv[level].hN.empty() ? 0 : c->lv[level].hN[pair];
    if (first_point < 0 || n_points < 0 || first_point + n_points > N) return fail(c, DVO_ERR_INVALID, "point range out of bounds");
    const int nb = accumulate_blocks_for(n_points);
    HIPCHK(c, launch_iter_accumulate(slab_of(c, level), pair, level, intrinsics_of(c, pair), c->d_states + pose_state_bytes() * pair,
                                     first_point, n_points, c->d_scratch, nb, d_acc32, c->stream));
    return DVO_OK;
}

int dvo_iter_update(dvo_ctx *c, int pair, int level, int itr, int n_total, const double *d_acc32) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !d_acc32 || n_total < 1) return fail(c, DVO_ERR_INVALID, "bad arguments");
    if (!c->d_states || c->iter_max[pair] == 0) return fail(c, DVO_ERR_STATE, "dvo_iter_begin has not been called for this pair");
    if (itr < 0 || itr >= c->iter_max[pair]) return fail(c, DVO_ERR_INVALID, "iteration index out of range");
    HIPCHK(c, launch_iter_update(c->d_states + pose_state_bytes() * pair, c->dprm, itr, n_total, d_acc32,
                                 c->d_iter_energy + (size_t)c->iter_energy_cap * pair, c->stream));
    return DVO_OK;
}

int dvo_iter_end(dvo_ctx *c, int pair, int level, double *R, double *t, float *energy, int *best_idx,
                 float *visible_ratio) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !R || !t) return fail(c, DVO_ERR_INVALID, "bad arguments");
    if (!c->d_states || c->iter_max[pair] == 0) return fail(c, DVO_ERR_STATE, "dvo_iter_begin has not been called for this pair");
    double *d_pose = c->d_poses + (size_t)12 * pair;
    HIPCHK(c, launch_iter_end(c->d_states + pose_state_bytes() * pair, d_pose, c->d_best + pair * DVO_LEVELS + level,
                              c->d_ratio + pair * DVO_LEVELS + level, c->stream));
    double h[12];
    HIPCHK(c, hipMemcpyAsync(h, d_pose, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    if (energy)
        HIPCHK(c, hipMemcpyAsync(energy, c->d_iter_energy + (size_t)c->iter_energy_cap * pair,
                                 sizeof(float) * c->iter_max[pair], hipMemcpyDeviceToHost, c->stream));
    if (best_idx) HIPCHK(c, hipMemcpyAsync(best_idx, c->d_best + pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (visible_ratio) HIPCHK(c, hipMemcpyAsync(visible_ratio, c->d_ratio + pair * DVO_LEVELS + level, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    std::memcpy(R, h, sizeof(double) * 9);
    std::memcpy(t, h + 9, sizeof(double) * 3);
    c->iter_max[pair] = 0;
    return DVO_OK;
}

/* The level schedule (SolveDVO.cpp:2097-2104) with every iteration spread over all CUs: the single-GPU
 * form of the host-driven loop, enqueued back to back from C (no collective, one synchronisation). */
}  /* extern "C" */

namespace dvo_host {

int ensure_step_buffers(dvo_ctx *c) {
    if (c->d_step_ticket) return DVO_OK;
    /* all or nothing; the ticket, the test above, goes last */
    if (c->d_step_state.alloc(2 * pose_state_bytes()) != hipSuccess || c->d_step_acc.alloc(2 * DVO_NACC_PAD) != hipSuccess ||
        c->d_step_ticket.alloc(4) != hipSuccess) {      /* [0] arrival ticket (launches with H), [1] launch sequence number, [2] a launch lost a workgroup's rows */
        (void)hipGetLastError();
        c->d_step_state.reset(); c->d_step_acc.reset();
        return fail(c, DVO_ERR_NOMEM, "cannot allocate the buffers of the tiled / wide schedule");
    }
    HIPCHK(c, hipMemsetAsync(c->d_step_acc, 0, sizeof(double) * 2 * DVO_NACC_PAD, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_step_ticket, 0, 4 * sizeof(unsigned), c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* a step launch whose workgroup 0 never saw the tagged rows of another workgroup leaves NaN sums and this word (dvo_tiled_step.h) */
int check_step_lost(dvo_ctx *c) {
    unsigned lost = 0;
    std::memcpy(&lost, c->h_pose + 12, sizeof(lost));
    if (!lost) return DVO_OK;
    (void)hipMemsetAsync(c->d_step_ticket + 2, 0, sizeof(unsigned), c->stream);
    return fail(c, DVO_ERR_HIP, "wide / tiled schedule: a step launch never received the sums of one of its workgroups; the results of that alignment are void");
}

static void shard_of(int n, int rank, int world, int &first, int &count) {      /* distributed.py::shard_range, dvo_tiled_shard */
    const int base = n / world, rem = n % world;
    count = base + (rank < rem ? 1 : 0);
    first = rank * base + (rank < rem ? rank : rem);
}

int team_err_check(dvo_ctx *c) { return check_team_err(c); }
/* the same without a host round trip of its own: the error word travels into a pinned slot in front of a wait the caller makes anyway */
hipError_t team_err_fetch(dvo_ctx *c, int *pinned_slot) {
    *pinned_slot = 0;
    if (!c->team_used || !c->d_team_cnt) return hipSuccess;
    return hipMemcpyAsync(pinned_slot, c->d_team_cnt + c->n_pairs, sizeof(int), hipMemcpyDeviceToHost, c->stream);
}
int team_err_result(dvo_ctx *c, const int *pinned_slot) {
    if (!*pinned_slot) return DVO_OK;
    c->team_err_dirty = true;
    return fail(c, DVO_ERR_HIP, "team mode: a workgroup gave up waiting for its team (members were not resident together); "
                                "the results of that launch are void -- set dvo_params.team_size = 1");
}

/* Round 6: the coarse levels of a large frame do not need 256 CUs -- a step launch costs ~7 us whatever it
 * holds (boundary + 255 -> 1 fan-in + the update at its head), an iteration of the fused kernel's team inside one XCD ~3-5 us.
 * The levels from the coarsest down to the first one beyond DVO_WIDE_TEAM_MAX points go to ONE launch of align_fused2_kernel in
 * team mode (dvo_enqueue's own machinery: same energies, best index, ratio bit for bit; the pose travels through d_poses), the
 * finer ones keep the step launches: on return `sc` holds those (same energy layout), coarse_mask the levels handed over (0: none --
 * then nothing was enqueued and the caller's sequence copies the pose in itself).  Over several ranks every rank runs the coarse levels
 * whole, like the one-launch small levels: no collective, identical bits.  Not with H (its per-iterate sums come from the step
 * launches), not without compact lists. */
int wide_coarse_levels_as_team(dvo_ctx *c, int pair, int n_levels, const int *iters, int flags, Schedule &sc, const double *h_pose_in,
                               double *d_pose, unsigned &coarse_mask, bool &coarse_team, bool allow_finest) {
    coarse_mask = 0;
    coarse_team = false;
    /* which levels go to which launch: dvo_launch_plan.h (allow_finest: one rank, nothing is sharded -- then sc may come back empty) */
    const TeamTiers &tiers = team_tiers();
    int N[DVO_LEVELS];
    bool compact_ok[DVO_LEVELS];
    for (int l = 0; l < n_levels; l++) {
        N[l] = sc.iters[l] > 0 ? c->lv[l].hN[pair] : 0;
        compact_ok[l] = !c->lv[l].compact_ok.empty() && c->lv[l].compact_ok[pair];
    }
    const WidePlan w = plan_wide_tiers(N, compact_ok, sc.iters, n_levels, tiers, c->n_cu, allow_finest, team_tiers_possible(c, flags));
    if (!w.whole_pyramid_one_launch && !(w.tier[0] | w.tier[1] | w.tier[2])) return DVO_OK;
    HIPCHK(c, hipMemcpyAsync(d_pose, h_pose_in, sizeof(double) * 12, hipMemcpyHostToDevice, c->stream));
    if (w.whole_pyramid_one_launch) {
        const int rc = enqueue(c, range_request(pair, 1, n_levels, iters, flags & DVO_FLAG_FINAL_OUTPUTS));
        if (rc) return rc;
        coarse_team = c->team_used;
        for (int l = 0; l < n_levels; l++) if (sc.iters[l] > 0) coarse_mask |= 1u << l;
    }
    for (int k = 0; k < 3 && !w.whole_pyramid_one_launch; k++) {
        if (!w.tier[k]) continue;
        EnqueueRequest q = range_request(pair, 1, n_levels, iters, (k == 2) ? (flags & DVO_FLAG_FINAL_OUTPUTS) : 0);
        q.level_mask = w.tier[k];
        q.forced_team = tiers.size[k];
        const int rc = enqueue(c, q);
        if (rc) return rc;
        coarse_team = coarse_team || c->team_used;
        coarse_mask |= w.tier[k];
    }
    for (int l = 0; l < n_levels; l++) if ((coarse_mask >> l) & 1u) sc.iters[l] = 0;      /* what is left for the step launches */
    sc.last_level = -1;
    for (int l = n_levels - 1; l >= 0; l--) if (sc.iters[l] > 0) sc.last_level = l;
    return DVO_OK;
}

/* after the wait of a wide / tiled alignment: the outputs follow the WHOLE schedule again (the team launches stamped their own);
 * all_team: every level ran inside team launches of the fused kernel, whose final outputs sit in the compact list's order */
int stamp_step_alignment(dvo_ctx *c, Schedule &sc, int pair, int n_levels, const int *iters, int flags, unsigned coarse_mask, bool coarse_team) {
    const bool all_team = coarse_mask != 0 && sc.last_level < 0;
    if (coarse_mask) {
        const int rc = build_schedule(c, n_levels, iters, flags, sc);
        if (rc) return rc;
    }
    sc.final_blk = all_team ? 1 : 0;
    c->wide_team_mask = (int)coarse_mask;
    stamp_outputs(c, sc, pair, 1);
    c->sched = sc;
    c->have_sched = true;
    c->team_used = coarse_team;
    return DVO_OK;
}

hipError_t enqueue_step_schedule(dvo_ctx *c, const Schedule &sc, int pair, int flags, double *d_pose, int rank, int world,
                                 const std::function<hipError_t(double *)> &all_reduce) {
    hipError_t first_err = hipSuccess;
    auto rec = [&first_err](hipError_t e) { if (first_err == hipSuccess && e != hipSuccess) first_err = e; };
    char *st[2] = {c->d_step_state, c->d_step_state + pose_state_bytes()};
    double *acc[2] = {c->d_step_acc, c->d_step_acc + DVO_NACC_PAD};
    double *partials = c->d_scratch;
    int cur = 0, k = 0;                                                 /* state to read next; launches so far (the sums alternate) */
    bool first_level = true;
    c->step_pk_mask = 0;
    c->step_solo_mask = 0;
    for (int l = sc.n_levels - 1; l >= 0; --l) {                        /* :2097 */
        if (sc.iters[l] <= 0) continue;                                 /* :2099 */
        const int N = c->lv[l].hN[pair];
        int first = 0, count = 0;
        shard_of(N, rank, world, first, count);
        float *energy = c->d_energy + (size_t)pair * sc.e_stride + sc.e_off[l];
        const LevelSlab sl = slab_of(c, l);
        /* the first level's state comes from the pose; every later level's was prepared by the finish launch of the level before it */
        if (first_level) rec(launch_iter_begin(st[cur], c->dprm, d_pose, energy, sc.iters[l], c->stream));
        first_level = false;
        const int nb = tiled_step_blocks(count, c->n_cu);
        /* DVO_FLAG_NORMAL_MATRIX: the launches also form H = sum w J J^T (21 more double sums per point: + 40 % on the launch),
         * it rides in the same 32 doubles through the all-reduce and is kept per iterate (dvo_get_level_normal_matrix); without
         * the flag those 21 slots are zeros -- the reference's update never reads them (SolveDVO.cpp:777) */
        double *H = (flags & DVO_FLAG_NORMAL_MATRIX) ? c->d_H + ((size_t)pair * sc.e_stride + sc.e_off[l]) * 21 : nullptr;
        /* round 5: the packed point loop (dvo_fused.hip: tiled_step_pk_kernel) where the level's list has its compact twin -- lists built
         * by the engine's own enlist kernels do -- and the interpolating look-up is not asked for (H rides along); DVO_TILED_PACKED=off for A/B */
        static const bool pk_off = [] { const char *e = std::getenv("DVO_TILED_PACKED"); return e && std::strcmp(e, "off") == 0; }();
        const bool pk = !pk_off && !c->prm.interpolate_dt && c->prm.engine_variant != 1 && sl.cpts &&
                        !c->lv[l].compact_ok.empty() && c->lv[l].compact_ok[pair];
        if (pk) c->step_pk_mask |= 1 << l;
        int ln = l - 1;                                                 /* the next level that runs */
        while (ln >= 0 && sc.iters[ln] <= 0) --ln;
        float *next_energy = ln >= 0 ? c->d_energy + (size_t)pair * sc.e_stride + sc.e_off[ln] : nullptr;
        const int next_iters = ln >= 0 ? sc.iters[ln] : 0;
        /* round 5: a small level as ONE launch of one workgroup (dvo_fused.hip: tiled_level_solo_kernel) -- every rank runs it over the
         * whole list, so its iterations need no collective either.  DVO_TILED_SOLO_MAX=n: levels of at most n points (0 = never) */
        static const int solo_max = [] { const char *e = std::getenv("DVO_TILED_SOLO_MAX"); return e ? std::atoi(e) : DVO_TILED_SOLO_MAX_DEFAULT; }();
        if (pk && !H && N <= solo_max) {
            c->step_solo_mask |= 1 << l;
            rec(launch_tiled_level_solo(sl, pair, l, intrinsics_of(c, pair), st[cur], st[cur ^ 1], sc.iters[l], N, energy, d_pose,
                                        c->d_best + pair * DVO_LEVELS + l, c->d_ratio + pair * DVO_LEVELS + l, next_energy, next_iters, c->stream));
            cur ^= 1;
            if ((flags & DVO_FLAG_FINAL_OUTPUTS) && l == sc.last_level)
                rec(launch_final_outputs_state(sl, pair, l, intrinsics_of(c, pair), st[cur], first, count, c->d_final_eps + (size_t)pair * c->final_cap,
                                               c->d_final_reproj + (size_t)pair * c->final_cap * 3, c->d_final_N + pair, c->stream));
            continue;
        }
        for (int itr = 0; itr < sc.iters[l]; itr++, k++) {
            const int apply = itr > 0;
            if (pk)
                rec(launch_tiled_step_pk(sl, pair, l, intrinsics_of(c, pair), st[cur], st[cur ^ 1], acc[(k + 1) & 1], itr, apply, N, first, count, partials,
                                         c->d_step_ticket, acc[k & 1], energy, nb, H ? H + (size_t)(itr > 0 ? itr - 1 : 0) * 21 : nullptr, c->stream));
            else
            rec(launch_tiled_step(sl, pair, l, intrinsics_of(c, pair), c->dprm, st[cur], st[cur ^ 1], acc[(k + 1) & 1], itr, apply, N, first, count, partials,
                                  c->d_step_ticket, acc[k & 1], energy, nb, H ? H + (size_t)(itr > 0 ? itr - 1 : 0) * 21 : nullptr, c->stream));
            if (apply) cur ^= 1;
            if (all_reduce) rec(all_reduce(acc[k & 1]));
        }
        rec(launch_tiled_finish(st[cur], st[cur ^ 1], c->dprm, acc[(k + 1) & 1], sc.iters[l] - 1, N, energy, d_pose,
                                c->d_best + pair * DVO_LEVELS + l, c->d_ratio + pair * DVO_LEVELS + l,
                                H ? H + (size_t)(sc.iters[l] - 1) * 21 : nullptr, next_energy, next_iters, c->stream));
        cur ^= 1;
        /* finalEpsilons / finalReprojections (:703-704, :1002-1003): this rank's share, at the points' own indices */
        if ((flags & DVO_FLAG_FINAL_OUTPUTS) && l == sc.last_level)
            rec(launch_final_outputs_state(sl, pair, l, intrinsics_of(c, pair), st[cur], first, count, c->d_final_eps + (size_t)pair * c->final_cap,
                                           c->d_final_reproj + (size_t)pair * c->final_cap * 3, c->d_final_N + pair, c->stream));
    }
    return first_err;
}

unsigned long long step_schedule_signature(dvo_ctx *c, const Schedule &sc, int pair, int n_levels, int flags, int rank, int world) {
    unsigned long long sig = 1469598103934665603ull;
    auto mix = [&sig](unsigned long long v) { sig = (sig ^ v) * 1099511628211ull; };
    mix((unsigned long long)pair); mix((unsigned long long)n_levels); mix((unsigned long long)(size_t)c->stream);
    mix((unsigned long long)flags); mix((unsigned long long)(size_t)c->d_final_eps.get()); mix((unsigned long long)c->final_cap);
    mix((unsigned long long)(size_t)c->d_energy.get()); mix((unsigned long long)sc.e_stride); mix((unsigned long long)rank); mix((unsigned long long)world);
    mix((unsigned long long)(size_t)c->d_H.get());
    for (int l = 0; l < n_levels; l++) {
        const LevelSlab sl = slab_of(c, l);
        mix((unsigned long long)sc.iters[l]); mix((unsigned long long)c->lv[l].hN[pair]);
        mix((unsigned long long)(size_t)sl.tex); mix((unsigned long long)(size_t)sl.pts); mix((unsigned long long)sl.tex_stride);
        mix((unsigned long long)(size_t)sl.cpts);                       /* which step kernel a level gets (enqueue_step_schedule: pk) */
        mix((unsigned long long)((!c->lv[l].compact_ok.empty() && c->lv[l].compact_ok[pair]) ? 1 : 0));
        mix((unsigned long long)sl.pt_cap); mix((unsigned long long)sl.rows); mix((unsigned long long)sl.cols);
    }
    { const Intrinsics kp = intrinsics_of(c, pair); unsigned long long kb[3] = {0, 0, 0}; std::memcpy(kb, &kp, sizeof(kb)); mix(kb[0]); mix(kb[1]); mix(kb[2]); }
    { unsigned long long pb[16] = {0}; std::memcpy(pb, &c->dprm, sizeof(c->dprm) < sizeof(pb) ? sizeof(c->dprm) : sizeof(pb)); for (unsigned long long v : pb) mix(v); }
    return sig;
}

}  // namespace dvo_host

extern "C" {

int dvo_align_pyramid_wide(dvo_ctx *c, int pair, int n_levels, const int *iters, int flags, double *R, double *t) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !R || !t) return fail(c, DVO_ERR_INVALID, "bad arguments");
    if (flags & ~(DVO_FLAG_FINAL_OUTPUTS | DVO_FLAG_NORMAL_MATRIX)) return fail(c, DVO_ERR_INVALID, "dvo_align_pyramid_wide takes DVO_FLAG_FINAL_OUTPUTS and DVO_FLAG_NORMAL_MATRIX only");
    Schedule sc;
    int rc = build_schedule(c, n_levels, iters, flags, sc);
    if (rc) return rc;
    for (int l = 0; l < n_levels; l++)
        if (sc.iters[l] > 0 && ((rc = check_ready(c, pair, l)) || (rc = ensure_tex16(c, l, pair, 1)))) return rc;
    if ((rc = ensure_outputs(c, sc))) return rc;
    if ((rc = ensure_step_buffers(c))) return rc;
    if (!c->h_pose) HIPCHK(c, c->h_pose.alloc(14));      /* [12]: the step launches' error word, [13]: the team launches' */
    double *h = c->h_pose;
    std::memcpy(h, R, sizeof(double) * 9);
    std::memcpy(h + 9, t, sizeof(double) * 3);
    double *d_pose = c->d_poses + (size_t)12 * pair;
    unsigned coarse_mask = 0;
    bool coarse_team = false;
    if ((rc = dvo_host::wide_coarse_levels_as_team(c, pair, n_levels, iters, flags, sc, h, d_pose, coarse_mask, coarse_team, true))) return rc;
    const bool all_team = coarse_mask != 0 && sc.last_level < 0;      /* every level ran inside team launches: no step launch, no graph */
    if (all_team) c->step_pk_mask = c->step_solo_mask = 0;            /* no step launch is enqueued: dvo_wide_packed_levels must not report the schedule before this one */
    /* everything the enqueued sequence depends on; an unchanged signature replays the instantiated graph.  One launch per iteration
     * (round 4: the update of an iteration rides at the head of the next one's accumulate launch, the partial sums are added by the
     * workgroup that arrives last -- dvo_kernels.hip: tiled_step_kernel); rounds 1-3 used two. */
    const unsigned long long sig = step_schedule_signature(c, sc, pair, n_levels, flags, 0, 1) ^ ((unsigned long long)coarse_mask << 48);
    const bool no_graph = c->stream == nullptr;                                    /* the legacy null stream cannot be captured */
    if (all_team) {
        HIPCHK(c, hipMemcpyAsync(h, d_pose, sizeof(double) * 12, hipMemcpyDeviceToHost, c->stream));
        std::memset(h + 12, 0, sizeof(double));
    } else if (no_graph || !c->wide_exec || sig != c->wide_sig) {
        if (c->wide_exec) { (void)hipGraphExecDestroy(c->wide_exec); c->wide_exec = nullptr; }
        if (!no_graph) HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        hipError_t first_err = hipSuccess;
        auto rec = [&first_err](hipError_t e) { if (first_err == hipSuccess && e != hipSuccess) first_err = e; };
        if (!coarse_mask) rec(hipMemcpyAsync(d_pose, h, sizeof(double) * 12, hipMemcpyHostToDevice, c->stream));      /* else: went in front of the team launch */
        rec(enqueue_step_schedule(c, sc, pair, flags, d_pose, 0, 1, nullptr));
        rec(hipMemcpyAsync(h, d_pose, sizeof(double) * 12, hipMemcpyDeviceToHost, c->stream));
        rec(hipMemcpyAsync(h + 12, c->d_step_ticket + 2, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        if (!no_graph) {
            hipGraph_t graph = nullptr;
            rec(hipStreamEndCapture(c->stream, &graph));
            if (first_err == hipSuccess) rec(hipGraphInstantiate(&c->wide_exec, graph, nullptr, nullptr, 0));
            if (graph) (void)hipGraphDestroy(graph);
            c->wide_sig = sig;
        }
        HIPCHK(c, first_err);
    }
    if (!no_graph && !all_team) HIPCHK(c, hipGraphLaunch(c->wide_exec, c->stream));
    c->team_used = coarse_team;
    HIPCHK(c, dvo_host::team_err_fetch(c, reinterpret_cast<int *>(h + 13)));
    HIPCHK(c, stream_wait(c->stream));
    { const int lrc = dvo_host::check_step_lost(c); if (lrc) return lrc; }
    { const int trc = dvo_host::team_err_result(c, reinterpret_cast<const int *>(h + 13)); if (trc) return trc; }
    std::memcpy(R, h, sizeof(double) * 9);
    std::memcpy(t, h + 9, sizeof(double) * 3);
    return dvo_host::stamp_step_alignment(c, sc, pair, n_levels, iters, flags, coarse_mask, coarse_team);
}

/* ---- inspection ------------------------------------------------------------- */
int dvo_eval_points(dvo_ctx *c, int pair, int level, const double *R, const double *t,
                    float *reproj, float *J, float *eps, float *w, int *visible) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !R || !t) return fail(c, DVO_ERR_INVALID, "bad arguments");
    int rc = check_ready(c, pair, level);
    if (rc) return rc;
    const int N = c->lv[level].hN[pair];
    if ((rc = ensure_tex16(c, level, pair, 1))) return rc;
    /* staging: reproj 3N | J 6N | eps N | w N | vis N  (floats/ints, 4 bytes each) */
    if ((rc = ensure_staging(c, sizeof(float) * 12 * (size_t)N))) return rc;
    float *d_re = c->staging, *d_J = d_re + 3 * (size_t)N, *d_e = d_J + 6 * (size_t)N, *d_w = d_e + N;
    int *d_v = (int *)(d_w + N);
    float Rf[9], tf[3];
    cast_pose(R, t, Rf, tf);
    HIPCHK(c, launch_eval_points(slab_of(c, level), pair, level, intrinsics_of(c, pair), Rf, tf, d_re, d_J, d_e, d_w, d_v, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    if (reproj) HIPCHK(c, hipMemcpy(reproj, d_re, sizeof(float) * 3 * (size_t)N, hipMemcpyDeviceToHost));
    if (J) HIPCHK(c, hipMemcpy(J, d_J, sizeof(float) * 6 * (size_t)N, hipMemcpyDeviceToHost));
    if (eps) HIPCHK(c, hipMemcpy(eps, d_e, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
    if (w) HIPCHK(c, hipMemcpy(w, d_w, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
    if (visible) HIPCHK(c, hipMemcpy(visible, d_v, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_accumulate(dvo_ctx *c, int pair, int level, const double *R, const double *t, double *acc29) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !R || !t || !acc29) return fail(c, DVO_ERR_INVALID, "bad arguments");
    int rc = check_ready(c, pair, level);
    if (rc) return rc;
    if ((rc = ensure_tex16(c, level, pair, 1))) return rc;
    const int N = c->lv[level].hN[pair];
    float Rf[9], tf[3];
    cast_pose(R, t, Rf, tf);
    const int nb = accumulate_blocks_for(N);
    double *partials = c->d_scratch, *acc = c->d_scratch + 1024 * DVO_NACC_PAD;
    HIPCHK(c, launch_accumulate(slab_of(c, level), pair, level, intrinsics_of(c, pair), Rf, tf, 0, N, partials, nb, acc, c->stream));
    double h[DVO_NACC_PAD];
    HIPCHK(c, hipMemcpyAsync(h, acc, sizeof(double) * DVO_NACC_PAD, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    std::memcpy(acc29, h, sizeof(double) * DVO_NUM_ACC);
    /* sum eps^2 = the correctly rounded exact sum (the three limbs in slots 29..31; dvo_device_math.h: the energy without an order);
     * the sum as the kernel added it only if a residual was outside the limbs' range (2^50 in limb 2) */
    if (h[31] < 1125899906842624.0) {
        unsigned __int128 S = (unsigned __int128)(unsigned long long)h[29] + ((unsigned __int128)(unsigned long long)h[30] << 32) +
                              ((unsigned __int128)(unsigned long long)h[31] << 64);
        double v = 0.0;
        if (S != 0) {
            int p = 127;
            while (!((S >> p) & 1)) p--;
            if (p <= 52) v = std::ldexp((double)(unsigned long long)S, -68);
            else {
                const int r = p - 52;
                unsigned long long q = (unsigned long long)(S >> r);
                const unsigned __int128 rem = S & ((((unsigned __int128)1) << r) - 1), half = ((unsigned __int128)1) << (r - 1);
                if (rem > half || (rem == half && (q & 1ull))) q++;
                v = std::ldexp((double)q, r - 68);
            }
        }
        acc29[27] = v;
    }
    return DVO_OK;
}

int dvo_device_se3_exp(dvo_ctx *c, const double *psi6, double *R, double *t) {
    DVO_ENTER(c);
    if (!psi6 || !R || !t) return DVO_ERR_INVALID;
    double *d = c->d_scratch;
    HIPCHK(c, hipMemcpyAsync(d, psi6, sizeof(double) * 6, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_se3_exp(d, d + 8, c->stream));
    double h[12];
    HIPCHK(c, hipMemcpyAsync(h, d + 8, sizeof(double) * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    std::memcpy(R, h, sizeof(double) * 9);
    std::memcpy(t, h + 9, sizeof(double) * 3);
    return DVO_OK;
}
int dvo_device_se3_log(dvo_ctx *c, const double *R, const double *t, double *psi6) {
    DVO_ENTER(c);
    if (!psi6 || !R || !t) return DVO_ERR_INVALID;
    double *d = c->d_scratch;
    double h[12];
    std::memcpy(h, R, sizeof(double) * 9);
    std::memcpy(h + 9, t, sizeof(double) * 3);
    HIPCHK(c, hipMemcpyAsync(d, h, sizeof(double) * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_se3_log(d, d + 16, c->stream));
    HIPCHK(c, hipMemcpyAsync(psi6, d + 16, sizeof(double) * 6, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}
int dvo_device_rotationize(dvo_ctx *c, double *R) {
    DVO_ENTER(c);
    if (!R) return DVO_ERR_INVALID;
    double *d = c->d_scratch;
    HIPCHK(c, hipMemcpyAsync(d, R, sizeof(double) * 9, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rotationize(d, c->stream));
    HIPCHK(c, hipMemcpyAsync(R, d, sizeof(double) * 9, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c->stream));
    return DVO_OK;
}

/* diagnostics: the library has no phase cycle counters; kept for the C ABI, always zeros */
int dvo_debug_stamps(dvo_ctx *c, int pair, unsigned long long *out64) {
    DVO_ENTER(c);
    if (!out64 || !pair_ok(c, pair)) return DVO_ERR_INVALID;
    std::memset(out64, 0, sizeof(unsigned long long) * 64);
    return DVO_OK;
}

/* inspection: where the packed fused kernel read the now level of (pair, level) from during the last launch that ran it */
int dvo_get_level_texel_mode(dvo_ctx *c, int pair, int level, int *mode) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !mode) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *mode = (v < 0) ? -1 : (v & 0xff);
    return DVO_OK;
}
int dvo_get_level_points4(dvo_ctx *c, int pair, int level, int *used) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !used) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *used = (v >= 0 && (v & DVO_TEXMODE_PT4)) ? 1 : 0;
    return DVO_OK;
}
int dvo_get_level_points4_direct(dvo_ctx *c, int pair, int level, int *used) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !used) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *used = (v >= 0 && (v & DVO_TEXMODE_PT4_DIRECT)) ? 1 : 0;
    return DVO_OK;
}
int dvo_get_level_final_fused(dvo_ctx *c, int pair, int level, int *fused) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !fused) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *fused = (v >= 0 && (v & DVO_TEXMODE_FINAL_FUSED)) ? 1 : 0;
    return DVO_OK;
}
/* 1 if the last fused launch looked that level's ranks up in an LDS copy of the whole level (round 5: coarse levels whose compact form
 * fits the LDS beside palette and points; dvo_get_level_texel_mode says 2 = compact form for them) */
int dvo_get_level_ranks_in_lds(dvo_ctx *c, int pair, int level, int *used) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !used) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *used = (v >= 0 && (v & DVO_TEXMODE_RANKS_LDS)) ? 1 : 0;
    return DVO_OK;
}
int dvo_get_level_exact_fallback(dvo_ctx *c, int pair, int level, int *ran) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !ran) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *ran = (v >= 0 && (v & DVO_TEXMODE_EXACT_RAN)) ? 1 : 0;
    return DVO_OK;
}

int dvo_get_level_energy_sweeps(dvo_ctx *c, int pair, int level, int *n) {
    DVO_ENTER(c);
    if (!pair_ok(c, pair) || !level_ok(level) || !n) return fail(c, DVO_ERR_INVALID, "bad arguments");
    HIPCHK(c, stream_wait(c->stream));
    int v = -1;
    HIPCHK(c, hipMemcpy(&v, c->d_tex_mode + (size_t)pair * DVO_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *n = (v < 0) ? 0 : ((v >> DVO_TEXMODE_E2_SHIFT) & DVO_TEXMODE_E2_MAX);
    return DVO_OK;
}

/* ---- measurement support ------------------------------------------------------ */
int dvo_algorithmic_bytes(dvo_ctx *c, int pair, int n_levels, const int *iters, int flags, uint64_t *bytes) {
    DVO_ENTER(c);
    if (!bytes) return DVO_ERR_INVALID;
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    Schedule sc;
    int rc = build_schedule(c, n_levels, iters, flags, sc);
    if (rc) return rc;
    uint64_t b = 0;
    for (int l = 0; l < n_levels; l++) {
        if (sc.iters[l] <= 0) continue;
        if ((rc = check_ready(c, pair, l))) return rc;
        b += 12ull * (uint64_t)c->lv[l].rows * (uint64_t)c->lv[l].cols;   /* DT, gx, gy f32 */
        b += 12ull * (uint64_t)c->lv[l].hN[pair];                         /* xyz f32 */
    }
    if (flags & DVO_FLAG_FINAL_OUTPUTS) b += 16ull * (uint64_t)c->lv[sc.last_level].hN[pair];
    *bytes = b;
    return DVO_OK;
}

int dvo_point_iterations(dvo_ctx *c, int pair, int n_levels, const int *iters, uint64_t *count) {
    DVO_ENTER(c);
    if (!count) return DVO_ERR_INVALID;
    if (!pair_ok(c, pair)) return fail(c, DVO_ERR_INVALID, "pair out of range");
    Schedule sc;
    int rc = build_schedule(c, n_levels, iters, 0, sc);
    if (rc) return rc;
    uint64_t n = 0;
    for (int l = 0; l < n_levels; l++) {
        if (sc.iters[l] <= 0) continue;
        if ((rc = check_ready(c, pair, l))) return rc;
        n += (uint64_t)sc.iters[l] * (uint64_t)c->lv[l].hN[pair];
    }
    *count = n;
    return DVO_OK;
}

}  // extern "C"
