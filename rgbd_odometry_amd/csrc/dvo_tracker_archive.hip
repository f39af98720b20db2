/*
 * dvo_tracker_archive.hip -- the key-frame archive of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_archive,
 * dvo_tracker_score, dvo_tracker_match; host side dvo_capi_tracker_archive.cpp, the store of a step dvo_capi_tracker.cpp).
 *
 * Four kernels, none of which touches the alignment:
 *   archive_store_kernel   a step's new key frames -> their slots of the ring: ONE launch for every stream that got a key frame and every
 *                          level, a plain device-side copy of the lists the reference extraction has just written (compact points, their
 *                          4-byte twins and chunk headers, cidx) and of the slot's header.
 *   archive_decode_kernel  a slot's list of one level as the 3 x N floats of dvo_get_ref_level (inspection: dvo_tracker_archive_get_points).
 *   archive_load_kernel    the candidates of dvo_tracker_match -> the pairs of the tracker's private match context: the slot's lists and the
 *                          stream's resident now levels (rank words, palette, 16-byte texels where they are the image's real form), device
 *                          to device, ONE launch -- across contexts what dvo_replicate_pairs does inside one.
 *   archive_score_kernel   the engine's accumulators of one archived list against one stream's now level at a given pose: ONE launch, one
 *                          512-thread workgroup per candidate.  It reads the slot and the stream's compact now level where they are -- rank
 *                          words from HBM, the palette in LDS, 16-byte texels for a partial or refused form.  The walk is the information
 *                          kernel's (dvo_tracker_info.h: the per-point code of dvo_device_math.h), the reduction is block_reduce (lanes,
 *                          then the waves in wave order): a record depends on its own candidate's list, now level and pose alone -- not on
 *                          how many candidates are listed, nor on their order.
 *
 * Every index is bounded by the capacities the host passes: a count read from the device is clamped to the slab it indexes.
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_tracker_info.h"

#include <mutex>
#include <vector>

namespace dvo {

namespace {

constexpr int COPY_BLOCK = 256;
constexpr int STORE_Z = 4, LOAD_Z = 8;      /* workgroups that share one (entry, level) */

/* n elements src -> dst by the workgroups blockIdx.z of gridDim.z */
template <typename T>
DVO_DEV void copy_share(T *__restrict__ dst, const T *__restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.z * COPY_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.z * COPY_BLOCK) dst[i] = src[i];
}

DVO_DEV int clamp_count(int N, int cap_a, int cap_b) {
    const int cap = cap_a < cap_b ? cap_a : cap_b;
    return N < 0 ? 0 : (N > cap ? cap : N);
}

}  // namespace

__global__ void __launch_bounds__(COPY_BLOCK)
archive_store_kernel(const ArchiveStore *__restrict__ entries, LevelSet src, ArchiveView A) {
    const ArchiveStore e = entries[blockIdx.x];
    const int l = blockIdx.y;
    if (e.slot < 0 || e.slot >= A.n_slots || l >= A.n_levels) return;
    const LevelSlab &S = src.l[l];
    const ArchiveLevel &D = A.l[l];
    const int N = S.N[e.pair];
    const int n = clamp_count(N, D.cap, S.pt_cap);
    const size_t so = (size_t)e.pair * S.pt_cap, dofs = (size_t)e.slot * D.cap;
    copy_share(D.cpts + dofs, S.cpts + so, (size_t)n);
    copy_share(D.cidx + dofs, S.cidx + so, (size_t)n);
    copy_share(D.cpt4 + dofs, S.cpt4 + so, (size_t)n);
    copy_share(D.chdr + (size_t)e.slot * (D.cap / 64), S.chdr + (size_t)e.pair * (S.pt_cap / 64), (size_t)((n + 63) / 64));
    if (blockIdx.z == 0 && threadIdx.x == 0) {
        ArchiveHeader &h = A.hdr[e.slot];
        h.N[l] = (n == N) ? N : 0;                /* a clamped list is no list */
        h.pt4_ok[l] = (n == N && S.pt4_ok) ? S.pt4_ok[e.pair] : 0;
        if (l == 0) { h.K = e.K; h.stream = e.pair; h.pad_ = 0; h.frame = e.frame; }
    }
}

__global__ void __launch_bounds__(COPY_BLOCK)
archive_decode_kernel(ArchiveView A, int slot, int level, float *__restrict__ xyz, int capacity) {
    const ArchiveHeader &h = A.hdr[slot];
    const ArchiveLevel &D = A.l[level];
    const int N = clamp_count(h.N[level], D.cap, D.cap);
    const int i = blockIdx.x * COPY_BLOCK + threadIdx.x;
    if (i >= N) return;
    Intrinsics K{h.K.x, h.K.y, h.K.z, h.K.w, 0, 0, nullptr};
    IterConst c;
    level_consts(c, K, level, 16, 16);            /* the point constants depend on the camera model and the level alone */
    const uint2 v = D.cpts[(size_t)slot * D.cap + i];
    const unsigned k = D.cidx[(size_t)slot * D.cap + i];
    float X, Y, Z;
    expand_compact(c, v.x, __uint_as_float(v.y), X, Y, Z);
    if (k < (unsigned)N && k < (unsigned)capacity) { xyz[3 * (size_t)k] = X; xyz[3 * (size_t)k + 1] = Y; xyz[3 * (size_t)k + 2] = Z; }
}

__global__ void __launch_bounds__(COPY_BLOCK)
archive_load_kernel(const ArchiveLoad *__restrict__ cands, ArchiveView A, LevelSet now, ArchiveDst dst) {
    const ArchiveLoad &cd = cands[blockIdx.x];
    const int l = blockIdx.y;
    const int slot = cd.slot, q = cd.dst, p = cd.now_pair;
    if (slot < 0 || slot >= A.n_slots || l >= A.n_levels) return;
    const ArchiveLevel &R = A.l[l];
    const ArchiveDst::Lv &D = dst.l[l];
    const LevelSlab &S = now.l[l];
    /* the reference lists */
    const int N = A.hdr[slot].N[l];
    const int n = clamp_count(N, R.cap, D.pt_cap);
    const size_t so = (size_t)slot * R.cap, dofs = (size_t)q * D.pt_cap;
    copy_share(D.cpts + dofs, R.cpts + so, (size_t)n);
    copy_share(D.cidx + dofs, R.cidx + so, (size_t)n);
    copy_share(D.cpt4 + dofs, R.cpt4 + so, (size_t)n);
    copy_share(D.chdr + (size_t)q * (D.pt_cap / 64), R.chdr + (size_t)slot * (R.cap / 64), (size_t)((n + 63) / 64));
    /* the now level, in the form(s) the stream holds it: both contexts have the level's geometry, hence its strides */
    const bool compact = S.p4 && S.pal_n && D.p4;
    const int pal_n = compact ? S.pal_n[p] : 0;
    if (pal_n > 0) {
        const size_t words = S.p4_stride;
        const unsigned *sp = S.p4 + (size_t)p * words;
        unsigned *dp = D.p4 + (size_t)q * words;
        if ((words & 3) == 0) copy_share(reinterpret_cast<uint4 *>(dp), reinterpret_cast<const uint4 *>(sp), words >> 2);
        else copy_share(dp, sp, words);
        /* + the zero sentinel, + a partial form's NaN entry right after it (dvo_palette.h): the look-up that meets it sends the alignment
         * kernel to the texels.  The builders keep pal_count <= DVO_PAL_MAX - 2; clamped to the slab like every count read from the device */
        const int n_copy = pal_count(pal_n) + (pal_partial(pal_n) ? 2 : 1);
        copy_share(D.pal + (size_t)q * DVO_PAL_MAX, S.pal + (size_t)p * DVO_PAL_MAX, (size_t)(n_copy < DVO_PAL_MAX ? n_copy : DVO_PAL_MAX));
    }
    /* 16-byte texels are an image's real form where it has no complete compact one: the device knows (pal_n), the host may not yet */
    const bool backed = D.tex_dense || ((cd.tex_mask >> (8 + l)) & 1);      /* a sparse slab: the host mapped memory where it could not tell */
    const bool tex_real = ((cd.tex_mask >> l) & 1) || (backed && (!compact || pal_n <= 0 || pal_partial(pal_n)));
    if (tex_real && S.tex && D.tex)
        copy_share(D.tex + (size_t)q * S.tex_stride, S.tex + (size_t)p * S.tex_stride, S.tex_stride);
    if (blockIdx.z == 0 && threadIdx.x == 0) {
        D.N[q] = (n == N) ? N : 0;
        D.pt4_ok[q] = (n == N) ? A.hdr[slot].pt4_ok[l] : 0;
        if (D.pal_n) D.pal_n[q] = pal_n;
        if (l == 0) {
            for (int k = 0; k < 12; k++) dst.poses[(size_t)q * 12 + k] = cd.pose[k];
            if (dst.pair_K) dst.pair_K[q] = A.hdr[slot].K;
        }
    }
}

__global__ void __launch_bounds__(INFO_BLOCK)
archive_score_kernel(const ScoreCand *__restrict__ cands, const double *__restrict__ poses, ArchiveView A, LevelSlab L, int level,
                     Intrinsics K, int use_p4, ScoreRecord *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) double red[INFO_BLOCK / 64][DVO_NACC_PAD];
    __shared__ __attribute__((aligned(16))) double tot[DVO_NACC_PAD];
    extern __shared__ __attribute__((aligned(16))) float2 pal_lds[];      /* DVO_PAL_MAX entries */
    const int i = blockIdx.x;
    const int slot = __builtin_amdgcn_readfirstlane(cands[i].slot);
    const int p = __builtin_amdgcn_readfirstlane(cands[i].now_pair);
    const int pi = __builtin_amdgcn_readfirstlane(cands[i].pose_idx);
    const ArchiveLevel &R = A.l[level];
    const ArchiveHeader &h = A.hdr[slot];
    const int N = __builtin_amdgcn_readfirstlane(clamp_count(h.N[level], R.cap, R.cap));
    const uint2 *__restrict__ pts = R.cpts + (size_t)slot * R.cap;

    /* the slot's camera model: the host refuses a candidate whose stream has another one */
    Intrinsics Kc = K;
    const float4 k4 = h.K;
    Kc.fx = uniform_f(k4.x); Kc.fy = uniform_f(k4.y); Kc.cx = uniform_f(k4.z); Kc.cy = uniform_f(k4.w);
    Kc.pair_K = nullptr;
    IterConst c;
    level_consts(c, Kc, level, L.rows, L.cols);
    info_set_pose(c, poses + (size_t)pi * 12);

    Acc a;
    acc_zero(a);
    if (N > 0) info_accumulate(c, pts, N, L, p, use_p4, pal_lds, a);
    block_reduce<INFO_BLOCK, true>(a, red, tot);
    ScoreRecord &o = out[i];
    if (threadIdx.x < 21) o.H[threadIdx.x] = tot[threadIdx.x];
    else if (threadIdx.x < 27) o.g[threadIdx.x - 21] = tot[threadIdx.x];
    else if (threadIdx.x == 27) {
        o.sum_eps2 = acc_sum_eps2(tot);
        o.n_visible = (int)tot[28];
        o.n_points = N;
    }
}

hipError_t launch_archive_store(const ArchiveStore *entries, int count, const LevelSet &src, const ArchiveView &A, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_store_kernel, dim3(count, A.n_levels, STORE_Z), dim3(COPY_BLOCK), 0, s, entries, src, A);
    return hipGetLastError();
}

hipError_t launch_archive_decode(const ArchiveView &A, int slot, int level, float *xyz, int capacity, hipStream_t s) {
    const int cap = A.l[level].cap;
    if (cap <= 0 || capacity <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_decode_kernel, dim3((cap + COPY_BLOCK - 1) / COPY_BLOCK), dim3(COPY_BLOCK), 0, s, A, slot, level, xyz, capacity);
    return hipGetLastError();
}

hipError_t launch_archive_load(const ArchiveLoad *cands, int count, const ArchiveView &A, const LevelSet &now, const ArchiveDst &dst, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_load_kernel, dim3(count, A.n_levels, LOAD_Z), dim3(COPY_BLOCK), 0, s, cands, A, now, dst);
    return hipGetLastError();
}

hipError_t launch_archive_score(const ScoreCand *cands, int count, const double *poses, const ArchiveView &A, const LevelSlab &now, int level,
                                const Intrinsics &K, bool use_p4, ScoreRecord *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const size_t dyn = sizeof(float2) * DVO_PAL_MAX;
    /* once per process and device: the attribute belongs to the kernel, not to a launch */
    static std::mutex once_mutex;
    static std::vector<char> once_done;
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(once_mutex);
        if ((size_t)dev >= once_done.size()) once_done.resize((size_t)dev + 1, 0);
        if (!once_done[dev]) {
            e = hipFuncSetAttribute((const void *)archive_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
            if (e != hipSuccess) return e;
            once_done[dev] = 1;
        }
    }
    hipLaunchKernelGGL(archive_score_kernel, dim3(count), dim3(INFO_BLOCK), dyn, s, cands, poses, A, now, level, K, use_p4 ? 1 : 0, out);
    return hipGetLastError();
}

}  // namespace dvo
