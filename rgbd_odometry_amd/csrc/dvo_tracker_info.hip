/*
 * dvo_tracker_info.hip -- the 6x6 pose information of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_information /
 * dvo_tracker_get_information; host side dvo_capi_tracker.cpp).
 *
 * ONE launch for a whole index list, after the alignment: workgroup i takes stream p = list[i].stream at the pose the alignment left in
 * poses + 12 p (narrowed to float like every evaluation, SolveDVO.cpp:673-674), walks the reference points of the finest level that
 * ran once and writes the engine's 32 accumulators (dvo_kernel_common.h) of that pose: H = sum w J J^T (21), g = J^T W eps (6),
 * sum eps^2 (the correctly rounded exact sum, from its three limbs) and the visible count.  What dvo_accumulate gives for one pair
 * with a launch pair and a host synchronisation of its own, for K streams in one launch and without 16-byte texels: the points are read
 * from the compact list and the now level from its compact form (dvo_palette.h), the forms the tracker's context keeps resident.
 *
 * Plain on purpose: one 512-thread workgroup per stream, one point per lane and trip, no teams, no exchange between workgroups, no
 * waiting.  The per-point arithmetic is the scalar code of dvo_device_math.h (project_point, jacobian_row) and acc_add<true> of
 * dvo_kernel_common.h, hence the oracle's floats; the workgroup's sums go through block_reduce (lanes by DPP / shuffles, then the
 * waves in wave order through LDS), so a stream's record depends on that stream's data alone -- not on K, not on its place in the
 * list, not on which other streams are listed.
 *
 * The alignment kernels' sources stay as they are (the committed traffic profiles carry their hash, bench.py): the three helpers of
 * dvo_fused.hip this file needs -- U3, p4_byte_offset, p4_texel -- are restated below, line for line.
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_kernel_common.h"
#include "dvo_palette.h"

namespace dvo {

namespace {

/* restated from dvo_fused.hip: three consecutive dwords at any 4-byte boundary (one global_load_dwordx3) */
struct __attribute__((packed, aligned(4))) InfoU3 { unsigned a, b, c; };

/* restated from dvo_fused.hip (p4_byte_offset): byte offset of the rank word ABOVE pixel (yy, xx) in the compact image; the 12 bytes
 * from there are above / centre / below.  yy / 6 by multiplication (exact for yy < 98 000) */
DVO_DEV unsigned info_p4_byte_offset(int yy, int xx, unsigned p4_col_bytes /* p4_tiles_per_col * 128 */) {
    static_assert(DVO_P4_ROWS == 6, "written for 6 interior rows per line");
    const unsigned ty = __umul24((unsigned)yy, 43691u) >> 18;
    return __umul24((unsigned)(xx >> 2), p4_col_bytes) + 128u /* the sentinel line */ + (((unsigned)xx & 3u) << 5) + ((unsigned)yy << 2) + __umul24(ty, 104u);
}

/* restated from dvo_fused.hip (p4_texel): {DT, gx, gy, w} from the three rank words of a pixel and the palette.  The words of the
 * sentinel line (offset 0) point at palette entry n = {0, 0}: exact zeros */
DVO_DEV float4 info_p4_texel(const InfoU3 &w, const float2 *pal_lds) {
    const int c = (int)((w.b >> 3) & 0x1fffu);
    const int cr = c + __builtin_amdgcn_sbfe((int)w.b, 16, 8), cl = c + (((int)w.b) >> 24);
    const float2 pc = pal_lds[c];
    const float pr = pal_lds[cr].x, pl = pal_lds[cl].x, pu = pal_lds[(w.a >> 3) & 0x1fffu].x, pd = pal_lds[(w.c >> 3) & 0x1fffu].x;
    return make_float4(pc.x, (pr - pl) * 0.5f, (pd - pu) * 0.5f, pc.y);      /* imageGradient, SolveDVO.cpp:1063-1098 */
}

constexpr int INFO_BLOCK = 512;
constexpr int INFO_U = 4;          /* points per lane in flight: their look-ups are issued before any Jacobian arithmetic */

struct InfoPoint {
    float xn, yn, zn;
    bool vis;
};

/* points [base, base + INFO_U * INFO_BLOCK) of the list: project (the trip count is the workgroup's, so the visible count can be
 * taken from ballots); returns the look-up position of each (pixel 0, 0 and vis = false where there is nothing to look up) */
DVO_DEV void info_project(const IterConst &c, const uint2 *__restrict__ pts, int base, int N, InfoPoint (&b)[INFO_U], int (&px)[INFO_U],
                          int (&py)[INFO_U], Acc &a) {
#pragma unroll
    for (int u = 0; u < INFO_U; u++) {
        const int i = base + u * INFO_BLOCK + (int)threadIdx.x;
        const bool valid = i < N;
        const uint2 v = pts[valid ? i : (N - 1)];
        float X, Y, Z, uu, vv;
        expand_compact(c, v.x, __uint_as_float(v.y), X, Y, Z);
        const bool vis = project_point(c, X, Y, Z, b[u].xn, b[u].yn, b[u].zn, uu, vv) && valid;
        b[u].vis = vis;
        px[u] = vis ? (int)uu : 0;                  /* :376-377 == floor for u, v >= 0 */
        py[u] = vis ? (int)vv : 0;
        if (!vis) { b[u].xn = 0.0f; b[u].yn = 0.0f; b[u].zn = 1.0f; }      /* finite dummy: exact zeros in every sum */
        a.nvis += __popcll(__ballot(vis));
    }
}

DVO_DEV void info_add(const IterConst &c, const InfoPoint &b, const float4 &t, Acc &a) {
    float J[6];
    jacobian_row(c, b.xn, b.yn, b.zn, b.vis ? t.y : 0.0f, b.vis ? t.z : 0.0f, J);
    acc_add<true>(a, J, b.vis ? t.x : 0.0f, b.vis ? t.w : 0.0f);
}

}  // namespace

__global__ void __launch_bounds__(INFO_BLOCK)
tracker_information_kernel(const TrackerEntry *__restrict__ list, const TrackerOut *__restrict__ out, int switched,
                           const double *__restrict__ poses, LevelSlab L, int level, Intrinsics K, int use_p4,
                           TrackerInfo *__restrict__ info) {
    __shared__ __attribute__((aligned(16))) double red[INFO_BLOCK / 64][DVO_NACC_PAD];
    __shared__ __attribute__((aligned(16))) double tot[DVO_NACC_PAD];
    extern __shared__ __attribute__((aligned(16))) float2 pal_lds[];      /* DVO_PAL_MAX entries */
    const int i = blockIdx.x;
    /* the same kernel serves both launches of a step: the streams that keep their key frame after the first alignment, the streams
     * that switched after their re-run */
    if ((out[i].event >= 2) != (switched != 0)) return;
    const int p = list[i].stream;
    const int N = __builtin_amdgcn_readfirstlane(L.N[p]);
    const uint2 *__restrict__ pts = L.cpts + (size_t)p * L.pt_cap;

    IterConst c;
    level_consts(c, pair_intrinsics(K, p), level, L.rows, L.cols);
    const double *P = poses + (size_t)p * 12;
    c.r[0] = uniform_f((float)P[0]); c.r[1] = uniform_f((float)P[1]); c.r[2] = uniform_f((float)P[2]);      /* cR.cast<float>() :673 */
    c.r[3] = uniform_f((float)P[3]); c.r[4] = uniform_f((float)P[4]); c.r[5] = uniform_f((float)P[5]);
    c.r[6] = uniform_f((float)P[6]); c.r[7] = uniform_f((float)P[7]); c.r[8] = uniform_f((float)P[8]);
    c.t[0] = uniform_f((float)P[9]); c.t[1] = uniform_f((float)P[10]); c.t[2] = uniform_f((float)P[11]);    /* :674 */

    /* the now level: its compact form where it is complete; a partial form's or a refused image's real form is its 16-byte texels
     * (dvo_palette.h), and so is that of a level the context keeps as texels */
    const int pal_n_raw = (use_p4 && L.pal_n) ? __builtin_amdgcn_readfirstlane(L.pal_n[p]) : 0;
    const int n_pal = pal_count(pal_n_raw);
    const bool p4 = n_pal > 0 && !pal_partial(pal_n_raw);

    Acc a;
    acc_zero(a);
    if (p4) {
        const float2 *__restrict__ pg = L.pal + (size_t)p * DVO_PAL_MAX;
        for (int k = threadIdx.x; k <= n_pal; k += INFO_BLOCK) pal_lds[k] = pg[k];      /* + the sentinel entry {0, 0} */
        __syncthreads();
        const char *__restrict__ img = reinterpret_cast<const char *>(L.p4 + (size_t)p * L.p4_stride);
        const unsigned col_bytes = (unsigned)p4_tiles_per_col(L.rows) * 128u;
        for (int base = 0; base < N; base += INFO_U * INFO_BLOCK) {
            InfoPoint b[INFO_U];
            int px[INFO_U], py[INFO_U];
            InfoU3 w[INFO_U];
            info_project(c, pts, base, N, b, px, py, a);
#pragma unroll
            for (int u = 0; u < INFO_U; u++)       /* a lane without a visible point reads the sentinel line */
                w[u] = *reinterpret_cast<const InfoU3 *>(img + (b[u].vis ? info_p4_byte_offset(py[u], px[u], col_bytes) : 0u));
#pragma unroll
            for (int u = 0; u < INFO_U; u++) info_add(c, b[u], info_p4_texel(w[u], pal_lds), a);
        }
    } else {
        const float4 *__restrict__ tex = L.tex + (size_t)p * L.tex_stride;
        for (int base = 0; base < N; base += INFO_U * INFO_BLOCK) {
            InfoPoint b[INFO_U];
            int px[INFO_U], py[INFO_U];
            float4 t[INFO_U];
            info_project(c, pts, base, N, b, px, py, a);
#pragma unroll
            for (int u = 0; u < INFO_U; u++) t[u] = tex[texel_index(py[u], px[u], c.tiles_per_col)];
#pragma unroll
            for (int u = 0; u < INFO_U; u++) info_add(c, b[u], t[u], a);
        }
    }
    block_reduce<INFO_BLOCK, true>(a, red, tot);
    TrackerInfo &o = info[i];
    if (threadIdx.x < 21) o.H[threadIdx.x] = tot[threadIdx.x];
    else if (threadIdx.x < 27) o.g[threadIdx.x - 21] = tot[threadIdx.x];
    else if (threadIdx.x == 27) {
        o.sum_eps2 = acc_sum_eps2(tot);             /* slot 27, the sum as added, only if a residual was outside the limbs' range */
        o.n_visible = (int)tot[28];
        o.level = level;
    }
}

hipError_t launch_tracker_information(const TrackerEntry *list, const TrackerOut *out, int switched, int count, const double *poses,
                                      const LevelSlab &L, int level, const Intrinsics &K, bool use_p4, TrackerInfo *info, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const size_t dyn = sizeof(float2) * DVO_PAL_MAX;
    const hipError_t e = hipFuncSetAttribute((const void *)tracker_information_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tracker_information_kernel, dim3(count), dim3(INFO_BLOCK), dyn, s, list, out, switched, poses, L, level, K,
                       use_p4 ? 1 : 0, info);
    return hipGetLastError();
}

}  // namespace dvo
