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
 * The walk itself lives in dvo_tracker_info.h, shared with the scoring of archived key frames (dvo_tracker_archive.hip).
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_tracker_info.h"

namespace dvo {

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
    info_set_pose(c, poses + (size_t)p * 12);

    Acc a;
    acc_zero(a);
    info_accumulate(c, pts, N, L, p, use_p4, pal_lds, a);
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
