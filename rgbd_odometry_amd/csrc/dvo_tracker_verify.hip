/*
 * dvo_tracker_verify.hip -- depth verification of loop-closure candidates of the multi-stream tracker (include/dvo_amd.h:
 * dvo_tracker_verify; host side dvo_capi_tracker_archive.cpp).
 *
 * Score and match measure a candidate on the edge distance transform, the signal the alignment minimised.  This kernel measures it on
 * the one the alignment never looks at: the DEPTH of the stream's current frame.  An archived key-frame point warped into the current
 * camera has a predicted depth p2; the frame store holds the measured depth at the pixel it lands on (float millimetres, column-major).
 * A point agrees when the two are within tol = tol_mm + tol_rel * d; it is a free-space violation (`front`) when it lies in front of the
 * measured surface by more than tol, an occlusion (`behind`, neutral) when it lies behind it.
 *
 *   archive_verify_kernel  ONE launch, one 512-thread workgroup per candidate, as archive_score_kernel: it reads the slot's compact list
 *                          of one level where it is, with the slot's camera model, and ONE 4-byte gather per point from the depth plane
 *                          of the frame-store slot that holds the stream's current frame.  INFO_U points per lane are in flight; their
 *                          gathers are issued before any classification.
 *
 * The record is integers only (counts from wave ballots, sum |r| in 1/16 mm as a 64-bit integer): every field has ONE value, whatever
 * the order of the reduction, the number of candidates or their order -- the tests compare with a numpy restatement for equality.
 *
 * project_point returns zn = p2 * (1 / p2) (1 or 1 - 2^-24), not the depth: its three warp lines are restated below, in its own order of
 * operations, to get p2.
 *
 * Every index is bounded by the capacities the host passes: a count read from the device is clamped to the slab it indexes, a visible
 * point's pixel lies inside rows x cols <= npx by the half-open visibility rule, every other lane reads index 0.
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_tracker_info.h"

namespace dvo {

namespace {

DVO_DEV int clamp_count(int N, int cap_a, int cap_b) {
    const int cap = cap_a < cap_b ? cap_a : cap_b;
    return N < 0 ? 0 : (N > cap ? cap : N);
}

/* restated from project_point (dvo_device_math.h): the third row of cR^T * (_3d - cT), the depth of the warped point in metres */
DVO_DEV float warped_depth(const IterConst &c, float X, float Y, float Z) {
    const float d0 = X - c.t[0], d1 = Y - c.t[1], d2 = Z - c.t[2];
    return (c.r[6] * d0 + c.r[7] * d1) + c.r[8] * d2;
}

constexpr int VERIFY_COUNTS = 5;      /* visible, depth, agree, front, behind */

}  // namespace

__global__ void __launch_bounds__(INFO_BLOCK)
archive_verify_kernel(const VerifyCand *__restrict__ cands, const double *__restrict__ poses, ArchiveView A, VerifyDepth D, int level,
                      Intrinsics K, VerifyTol T, VerifyRecord *__restrict__ out) {
    __shared__ int red_n[INFO_BLOCK / 64][VERIFY_COUNTS];
    __shared__ unsigned long long red_q[INFO_BLOCK / 64];
    const int i = blockIdx.x;
    const int slot = __builtin_amdgcn_readfirstlane(cands[i].slot);
    const int fs = __builtin_amdgcn_readfirstlane(cands[i].frame_slot);
    const int pi = __builtin_amdgcn_readfirstlane(cands[i].pose_idx);
    const bool in_range = slot >= 0 && slot < A.n_slots && fs >= 0 && fs < D.n_slots && (size_t)D.rows * (size_t)D.cols <= D.npx;
    const ArchiveLevel &R = A.l[level];
    const ArchiveHeader &h = A.hdr[in_range ? slot : 0];
    const int N = __builtin_amdgcn_readfirstlane(in_range ? clamp_count(h.N[level], R.cap, R.cap) : 0);
    const uint2 *__restrict__ pts = R.cpts + (size_t)(in_range ? slot : 0) * R.cap;
    const float *__restrict__ depth = D.depth + (size_t)(in_range ? fs : 0) * D.npx;

    /* the slot's camera model: the host refuses a candidate whose stream has another one */
    Intrinsics Kc = K;
    const float4 k4 = h.K;
    Kc.fx = uniform_f(k4.x); Kc.fy = uniform_f(k4.y); Kc.cx = uniform_f(k4.z); Kc.cy = uniform_f(k4.w);
    Kc.pair_K = nullptr;
    IterConst c;
    level_consts(c, Kc, level, D.rows, D.cols);
    info_set_pose(c, poses + (size_t)pi * 12);

    /* wave-uniform counts (ballots: the trip count is the workgroup's), one 64-bit sum per lane */
    int n_vis = 0, n_depth = 0, n_agree = 0, n_front = 0, n_behind = 0;
    unsigned long long q_sum = 0;
    for (int base = 0; base < N; base += INFO_U * INFO_BLOCK) {
        float p2[INFO_U], d[INFO_U];
        bool vis[INFO_U];
        int idx[INFO_U];
#pragma unroll
        for (int u = 0; u < INFO_U; u++) {
            const int j = base + u * INFO_BLOCK + (int)threadIdx.x;
            const bool valid = j < N;
            const uint2 v = pts[valid ? j : (N - 1)];
            float X, Y, Z, xn, yn, zn, uu, vv;
            expand_compact(c, v.x, __uint_as_float(v.y), X, Y, Z);
            vis[u] = project_point(c, X, Y, Z, xn, yn, zn, uu, vv) && valid;
            p2[u] = warped_depth(c, X, Y, Z);
            const int px = vis[u] ? (int)uu : 0, py = vis[u] ? (int)vv : 0;      /* == floor for u, v >= 0 */
            idx[u] = px * D.rows + py;                                           /* < rows * cols: 0 <= px < cols, 0 <= py < rows */
        }
#pragma unroll
        for (int u = 0; u < INFO_U; u++) d[u] = depth[idx[u]];                   /* a lane without a visible point reads pixel 0 */
#pragma unroll
        for (int u = 0; u < INFO_U; u++) {
            const bool has = vis[u] && d[u] > T.min_depth_mm && d[u] <= T.max_depth_mm;      /* false for NaN */
            const float z_mm = p2[u] * 1000.0f;
            const float r = z_mm - d[u];
            const float tol = T.tol_mm + T.tol_rel * d[u];
            const bool agree = has && fabsf(r) <= tol;
            const bool front = has && r < -tol;
            const bool behind = has && r > tol;
            n_vis += __popcll(__ballot(vis[u]));
            n_depth += __popcll(__ballot(has));
            n_agree += __popcll(__ballot(agree));
            n_front += __popcll(__ballot(front));
            n_behind += __popcll(__ballot(behind));
            if (agree) q_sum += (unsigned long long)(unsigned)(fminf(fabsf(r), 65535.0f) * 16.0f);
        }
    }
    /* lanes, then the waves in wave order */
    for (int o = 32; o > 0; o >>= 1) q_sum += (unsigned long long)__shfl_xor((long long)q_sum, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_n[wave][0] = n_vis; red_n[wave][1] = n_depth; red_n[wave][2] = n_agree; red_n[wave][3] = n_front; red_n[wave][4] = n_behind;
        red_q[wave] = q_sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot[VERIFY_COUNTS] = {0, 0, 0, 0, 0};
        unsigned long long q = 0;
        for (int w = 0; w < INFO_BLOCK / 64; w++) {
            for (int k = 0; k < VERIFY_COUNTS; k++) tot[k] += red_n[w][k];
            q += red_q[w];
        }
        VerifyRecord &o = out[i];
        o.n_points = N; o.n_visible = tot[0]; o.n_depth = tot[1]; o.n_agree = tot[2]; o.n_front = tot[3]; o.n_behind = tot[4];
        o.sum_abs_q4 = q;
    }
}

hipError_t launch_archive_verify(const VerifyCand *cands, int count, const double *poses, const ArchiveView &A, const VerifyDepth &D, int level,
                                 const Intrinsics &K, const VerifyTol &T, VerifyRecord *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_verify_kernel, dim3(count), dim3(INFO_BLOCK), 0, s, cands, poses, A, D, level, K, T, out);
    return hipGetLastError();
}

}  // namespace dvo
