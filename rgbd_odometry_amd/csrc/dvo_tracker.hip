/*
 * dvo_tracker.hip -- the device half of the multi-stream tracker (include/dvo_amd.h, "many camera streams";
 * host side dvo_capi_tracker.cpp).
 *
 * After the first alignment of a step, ONE launch evaluates the key-frame rule of SolveDVO::loop for every listed stream
 * (SolveDVO.cpp:2129-2160, the adaptive exits as dvo_amd::SolveDVO::processFrame evaluates them) and gathers the stream's
 * pose, so that the host reads one array of TrackerOut per step instead of a level report, the finalEpsilons list and a
 * pose per stream.
 *
 * b_cap (processResidueHistogram, :1455-1462; oracle/tracker_oracle.py::laplacian_b) is a float32 sum in the LIST's order
 * followed by one division.  A float sum's rounding depends on its order, and no parallel order reproduces the sequential
 * one in general, so the sum IS sequential: one lane per stream adds the residues one after the other, in list order, in
 * float32 (-ffp-contract=off, no reassociation), then divides by (float)N with the IEEE division -- the same operations in
 * the same order as the host loop, hence the same float.  The packed alignment kernel keeps finalEpsilons in the order of
 * its compact (block-ordered) point list; the workgroup first scatters them into list order through `scratch` (cidx =
 * list index of each compact point, the permutation dvo_get_final_outputs applies).  The streams run side by side, one
 * workgroup each.
 */
#include "dvo_launch.h"

namespace dvo {

__global__ void __launch_bounds__(256)
tracker_signals_kernel(const TrackerEntry *__restrict__ list, const double *__restrict__ poses, const float *__restrict__ ratio,
                       int last_level, const int *__restrict__ n_points, const float *__restrict__ eps,
                       const unsigned *__restrict__ cidx, int eps_stride, int cidx_stride, float *__restrict__ scratch,
                       int scratch_stride, TrackerRule rule, TrackerOut *__restrict__ out) {
    const int i = blockIdx.x;
    const TrackerEntry e = list[i];
    const int p = e.stream;
    const int N = n_points[p];
    float b_cap = 0.0f;
    if (eps && N > 0) {
        const float *src = eps + (size_t)p * eps_stride;
        const float *ordered = src;
        if (cidx) {                                     /* compact (block) order -> list order */
            float *dst = scratch + (size_t)i * scratch_stride;
            const unsigned *ix = cidx + (size_t)p * cidx_stride;
            for (int j = threadIdx.x; j < N; j += blockDim.x) {
                const unsigned k = ix[j];
                if (k < (unsigned)N) dst[k] = src[j];
            }
            __syncthreads();                            /* workgroup-scope release / acquire: the scattered values are visible */
            ordered = dst;
        }
        if (threadIdx.x == 0) {
            float acc = 0.0f;                           /* b_cap += residi[i] in list order (:1455-1462) */
            for (int j = 0; j < N; j++) acc += ordered[j];
            b_cap = acc / (float)N;
        }
    }
    if (threadIdx.x != 0) return;
    const float r = ratio[p * DVO_LEVELS + last_level];
    bool signal = false;
    int reason = 0;
    if (rule.adaptive) {                                /* dvo_amd::SolveDVO::processFrame: later exits overwrite the reason */
        if (b_cap > rule.lap_thresh) { signal = true; reason = 2; }
        if (r < rule.ratio_thresh) { signal = true; reason = 3; }
        if (N < rule.min_points) { signal = true; reason = 4; }
    }
    if (e.flags & DVO_TRK_FORCED) { signal = true; reason = 5; }
    TrackerOut o;
    for (int k = 0; k < 12; k++) o.pose[k] = poses[(size_t)p * 12 + k];
    o.b_cap = b_cap;
    o.ratio = r;
    o.n_points = N;
    o.event = (signal && (e.flags & DVO_TRK_MAY_SWITCH)) ? reason : 0;
    out[i] = o;
}

/* points4_build_kernel (dvo_kernels.hip) for the pairs of an index list: workgroup b builds the 4-byte twin of pair map[b].y.  The
 * body is that kernel's, line for line -- kept here so that the alignment kernels' sources (whose hash the committed traffic
 * profiles carry, bench.py) stay as they are. */
__global__ void __launch_bounds__(256)
points4_build_list_kernel(const uint2 *__restrict__ cpts, const int *__restrict__ N, int pt_cap, int rows, unsigned *__restrict__ cpt4,
                          unsigned *__restrict__ chdr, int *__restrict__ pt4_ok, const int2 *__restrict__ map) {
    const int pair = map[blockIdx.x].y;
    const int n = N[pair];
    cpts += (size_t)pair * pt_cap; cpt4 += (size_t)pair * pt_cap; chdr += (size_t)pair * (pt_cap / 64);
    const unsigned nby = (unsigned)((rows + 15) >> 4);
    const float inv_nby = 1.0f / (float)nby, half_inv = 0.5f * inv_nby;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += 256) {
        const uint2 p = cpts[i], p0 = cpts[i & ~63];
        const unsigned xx = p.x & 0xffffu, yy = p.x >> 16;
        const unsigned L = (xx >> 4) * nby + (yy >> 4), L0 = ((p0.x & 0xffffu) >> 4) * nby + ((p0.x >> 16) >> 4);
        const float Z = __uint_as_float(p.y);
        const float dmm = rintf(Z * 1000.0f);
        const bool enc = (L >= L0) && (L - L0 <= 255u) && (L < (1u << 20)) && (dmm >= 0.0f) && (dmm <= 65535.0f);
        const unsigned w = enc ? ((xx & 15u) | ((yy & 15u) << 4) | ((unsigned)dmm << 8) | ((L - L0) << 24)) : 0u;
        float xf, yf, zf;
        pt4_decode(nby, inv_nby, half_inv, w, L0, xf, yf, zf);
        if (!enc || xf != (float)xx || yf != (float)yy || __float_as_uint(zf) != p.y) bad = true;
        cpt4[i] = w;
        if ((i & 63) == 0) chdr[i >> 6] = L0;
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) pt4_ok[pair] = (n > 0 && !any_bad) ? 1 : 0;
}
hipError_t launch_points4_build_list(const uint2 *cpts, const int *N, int pt_cap, int rows, unsigned *cpt4, unsigned *chdr, int *pt4_ok,
                                     const int2 *map, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(points4_build_list_kernel, dim3(count), dim3(256), 0, s, cpts, N, pt_cap, rows, cpt4, chdr, pt4_ok, map);
    return hipGetLastError();
}

__device__ inline void identity_pose(double *P) {
    for (int k = 0; k < 12; k++) P[k] = (k < 9 && k % 4 == 0) ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(64)
tracker_reset_kernel(const TrackerEntry *__restrict__ list, const TrackerOut *__restrict__ out, int count, double *__restrict__ poses) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (out && out[i].event < 2) return;
    identity_pose(poses + (size_t)list[i].stream * 12);
}

__global__ void __launch_bounds__(64)
tracker_gather_kernel(const TrackerEntry *__restrict__ list, int count, const double *__restrict__ poses, TrackerOut *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || out[i].event < 2) return;
    for (int k = 0; k < 12; k++) out[i].pose[k] = poses[(size_t)list[i].stream * 12 + k];
}

hipError_t launch_tracker_signals(const TrackerEntry *list, int count, const double *poses, const float *ratio, int last_level,
                                  const int *n_points, const float *eps, const unsigned *cidx, int eps_stride, int cidx_stride,
                                  float *scratch, int scratch_stride, TrackerRule rule, TrackerOut *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(tracker_signals_kernel, dim3(count), dim3(eps && cidx ? 256 : 64), 0, s, list, poses, ratio, last_level, n_points,
                       eps, cidx, eps_stride, cidx_stride, scratch, scratch_stride, rule, out);
    return hipGetLastError();
}

hipError_t launch_tracker_reset_switched(const TrackerEntry *list, const TrackerOut *out, int count, double *poses, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(tracker_reset_kernel, dim3((count + 63) / 64), dim3(64), 0, s, list, out, count, poses);
    return hipGetLastError();
}

hipError_t launch_tracker_reset_listed(const TrackerEntry *list, int count, double *poses, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(tracker_reset_kernel, dim3((count + 63) / 64), dim3(64), 0, s, list, (const TrackerOut *)nullptr, count, poses);
    return hipGetLastError();
}

hipError_t launch_tracker_gather_switched(const TrackerEntry *list, int count, const double *poses, TrackerOut *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(tracker_gather_kernel, dim3((count + 63) / 64), dim3(64), 0, s, list, count, poses, out);
    return hipGetLastError();
}

}  // namespace dvo
