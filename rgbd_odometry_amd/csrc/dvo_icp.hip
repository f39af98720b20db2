/*
 * dvo_icp.hip -- projective point-to-plane ICP against ray-cast model views (include/dvo_amd.h, "frame-to-model alignment").
 * dvo_icp.h is the definition; the kernels call its per-pixel function term() and its per-sweep function after_sweep() as they are.
 *
 * TWO launches per sweep, for every listed view at once, and nothing of a sweep is looked at by the host.
 *   The sweep kernel.  A workgroup owns kGroup = 4096 consecutive entries of one view's list -- four waves, or sixteen when the whole
 *   sweep is at most kWideSweepMost workgroups (profiles/icp: one VGA view is 22 % faster with sixteen, 256 views 20 % slower; the
 *   sums are the same bits, the tree being the same) --; a wave takes 64 consecutive entries at a time -- one coalesced run of the now depth at level 0 -- computes their terms in double and sums them in the
 *   definition's tree64 order, leaving one value per sum in LDS: 64 of them per workgroup.  Wave 0 then sums those 64 in tree64 order
 *   again (the tree's second round) and writes one partial per sum.  A list of at most 64 entries has a single round: its one value is
 *   written as it is.
 *   The solve kernel.  One workgroup per view sums the partials in the tree's third and fourth round (lists beyond 4096 and 2^18
 *   entries), and one thread runs after_sweep(): the 6 x 6 factorisation, the pose update, the view's state and, where the view ends,
 *   its pose and record.
 * A call with now normals (dvo_icp_align_gated) takes the GATED instantiation of the sweep kernel: the same kernel with the normal gate in
 * its term, one more 12-byte read per paired pixel.
 * A view that has stopped, or has converged at the sweep's level, is skipped by both kernels through its state: whole workgroups
 * leave at once.  No atomics, no workgroup waits on another; a kernel boundary stands between a sweep's partials and their sums.
 *
 * tree64 inside a wave is a reduce-scatter: 32 values per lane (the 28 sums, the count as a double -- a sum of zeros and ones, exact
 * in any order -- and three zeros); at lane bit B, lanes exchange half of the values they still hold and add, value by value, what the
 * definition adds at stride B: x[l] + x[l + B], in the upper partner as x[l + B] + x[l] -- the same bits, IEEE addition being
 * commutative.  31 exchanges and one fold instead of 32 x 6, and every one a register move: permlane swaps for the bits 32 and 16,
 * DPP for the rest (dvo_kernel_common.h).  Lane L ends with the total of value L >> 1.
 */
#include "dvo_launch.h"
#include "dvo_kernel_common.h"
#include "dvo_icp_launch.h"

namespace dvo {
using namespace dvo_icp;

/* what lane L ^ BIT holds in x; up: L has the bit set */
template <int BIT>
DVO_DEV double icp_partner(double x, bool up) {
    if constexpr (BIT == 32 || BIT == 16) {
        const long long b = __double_as_longlong(x);
        unsigned lo0, lo1, hi0, hi1;
        if constexpr (BIT == 32) {
            const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
            const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
            lo0 = lo[0]; lo1 = lo[1]; hi0 = hi[0]; hi1 = hi[1];
        } else {
            const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
            lo0 = lo[0]; lo1 = lo[1]; hi0 = hi[0]; hi1 = hi[1];
        }
        /* the first result holds the lower partner's value in both partners, the second the upper partner's (see xor32_sum) */
        return __longlong_as_double((long long)(((unsigned long long)(up ? hi0 : hi1) << 32) | (up ? lo0 : lo1)));
    } else if constexpr (BIT == 8 || BIT == 4) {
        return dpp_xor_row<BIT>(x);
    } else if constexpr (BIT == 2) {
        return dpp_quad<DVO_DPP_QUAD_XOR2>(x);
    } else {
        return dpp_quad<DVO_DPP_QUAD_XOR1>(x);
    }
}
template <int HALF, int BIT>
DVO_DEV void icp_scatter_step(double (&v)[kSlots], int lane) {
    const bool up = (lane & BIT) != 0;
#pragma unroll
    for (int j = 0; j < HALF; j++) {
        const double keep = up ? v[j + HALF] : v[j], send = up ? v[j] : v[j + HALF];
        v[j] = keep + icp_partner<BIT>(send, up);
    }
}
/* tree64 of the 32 values of every lane: lane L ends with the total of value L >> 1 in v[0].  The whole wave takes part */
DVO_DEV void icp_wave_tree64(double (&v)[kSlots], int lane) {
    static_assert(kSlots == 32, "five scatter steps and one fold");
    icp_scatter_step<16, 32>(v, lane);
    icp_scatter_step<8, 16>(v, lane);
    icp_scatter_step<4, 8>(v, lane);
    icp_scatter_step<2, 4>(v, lane);
    icp_scatter_step<1, 2>(v, lane);
    v[0] = v[0] + icp_partner<1>(v[0], (lane & 1) != 0);
}

/* GATED: the call has now normals and term_of() tests them; the ungated instantiations are the code they were without the gate */
template <int BLOCK, bool GATED>
__global__ __launch_bounds__(BLOCK) void icp_sweep_kernel(const DeviceView *__restrict__ views, double *__restrict__ partials, SweepConst c, int level,
                                                          int record_sweep, unsigned blocks_per_view, unsigned stride, int entries, int list_cols) {
    __shared__ double red[kSlots][64];
    const unsigned vi = blockIdx.x / blocks_per_view, b = blockIdx.x - vi * blocks_per_view;
    const DeviceView &DV = views[vi];
    if (record_sweep ? DV.state.stopped != 0 : !takes_part(DV.state, level)) return;
    const View V = DV.view;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = DV.state.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = DV.state.t[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int run = wave; run < 64; run += BLOCK / 64) {
        const int first = (int)b * kGroup + run * 64;
        double v[kSlots];
#pragma unroll
        for (int k = 0; k < kSlots; k++) v[k] = 0.0;
        if (first < entries) {                     /* the same for the whole wave */
            const int e = first + lane;
            if (e < entries) {
                const int j = e / list_cols, i = e - j * list_cols;
                if (term_of<GATED>(V, c, R, t, i << level, j << level, v)) v[kCountSlot] = 1.0;
            }
            icp_wave_tree64(v, lane);
        }
        if ((lane & 1) == 0) red[lane >> 1][run] = v[0];
    }
    __syncthreads();
    double *P = partials + (size_t)vi * kSlots * stride + b;
    if (entries > 64) {                            /* the second round */
        if (wave == 0) {
            double v[kSlots];
#pragma unroll
            for (int k = 0; k < kSlots; k++) v[k] = red[k][lane];
            icp_wave_tree64(v, lane);
            if ((lane & 1) == 0 && (lane >> 1) <= kCountSlot) P[(size_t)(lane >> 1) * stride] = v[0];
        }
    } else if (threadIdx.x <= kCountSlot) {
        P[(size_t)threadIdx.x * stride] = red[threadIdx.x][0];
    }
}

__global__ __launch_bounds__(kSolveBlock) void icp_solve_kernel(DeviceView *__restrict__ views, const double *__restrict__ partials,
                                                                DeviceResult *__restrict__ results, dvo_icp_params p, int level, int record_sweep,
                                                                unsigned blocks, unsigned stride, int entries) {
    __shared__ double red[kSlots][64];
    __shared__ double total[kSlots];
    const unsigned vi = blockIdx.x;
    State &state = views[vi].state;
    if (record_sweep ? state.stopped != 0 : !takes_part(state, level)) return;
    const double *P = partials + (size_t)vi * kSlots * stride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (entries <= kGroup) {                       /* one sweep workgroup: its partial is the sum */
        if (threadIdx.x <= kCountSlot) total[threadIdx.x] = P[(size_t)threadIdx.x * stride];
    } else {
        const unsigned groups = (blocks + 63) / 64;
        for (unsigned g = wave; g < 64; g += kSolveBlock / 64) {          /* the third round */
            double v[kSlots];
#pragma unroll
            for (int k = 0; k < kSlots; k++) v[k] = 0.0;
            if (g < groups) {
                const unsigned blk = g * 64 + lane;
                if (blk < blocks) {
#pragma unroll
                    for (int k = 0; k <= kCountSlot; k++) v[k] = P[(size_t)k * stride + blk];
                }
                icp_wave_tree64(v, lane);
            }
            if ((lane & 1) == 0) red[lane >> 1][g] = v[0];
        }
        __syncthreads();
        if (entries > 64 * kGroup) {               /* the fourth round */
            if (wave == 0) {
                double v[kSlots];
#pragma unroll
                for (int k = 0; k < kSlots; k++) v[k] = red[k][lane];
                icp_wave_tree64(v, lane);
                if ((lane & 1) == 0) total[lane >> 1] = v[0];
            }
        } else if (threadIdx.x <= kCountSlot) {
            total[threadIdx.x] = red[threadIdx.x][0];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sums[kSums];
        for (int k = 0; k < kSums; k++) sums[k] = total[k];
        State st = state;
        DeviceResult &out = results[vi];
        if (after_sweep(st, sums, (int)total[kCountSlot], p, level, record_sweep != 0, &out.record)) {
            for (int k = 0; k < 9; k++) out.pose12[k] = st.R[k];
            for (int k = 0; k < 3; k++) out.pose12[9 + k] = st.t[k];
        }
        state = st;
    }
}
}  // namespace dvo

namespace dvo_icp {

int launch_icp_sweep(const CallArgs &a, int level, bool record_sweep, void *stream) {
    if (!a.views || !a.partials || !a.results || a.count < 1 || level < 0 || level >= kMaxLevels || !shape_ok(a.c.rows, a.c.cols))
        return (int)hipErrorInvalidValue;
    const int entries = level_entries(a.c.rows, a.c.cols, level), list_cols = level_cols(a.c.cols, level);
    const unsigned blocks = sweep_blocks(entries);
    if (blocks > a.stride || (unsigned long long)blocks * (unsigned long long)a.count > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const unsigned total = blocks * (unsigned)a.count;
    const bool wide = total <= kWideSweepMost;
    const dim3 block(wide ? kSweepBlockWide : kSweepBlock);
    const int record = record_sweep ? 1 : 0;
    if (wide && a.gated)
        hipLaunchKernelGGL((dvo::icp_sweep_kernel<kSweepBlockWide, true>), dim3(total), block, 0, (hipStream_t)stream, a.views, a.partials, a.c, level, record,
                           blocks, a.stride, entries, list_cols);
    else if (wide)
        hipLaunchKernelGGL((dvo::icp_sweep_kernel<kSweepBlockWide, false>), dim3(total), block, 0, (hipStream_t)stream, a.views, a.partials, a.c, level, record,
                           blocks, a.stride, entries, list_cols);
    else if (a.gated)
        hipLaunchKernelGGL((dvo::icp_sweep_kernel<kSweepBlock, true>), dim3(total), block, 0, (hipStream_t)stream, a.views, a.partials, a.c, level, record,
                           blocks, a.stride, entries, list_cols);
    else
        hipLaunchKernelGGL((dvo::icp_sweep_kernel<kSweepBlock, false>), dim3(total), block, 0, (hipStream_t)stream, a.views, a.partials, a.c, level, record,
                           blocks, a.stride, entries, list_cols);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::icp_solve_kernel, dim3((unsigned)a.count), dim3(kSolveBlock), 0, (hipStream_t)stream, a.views, a.partials, a.results, a.p, level,
                       record_sweep ? 1 : 0, blocks, a.stride, entries);
    return (int)hipGetLastError();
}

}  // namespace dvo_icp
