/*
 * dvo_tsdf_walk.h -- the ordered, atomic-free compaction of a voxel walk, once, for the kernels that extract something from a fused
 * volume (dvo_tsdf_map.hip: points; dvo_tsdf_mesh.hip: vertices and triangles).  Device code; internal, not installed.
 *
 * A workgroup of kBlock threads walks kExtractTile consecutive voxels in kExtractPasses passes of one voxel per thread, in three
 * launches.  COUNT: what the tile's voxels contribute (walk_wave_sums).  SCAN: one workgroup turns the tile counts into offsets
 * (walk_scan).  PLACE: the walk again; an item's place is the tile's offset + the passes before + the waves before (in wave
 * order, through LDS) + the lanes before (walk_before_mask or walk_before_count, then walk_place) -- the order of the voxel indices,
 * which is the definitions' order.  What a voxel contributes, when a tile may leave early and what is stored stay with each kernel.
 * No atomics, no workgroup waits on another: the result is bit-identical under any schedule.
 */
#ifndef DVO_TSDF_WALK_H_
#define DVO_TSDF_WALK_H_

#include "dvo_tsdf_launch.h"

namespace dvo {
constexpr int kWalkWaves = dvo_tsdf::kBlock / 64;
/* (x, y, z) of voxel index a (n <= 2^30: two 32-bit divisions) */
__device__ __forceinline__ void walk_xyz(const dvo_tsdf::VolumeConst &vc, unsigned a, int &x, int &y, int &z) {
    const unsigned row = a / (unsigned)vc.nx;
    x = (int)(a - row * (unsigned)vc.nx); z = (int)(row / (unsigned)vc.ny); y = (int)(row - (unsigned)z * (unsigned)vc.ny);
}
/* the first voxel of this workgroup's tile, and this thread's voxel in pass `pass` of it */
__device__ __forceinline__ long long walk_base() { return (long long)blockIdx.x * dvo_tsdf::kExtractTile; }
__device__ __forceinline__ long long walk_voxel(long long base, int pass) { return base + (long long)pass * dvo_tsdf::kBlock + threadIdx.x; }
/* COUNT: the sum of `mine` over each wave, in LDS behind a barrier; thread 0 of a count kernel adds the kWalkWaves sums up */
__device__ __forceinline__ const unsigned *walk_wave_sums(unsigned mine) {
    __shared__ unsigned wave_sum[kWalkWaves];
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_down(mine, s, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    return wave_sum;
}
/* SCAN, by one workgroup of a launch of its own: counts[0 .. nb) -> their exclusive prefix sums, counts[nb] = *total = the total.  A thread
 * sums its `per` consecutive counts into part[] (kBlock words of LDS; a barrier before it is used again), thread 0 scans those, the thread its own */
__device__ __forceinline__ void walk_scan(unsigned long long *__restrict__ counts, unsigned nb, unsigned long long *part, unsigned long long *__restrict__ total) {
    const unsigned kBlock = dvo_tsdf::kBlock, per = (nb + kBlock - 1) / kBlock;
    const unsigned lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    unsigned long long s = 0;
    for (unsigned i = lo; i < hi; i++) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (unsigned t = 0; t < kBlock; t++) { const unsigned long long c = part[t]; part[t] = run; run += c; }
        counts[nb] = run;
        *total = run;
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (unsigned i = lo; i < hi; i++) { const unsigned long long c = counts[i]; counts[i] = run; run += c; }
}
/* PLACE, the lanes before: the items of lower lanes of the wave, and in_wave = the whole wave's.  Either a thread's items are the
 * low NBITS bits of `mask` (ballot and popcount per bit) ... */
template <int NBITS>
__device__ __forceinline__ unsigned walk_before_mask(unsigned mask, unsigned &in_wave) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    unsigned before = in_wave = 0;
#pragma unroll
    for (int d = 0; d < NBITS; d++) {
        const unsigned long long b = __ballot(mask & (1u << d));
        before += (unsigned)__popcll(b & below);
        in_wave += (unsigned)__popcll(b);
    }
    return before;
}
/* ... or a thread has `mine` of them (inclusive scan over the wave) */
__device__ __forceinline__ unsigned walk_before_count(unsigned mine, unsigned &in_wave) {
    const int lane = threadIdx.x & 63;
    unsigned upto = mine;
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned other = __shfl_up(upto, s, 64);
        if (lane >= s) upto += other;
    }
    in_wave = (unsigned)__builtin_amdgcn_readlane((int)upto, 63);
    return upto - mine;
}
/* PLACE: the place of this thread's first item of the pass, `at` being the tile's running offset, which moves on by the pass's items.
 * Every thread of the workgroup calls it in every pass; wave_sum[] is free again when it returns */
__device__ __forceinline__ unsigned long long walk_place(unsigned long long &at, unsigned before, unsigned in_wave) {
    __shared__ unsigned wave_sum[kWalkWaves];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_sum[wave] = in_wave;
    __syncthreads();
    unsigned long long o = at + before;
    unsigned all = 0;
    for (int w = 0; w < kWalkWaves; w++) {
        if (w < wave) o += wave_sum[w];
        all += wave_sum[w];
    }
    __syncthreads();
    at += all;
    return o;
}
}  // namespace dvo
#endif
