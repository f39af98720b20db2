/*
 * dvo_tsdf_map.hip -- depth fusion into TSDF volumes (include/dvo_amd.h, "depth fusion"): the integrate kernel and the three extract
 * kernels.  dvo_tsdf_map.h is the definition; the kernels call its per-voxel functions update() and crossing() as they are.
 *
 * INTEGRATE, one launch per call.  A thread owns one aligned 16-byte group of the pool -- kRun consecutive words, a run of consecutive
 * x voxels that wraps into the next row where nx is no multiple of 4 -- loads it once, applies every frame of its volume in list order
 * in registers, and stores it once if a word changed: the volume crosses HBM once per call, not once per frame.  Volumes sit back to back
 * in the pool, so a volume's first and last group may be shared with a neighbour: there the thread touches only its own words, one by
 * one.  The volume and frame records are the same for a whole workgroup and are read through uniform indices (scalar loads).  Every word
 * is one thread's: no atomics, no workgroup waits on another, and the result is bit-identical under any schedule.
 * No brick is rejected against a frustum: every voxel runs the definition's own tests.
 * With colour (dvo_tsdf_colour.h; a kernel of its own from the same body, so the plain kernel keeps its code) the thread also owns the
 * four colour words of its voxels, 32 bytes of the colour pool in two 16-byte accesses, loads them with the group, runs update_colour()
 * in place of update(), and stores each 16-byte half that changed; in a shared group it touches its own colour words one by one.
 *
 * EXTRACT, three launches over the tile walk of dvo_tsdf_walk.h.  Count: the crossings of the tile.  Scan: one workgroup turns the counts
 * into offsets and writes the total (the walk's scan).  Write: the same walk again; a voxel's points are the bits
 * of its axis mask, placed in the definition's order.
 */
#include "dvo_launch.h"
#include "dvo_tsdf_walk.h"

namespace dvo {
using namespace dvo_tsdf;

/* the volume of workgroup `blk`: the last one whose block_first <= blk (block_first ascends) */
__device__ __forceinline__ int volume_of_block(const DeviceVolume *__restrict__ vols, int n_vols, unsigned blk) {
    int lo = 0, hi = n_vols - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (vols[mid].block_first <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool COLOUR>
__device__ __forceinline__ void tsdf_integrate_body(unsigned *__restrict__ pool, unsigned long long *__restrict__ cpool,
                                                    const DeviceVolume *__restrict__ vols, int n_vols, const Frame *__restrict__ frames,
                                                    const void *const *__restrict__ images, int image_format, const FrameConst &fc) {
    const int vi = __builtin_amdgcn_readfirstlane(volume_of_block(vols, n_vols, blockIdx.x));
    const DeviceVolume &V = vols[vi];
    const VolumeConst vc = V.vc;
    const long long off = V.off, n = V.n;
    /* the group's first word in the pool, and the voxel index that word would have (negative in a first group shared with a neighbour) */
    const long long p0 = (off / kRun + ((long long)(blockIdx.x - V.block_first) * kBlock + threadIdx.x)) * kRun;
    const long long i0 = p0 - off;
    if (i0 >= n) return;
    const bool whole = i0 >= 0 && i0 + kRun <= n;
    unsigned word[kRun], before[kRun];
    bool own[kRun];
    double wx[kRun], wy[kRun], wz[kRun];
    if (whole) {
        const uint4 q = *reinterpret_cast<const uint4 *>(pool + p0);
        word[0] = q.x; word[1] = q.y; word[2] = q.z; word[3] = q.w;
    }
    unsigned long long cw[kRun], cbefore[kRun];
    if constexpr (COLOUR) {
        if (whole) {
            const ulonglong2 lo = *reinterpret_cast<const ulonglong2 *>(cpool + p0), hi = *reinterpret_cast<const ulonglong2 *>(cpool + p0 + 2);
            cw[0] = lo.x; cw[1] = lo.y; cw[2] = hi.x; cw[3] = hi.y;
        }
    }
    /* (x, y, z) of the group's first voxel of this volume by division (n <= 2^30), of the others by stepping the INDEX; every position
     * is then the direct formula of its own index */
    int x, y, z;
    walk_xyz(vc, i0 < 0 ? 0u : (unsigned)i0, x, y, z);
    bool wrapped = false;
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        const long long i = i0 + k;
        own[k] = i >= 0 && i < n;
        if (!whole) word[k] = own[k] ? pool[p0 + k] : 0u;
        before[k] = word[k];
        if constexpr (COLOUR) {
            if (!whole) cw[k] = own[k] ? cpool[p0 + k] : 0ull;
            cbefore[k] = cw[k];
        }
        if (k > 0 && i > 0 && ++x == vc.nx) {
            x = 0; wrapped = true;
            if (++y == vc.ny) { y = 0; z++; }
        }
        wx[k] = centre(vc.origin[0], vc.voxel_size, x);
        wy[k] = centre(vc.origin[1], vc.voxel_size, y);
        wz[k] = centre(vc.origin[2], vc.voxel_size, z);
    }
    /* a whole group inside one row -- every group when nx is a multiple of 4 and the volume starts on a 16-byte boundary -- hands
     * update() the same wy and wz four times: the terms of X, Y, Z that depend on them alone are then computed once (the same values
     * in the same order, so the same bits) */
    const bool one_row = whole && !wrapped;
    for (int j = 0; j < V.frame_count; j++) {
        const Frame &f = frames[V.frame_first + j];
        if constexpr (COLOUR) {
            const void *image = images[V.frame_first + j];
            if (one_row) {
#pragma unroll
                for (int k = 0; k < kRun; k++) word[k] = update_colour(word[k], &cw[k], wx[k], wy[0], wz[0], vc, f, image, image_format, fc);
            } else {
#pragma unroll
                for (int k = 0; k < kRun; k++)
                    if (own[k]) word[k] = update_colour(word[k], &cw[k], wx[k], wy[k], wz[k], vc, f, image, image_format, fc);
            }
        } else if (one_row) {
#pragma unroll
            for (int k = 0; k < kRun; k++) word[k] = update(word[k], wx[k], wy[0], wz[0], vc, f, fc);
        } else {
#pragma unroll
            for (int k = 0; k < kRun; k++)
                if (own[k]) word[k] = update(word[k], wx[k], wy[k], wz[k], vc, f, fc);
        }
    }
    if constexpr (COLOUR) {
        if (whole) {
            if (cw[0] != cbefore[0] || cw[1] != cbefore[1]) *reinterpret_cast<ulonglong2 *>(cpool + p0) = make_ulonglong2(cw[0], cw[1]);
            if (cw[2] != cbefore[2] || cw[3] != cbefore[3]) *reinterpret_cast<ulonglong2 *>(cpool + p0 + 2) = make_ulonglong2(cw[2], cw[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kRun; k++)
                if (own[k] && cw[k] != cbefore[k]) cpool[p0 + k] = cw[k];
        }
    }
    if (whole) {
        if (word[0] != before[0] || word[1] != before[1] || word[2] != before[2] || word[3] != before[3])
            *reinterpret_cast<uint4 *>(pool + p0) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kRun; k++)
            if (own[k] && word[k] != before[k]) pool[p0 + k] = word[k];
    }
}

__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(unsigned *__restrict__ pool, const DeviceVolume *__restrict__ vols, int n_vols,
                                                                const Frame *__restrict__ frames, FrameConst fc) {
    tsdf_integrate_body<false>(pool, nullptr, vols, n_vols, frames, nullptr, 0, fc);
}
__global__ __launch_bounds__(kBlock) void tsdf_integrate_colour_kernel(unsigned *__restrict__ pool, unsigned long long *__restrict__ cpool,
                                                                       const DeviceVolume *__restrict__ vols, int n_vols,
                                                                       const Frame *__restrict__ frames, const void *const *__restrict__ images,
                                                                       int image_format, FrameConst fc) {
    tsdf_integrate_body<true>(pool, cpool, vols, n_vols, frames, images, image_format, fc);
}

/* the crossings of voxel a with its neighbours along x, y, z: bit `axis` of the result, the points in pts[axis] */
__device__ __forceinline__ unsigned voxel_crossings(const unsigned *__restrict__ words, const VolumeConst &vc, long long n, long long a, int min_weight,
                                                    float pts[3][3]) {
    if (a >= n) return 0u;
    int x, y, z;
    walk_xyz(vc, (unsigned)a, x, y, z);
    const unsigned wa = words[a];
    if (word_w(wa) < min_weight) return 0u;
    const double cx = centre(vc.origin[0], vc.voxel_size, x), cy = centre(vc.origin[1], vc.voxel_size, y), cz = centre(vc.origin[2], vc.voxel_size, z);
    unsigned mask = 0u;
    if (x + 1 < vc.nx && crossing(wa, words[a + 1], min_weight, 0, cx, cy, cz, vc.voxel_size, pts[0])) mask |= 1u;
    if (y + 1 < vc.ny && crossing(wa, words[a + (long long)axis_step(vc, 1)], min_weight, 1, cx, cy, cz, vc.voxel_size, pts[1])) mask |= 2u;
    if (z + 1 < vc.nz && crossing(wa, words[a + (long long)axis_step(vc, 2)], min_weight, 2, cx, cy, cz, vc.voxel_size, pts[2])) mask |= 4u;
    return mask;
}

__global__ __launch_bounds__(kBlock) void tsdf_extract_count_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                    unsigned long long *__restrict__ counts) {
    const long long base = walk_base();
    unsigned mine = 0;
    float pts[3][3];
    for (int pass = 0; pass < kExtractPasses; pass++) mine += __popc(voxel_crossings(words, vc, n, walk_voxel(base, pass), min_weight, pts));
    const unsigned *wave_sum = walk_wave_sums(mine);
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < kWalkWaves; w++) t += wave_sum[w];
        counts[blockIdx.x] = t;
    }
}

/* one workgroup: the walk's scan; out's first 16 bytes = {the total, 0} */
__global__ __launch_bounds__(kBlock) void tsdf_extract_scan_kernel(unsigned long long *__restrict__ counts, unsigned nb, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[kBlock];
    walk_scan(counts, nb, part, total);
    if (threadIdx.x == 0) total[1] = 0;
}

__global__ __launch_bounds__(kBlock) void tsdf_extract_write_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                    const unsigned long long *__restrict__ counts, float *__restrict__ xyz,
                                                                    long long capacity) {
    const long long base = walk_base();
    unsigned long long at = counts[blockIdx.x];
    if (at >= (unsigned long long)capacity) return;      /* the same for the whole workgroup: everything from here on is beyond the buffer */
    for (int pass = 0; pass < kExtractPasses; pass++) {
        float pts[3][3];
        const unsigned mask = voxel_crossings(words, vc, n, walk_voxel(base, pass), min_weight, pts);
        unsigned in_wave;
        const unsigned before = walk_before_mask<3>(mask, in_wave);
        unsigned long long o = walk_place(at, before, in_wave);
        for (int axis = 0; axis < 3; axis++)
            if (mask & (1u << axis)) {
                if (o < (unsigned long long)capacity) { xyz[3 * o] = pts[axis][0]; xyz[3 * o + 1] = pts[axis][1]; xyz[3 * o + 2] = pts[axis][2]; }
                o++;
            }
    }
}
}  // namespace dvo

namespace dvo_tsdf {

int launch_tsdf_integrate(unsigned *pool, const DeviceVolume *vols, int n_vols, const Frame *frames, const FrameConst &fc, unsigned total_blocks,
                          void *stream) {
    if (!pool || !vols || !frames || n_vols < 1 || total_blocks < 1 || total_blocks > 0x7FFFFFFFu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::tsdf_integrate_kernel, dim3(total_blocks), dim3(kBlock), 0, (hipStream_t)stream, pool, vols, n_vols, frames, fc);
    return (int)hipGetLastError();
}

int launch_tsdf_integrate_colour(unsigned *pool, unsigned long long *colours, const DeviceVolume *vols, int n_vols, const Frame *frames,
                                 const void *const *images, int image_format, const FrameConst &fc, unsigned total_blocks, void *stream) {
    if (!pool || !colours || !vols || !frames || !images || !image_format_ok(image_format) || n_vols < 1 || total_blocks < 1 ||
        total_blocks > 0x7FFFFFFFu)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::tsdf_integrate_colour_kernel, dim3(total_blocks), dim3(kBlock), 0, (hipStream_t)stream, pool, colours, vols, n_vols, frames,
                       images, image_format, fc);
    return (int)hipGetLastError();
}

int launch_tsdf_extract(const unsigned *words, const VolumeConst &vc, int min_weight, unsigned long long *counts, unsigned char *out,
                        long long capacity, void *stream) {
    if (!words || !counts || !out || capacity < 0 || min_weight < 1) return (int)hipErrorInvalidValue;
    const long long n = (long long)vc.nx * vc.ny * vc.nz;
    const unsigned nb = extract_blocks(n);
    hipLaunchKernelGGL(dvo::tsdf_extract_count_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, vc, n, min_weight, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::tsdf_extract_scan_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, counts, nb, reinterpret_cast<unsigned long long *>(out));
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::tsdf_extract_write_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, vc, n, min_weight, counts,
                       reinterpret_cast<float *>(out + 16), capacity);
    return (int)hipGetLastError();
}

}  // namespace dvo_tsdf
