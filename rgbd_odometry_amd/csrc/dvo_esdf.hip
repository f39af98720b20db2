/*
 * dvo_esdf.hip -- Euclidean signed distance fields of fused volumes (include/dvo_amd.h, "distance fields"): the three kernels of an
 * update, the conversion to metres and the point query.  dvo_esdf.h is the definition; the kernels call its esdf_flags(), esdf_scan(),
 * esdf_metres() and esdf_query_point() as they are.  d2 is an integer minimum: the result has no order, so it is byte-equal to the host
 * whatever the schedule.
 *
 * PASS X, fused with the classification (TSDF pool -> ESDF pool).  A wave owns one x-row and walks it in chunks of 64 voxels, a lane per
 * voxel: the TSDF word and its six neighbours are read (the row itself coalesced, the rows at y +- 1 and z +- 1 from the cache), the
 * site flags of a chunk are one 64-bit ballot kept in scalar registers -- at most sixteen per row -- and the nearest site to the left and
 * to the right of a voxel is a count of leading or trailing zeros over those words.  It writes dx^2 plus the two flag bits.
 * PASSES Y and Z (ESDF pool -> scratch -> ESDF pool).  The min-plus transform along a strided axis; lanes sit on consecutive x, so every
 * access of a wave is one contiguous run, and each output scans outwards with the definition's exact stopping radius.  A pass's outputs
 * are other threads' inputs, so the passes ping-pong between the pool and a scratch block and none runs in place.
 * No atomics, no LDS, no workgroup waits on another.
 */
#include "dvo_launch.h"
#include "dvo_esdf_launch.h"

namespace dvo {
using namespace dvo_tsdf;

/* the volume of workgroup `blk` of pass `pass`: the last one whose first[pass] <= blk (first[] ascends) */
__device__ __forceinline__ int esdf_volume_of_block(const EsdfVolume *__restrict__ vols, int n_vols, int pass, unsigned blk) {
    int lo = 0, hi = n_vols - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (vols[mid].first[pass] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kEsdfBlock) void esdf_pass_x_kernel(const unsigned *__restrict__ pool, unsigned *__restrict__ esdf,
                                                                 const EsdfVolume *__restrict__ vols, int n_vols, int min_weight, int sites) {
    const int vi = __builtin_amdgcn_readfirstlane(esdf_volume_of_block(vols, n_vols, 0, blockIdx.x));
    const EsdfVolume &V = vols[vi];
    const int nx = V.nx, ny = V.ny, nz = V.nz;
    const int lane = threadIdx.x & 63;
    const long long row = (long long)(blockIdx.x - V.first[0]) * kEsdfWaves + (threadIdx.x >> 6);
    if (row >= (long long)ny * nz) return;         /* the same for a whole wave */
    const int y = (int)(row % ny), z = (int)(row / ny);
    const unsigned *words = pool + V.off;
    unsigned *out = esdf + V.off + row * nx;
    /* the row's site flags, a ballot per chunk, and every lane's flag bits of its voxel in each chunk */
    unsigned long long mask[kEsdfRowChunks];
    unsigned flags[kEsdfRowChunks];
#pragma unroll
    for (int c = 0; c < kEsdfRowChunks; c++) {
        mask[c] = 0ull; flags[c] = 0u;
        if (c * kEsdfRowChunk < nx) {
            const int x = c * kEsdfRowChunk + lane;
            bool site = false;
            if (x < nx) flags[c] = esdf_flags(words, nx, ny, nz, x, y, z, min_weight, sites, &site);
            mask[c] = __ballot(site);
        }
    }
#pragma unroll
    for (int c = 0; c < kEsdfRowChunks; c++) {
        if (c * kEsdfRowChunk >= nx) break;
        const int x = c * kEsdfRowChunk + lane;
        int best = 0x7FFFFFFF;                     /* |x - the nearest site| */
#pragma unroll
        for (int s = 0; s < kEsdfRowChunks; s++) {
            if (s * kEsdfRowChunk >= nx) break;
            /* the sites of chunk s at or left of x, and at or right of it */
            const unsigned long long upto = 2ull << lane, from = 1ull << lane;
            const unsigned long long left = s < c ? mask[s] : s == c ? mask[s] & (upto - 1ull) : 0ull;
            const unsigned long long right = s > c ? mask[s] : s == c ? mask[s] & ~(from - 1ull) : 0ull;
            if (left) best = min(best, x - (s * kEsdfRowChunk + 63 - __clzll((long long)left)));
            if (right) best = min(best, s * kEsdfRowChunk + (__ffsll((long long)right) - 1) - x);
        }
        if (x < nx) out[x] = flags[c] | (best == 0x7FFFFFFF ? kEsdfNoSite : (unsigned)(best * best));
    }
}

/* pass y (AXIS 1) or z (AXIS 2): src -> dst, both laid out like the volume */
template <int AXIS>
__global__ __launch_bounds__(kEsdfBlock) void esdf_pass_axis_kernel(const unsigned *__restrict__ src_pool, unsigned *__restrict__ dst_pool,
                                                                    const EsdfVolume *__restrict__ vols, int n_vols, bool src_is_scratch) {
    const int vi = __builtin_amdgcn_readfirstlane(esdf_volume_of_block(vols, n_vols, AXIS, blockIdx.x));
    const EsdfVolume &V = vols[vi];
    const int nx = V.nx, ny = V.ny, nz = V.nz;
    const int n = AXIS == 1 ? ny : nz, others = AXIS == 1 ? nz : ny;
    const unsigned chunks = (unsigned)esdf_x_chunks(nx), tiles = (unsigned)esdf_tiles(n);
    const unsigned local = blockIdx.x - V.first[AXIS];
    const unsigned xc = local % chunks, rest = local / chunks, tile = rest % tiles, other = rest / tiles;
    if (other >= (unsigned)others) return;
    const int x = (int)xc * kEsdfRowChunk + (int)(threadIdx.x & 63);
    if (x >= nx) return;
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny;
    const size_t stride = AXIS == 1 ? sy : sz, line = (size_t)x + (AXIS == 1 ? sz : sy) * (size_t)other;
    const unsigned *src = src_pool + (src_is_scratch ? V.scratch_off : V.off) + line;
    unsigned *dst = dst_pool + (src_is_scratch ? V.off : V.scratch_off) + line;
    constexpr int kPerWave = kEsdfColumnTile / kEsdfWaves;
    const int i0 = (int)tile * kEsdfColumnTile + (int)(threadIdx.x >> 6) * kPerWave;
    for (int k = 0; k < kPerWave; k++) {
        const int i = i0 + k;
        if (i >= n) break;
        dst[(size_t)i * stride] = (src[(size_t)i * stride] & ~kEsdfD2Mask) | esdf_scan(src, stride, n, i);
    }
}

__global__ __launch_bounds__(kEsdfBlock) void esdf_distances_kernel(const unsigned *__restrict__ words, long long count, double voxel_size,
                                                                    float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kEsdfBlock + threadIdx.x;
    if (i < count) out[i] = esdf_metres(words[i], voxel_size);
}

__global__ __launch_bounds__(kEsdfBlock) void esdf_query_kernel(const unsigned *__restrict__ words, VolumeConst vc, int count,
                                                                const double *__restrict__ xyz, dvo_esdf_sample *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kEsdfBlock + threadIdx.x;
    if (i < count) out[i] = esdf_query_point(vc, words, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}
}  // namespace dvo

namespace dvo_tsdf {

int launch_esdf_update(const unsigned *pool, unsigned *esdf, unsigned *scratch, const EsdfVolume *vols, int n_vols, int min_weight, int sites,
                       const unsigned blocks[3], void *stream) {
    if (!pool || !esdf || !scratch || !vols || n_vols < 1 || min_weight < 1 || !blocks) return (int)hipErrorInvalidValue;
    for (int p = 0; p < 3; p++)
        if (blocks[p] < 1 || blocks[p] > 0x7FFFFFFFu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::esdf_pass_x_kernel, dim3(blocks[0]), dim3(kEsdfBlock), 0, (hipStream_t)stream, pool, esdf, vols, n_vols, min_weight, sites);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::esdf_pass_axis_kernel<1>, dim3(blocks[1]), dim3(kEsdfBlock), 0, (hipStream_t)stream, (const unsigned *)esdf, scratch, vols,
                       n_vols, false);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::esdf_pass_axis_kernel<2>, dim3(blocks[2]), dim3(kEsdfBlock), 0, (hipStream_t)stream, (const unsigned *)scratch, esdf, vols,
                       n_vols, true);
    return (int)hipGetLastError();
}

int launch_esdf_distances(const unsigned *words, long long count, double voxel_size, float *out, void *stream) {
    if (!words || !out || count < 1 || (count + kEsdfBlock - 1) / kEsdfBlock > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::esdf_distances_kernel, dim3((unsigned)((count + kEsdfBlock - 1) / kEsdfBlock)), dim3(kEsdfBlock), 0, (hipStream_t)stream, words,
                       count, voxel_size, out);
    return (int)hipGetLastError();
}

int launch_esdf_query(const unsigned *words, const VolumeConst &vc, int count, const double *xyz, dvo_esdf_sample *out, void *stream) {
    if (!words || !xyz || !out || count < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::esdf_query_kernel, dim3((unsigned)((count + kEsdfBlock - 1) / kEsdfBlock)), dim3(kEsdfBlock), 0, (hipStream_t)stream, words, vc,
                       count, xyz, out);
    return (int)hipGetLastError();
}

}  // namespace dvo_tsdf
