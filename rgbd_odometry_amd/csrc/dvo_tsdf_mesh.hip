/*
 * dvo_tsdf_mesh.hip -- the triangle mesh of a fused volume (include/dvo_amd.h, "the surface as a triangle mesh"): four kernels.
 * dvo_tsdf_mesh.h is the definition; the kernels call its per-voxel and per-cell functions as they are.
 *
 * A workgroup walks kExtractTile consecutive voxels in kExtractPasses passes of one voxel per thread, as the point extraction does.
 * COUNT: per tile, the vertices its voxels own and the triangles of the cells its voxels are the first corner of.  SCAN: one workgroup
 * turns both count arrays into offsets and writes the two totals.  VERTICES: the walk again; a vertex's place is the tile's offset +
 * the passes before + the waves before (in wave order, through LDS) + the lanes before (ballot and popcount per direction d), which is
 * the definition's order; a voxel that owns a vertex also records the number of its first one and its 7-bit edge mask in the scratch.
 * TRIANGLES: the walk again, a launch of its own because it reads scratch that other workgroups wrote; a thread checks its cell, runs
 * the six tetrahedra through the definition's table and names each vertex through the scratch record of the corner voxel that owns the
 * edge; its triangles go to the tile's offset + an exclusive scan of the per-thread counts over the workgroup.
 *
 * A scratch record is read only for an edge that carries a vertex, and such an edge's owner writes its record in the same call: records
 * of voxels without a vertex are never written and never read, so what an earlier call left in the scratch does not matter.
 * No atomics, no workgroup waits on another: the result is bit-identical under any schedule.  A tile whose offset is already past the
 * caller's capacity leaves at once -- a vertices tile only when, in addition, no triangle tile that still writes can name its vertices.
 * A mesh of more than kMeshMaxVertices vertices writes nothing (the host refuses it from the counts).
 */
#include "dvo_launch.h"
#include "dvo_tsdf_launch.h"

namespace dvo {
using namespace dvo_tsdf;

/* the corner words of voxel a's cell; false: a is past the volume or its own weight is below min_weight (it owns no vertex and is the
 * first corner of no valid cell) */
__device__ __forceinline__ bool mesh_voxel(const unsigned *__restrict__ words, const VolumeConst &vc, long long n, long long a, int min_weight,
                                           unsigned w[8], int &x, int &y, int &z) {
    if (a >= n) return false;
    if (word_w(words[a]) < min_weight) return false;
    const unsigned ua = (unsigned)a, row = ua / (unsigned)vc.nx;
    x = (int)(ua - row * (unsigned)vc.nx); z = (int)(row / (unsigned)vc.ny); y = (int)(row - (unsigned)z * (unsigned)vc.ny);
    mesh_corner_words(words, vc, x, y, z, (size_t)a, w);
    return true;
}

/* counts of one voxel: vertices in the low 16 bits, triangles in the high ones (a tile has at most 7 * 2048 and 12 * 2048) */
__global__ __launch_bounds__(kBlock) void tsdf_mesh_count_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                 unsigned long long *__restrict__ vcounts, unsigned long long *__restrict__ tcounts) {
    __shared__ unsigned wave_sum[kBlock / 64];
    const long long base = (long long)blockIdx.x * kExtractTile;
    unsigned mine = 0;
    for (int pass = 0; pass < kExtractPasses; pass++) {
        unsigned w[8];
        int x, y, z;
        if (!mesh_voxel(words, vc, n, base + (long long)pass * kBlock + threadIdx.x, min_weight, w, x, y, z)) continue;
        const int inside8 = mesh_cell_inside(w, min_weight);
        mine += (unsigned)__popc(mesh_edge_mask(w, min_weight)) + ((unsigned)(inside8 < 0 ? 0 : mesh_cell_triangles(inside8)) << 16);
    }
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_down(mine, s, 64);      /* a wave: at most 7 * 512 and 12 * 512, no carry between the halves */
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned v = 0, t = 0;
        for (int k = 0; k < kBlock / 64; k++) { v += wave_sum[k] & 0xFFFFu; t += wave_sum[k] >> 16; }
        vcounts[blockIdx.x] = v;
        tcounts[blockIdx.x] = t;
    }
}

/* one workgroup: each of the two arrays counts[0 .. nb) -> its exclusive prefix sums, counts[nb] = the total; totals = {vertices, triangles} */
__global__ __launch_bounds__(kBlock) void tsdf_mesh_scan_kernel(unsigned long long *__restrict__ vcounts, unsigned long long *__restrict__ tcounts, unsigned nb,
                                                                unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long part[kBlock];
    const unsigned per = (nb + kBlock - 1) / kBlock;
    const unsigned lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    for (int which = 0; which < 2; which++) {
        unsigned long long *counts = which ? tcounts : vcounts;
        unsigned long long s = 0;
        for (unsigned i = lo; i < hi; i++) s += counts[i];
        part[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long run = 0;
            for (int t = 0; t < kBlock; t++) { const unsigned long long c = part[t]; part[t] = run; run += c; }
            counts[nb] = run;
            totals[which] = run;
        }
        __syncthreads();
        unsigned long long run = part[threadIdx.x];
        for (unsigned i = lo; i < hi; i++) { const unsigned long long c = counts[i]; counts[i] = run; run += c; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void tsdf_mesh_vertices_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                    const unsigned long long *__restrict__ vcounts,
                                                                    const unsigned long long *__restrict__ tcounts, MeshScratch scratch,
                                                                    float *__restrict__ xyz, long long vertex_capacity, long long triangle_capacity) {
    __shared__ unsigned wave_sum[kBlock / 64];
    if (vcounts[gridDim.x] > (unsigned long long)kMeshMaxVertices) return;
    const long long base = (long long)blockIdx.x * kExtractTile;
    unsigned long long at = vcounts[blockIdx.x];
    /* a cell names vertices of voxels up to nx ny + nx + 1 words ahead of it: the first triangle tile that can name this tile's */
    const long long reach = (long long)vc.nx * vc.ny + vc.nx + 1;
    const unsigned first_user = base > reach ? (unsigned)((base - reach) / kExtractTile) : 0u;
    /* the same for the whole workgroup: no vertex of this tile is inside the buffer, and no triangle that is written names one */
    if (at >= (unsigned long long)vertex_capacity && tcounts[first_user] >= (unsigned long long)triangle_capacity) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int pass = 0; pass < kExtractPasses; pass++) {
        const long long a = base + (long long)pass * kBlock + threadIdx.x;
        unsigned w[8];
        int x = 0, y = 0, z = 0;
        const unsigned mask = mesh_voxel(words, vc, n, a, min_weight, w, x, y, z) ? mesh_edge_mask(w, min_weight) : 0u;
        unsigned before = 0, in_wave = 0;
#pragma unroll
        for (int d = 0; d < kMeshEdges; d++) {
            const unsigned long long b = __ballot(mask & (1u << d));
            before += (unsigned)__popcll(b & below);
            in_wave += (unsigned)__popcll(b);
        }
        if (lane == 0) wave_sum[wave] = in_wave;
        __syncthreads();
        unsigned long long o = at + before;
        unsigned all = 0;
        for (int k = 0; k < kBlock / 64; k++) {
            if (k < wave) o += wave_sum[k];
            all += wave_sum[k];
        }
        if (mask) {
            mesh_scratch_store(scratch, a, (int)o, mask);
            const double cx = centre(vc.origin[0], vc.voxel_size, x), cy = centre(vc.origin[1], vc.voxel_size, y), cz = centre(vc.origin[2], vc.voxel_size, z);
#pragma unroll
            for (int d = 0; d < kMeshEdges; d++)
                if (mask & (1u << d)) {
                    if (o < (unsigned long long)vertex_capacity) {
                        float pt[3];
                        mesh_vertex(w[0], w[mesh_dir_corner(d)], d, cx, cy, cz, vc.voxel_size, pt);
                        xyz[3 * o] = pt[0]; xyz[3 * o + 1] = pt[1]; xyz[3 * o + 2] = pt[2];
                    }
                    o++;
                }
        }
        at += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void tsdf_mesh_triangles_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                     const unsigned long long *__restrict__ vcounts,
                                                                     const unsigned long long *__restrict__ tcounts, MeshScratch scratch,
                                                                     int *__restrict__ tri, long long triangle_capacity) {
    __shared__ unsigned wave_sum[kBlock / 64];
    if (vcounts[gridDim.x] > (unsigned long long)kMeshMaxVertices) return;
    const long long base = (long long)blockIdx.x * kExtractTile;
    unsigned long long at = tcounts[blockIdx.x];
    if (at >= (unsigned long long)triangle_capacity) return;      /* the same for the whole workgroup: everything from here on is beyond the buffer */
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int pass = 0; pass < kExtractPasses; pass++) {
        const long long a = base + (long long)pass * kBlock + threadIdx.x;
        unsigned w[8];
        int x, y, z;
        const int inside8 = mesh_voxel(words, vc, n, a, min_weight, w, x, y, z) ? mesh_cell_inside(w, min_weight) : -1;
        const unsigned mine = inside8 < 0 ? 0u : (unsigned)mesh_cell_triangles(inside8);
        unsigned upto = mine;                                       /* inclusive scan over the wave */
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned other = __shfl_up(upto, s, 64);
            if (lane >= s) upto += other;
        }
        if (lane == 63) wave_sum[wave] = upto;
        __syncthreads();
        unsigned long long o = at + (upto - mine);
        unsigned all = 0;
        for (int k = 0; k < kBlock / 64; k++) {
            if (k < wave) o += wave_sum[k];
            all += wave_sum[k];
        }
        if (mine)
            mesh_cell_emit(inside8,
                           [&](int corner, int d) { return mesh_scratch_vertex(scratch, a + (long long)mesh_corner_step(vc, corner), d); },
                           [&](int i0, int i1, int i2) {
                               if (o < (unsigned long long)triangle_capacity) { tri[3 * o] = i0; tri[3 * o + 1] = i1; tri[3 * o + 2] = i2; }
                               o++;
                           });
        at += all;
        __syncthreads();
    }
}
}  // namespace dvo

namespace dvo_tsdf {

int launch_tsdf_mesh(const unsigned *words, const VolumeConst &vc, int min_weight, unsigned long long *counts, const MeshScratch &scratch,
                     unsigned long long *totals, float *xyz, long long vertex_capacity, int *tri, long long triangle_capacity, void *stream) {
    if (!words || !counts || !mesh_scratch_ok(scratch) || !totals || vertex_capacity < 0 || triangle_capacity < 0 || min_weight < 1 ||
        (vertex_capacity > 0 && !xyz) || (triangle_capacity > 0 && !tri))
        return (int)hipErrorInvalidValue;
    const long long n = (long long)vc.nx * vc.ny * vc.nz;
    const unsigned nb = extract_blocks(n);
    unsigned long long *vcounts = counts, *tcounts = counts + nb + 1;
    hipLaunchKernelGGL(dvo::tsdf_mesh_count_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, vc, n, min_weight, vcounts, tcounts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::tsdf_mesh_scan_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, vcounts, tcounts, nb, totals);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::tsdf_mesh_vertices_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, vc, n, min_weight, vcounts, tcounts, scratch,
                       xyz, vertex_capacity, triangle_capacity);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::tsdf_mesh_triangles_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, vc, n, min_weight, vcounts, tcounts, scratch,
                       tri, triangle_capacity);
    return (int)hipGetLastError();
}

}  // namespace dvo_tsdf
