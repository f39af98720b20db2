/*
 * dvo_tsdf_mesh.hip -- the triangle mesh of a fused volume (include/dvo_amd.h, "the surface as a triangle mesh"): four kernels.
 * dvo_tsdf_mesh.h is the definition; the kernels call its per-voxel and per-cell functions as they are.
 *
 * The tile walk of dvo_tsdf_walk.h.  COUNT: per tile, the vertices its voxels own and the triangles of the cells its voxels are the
 * first corner of.  SCAN: the walk's scan turns both count arrays into offsets and writes the two totals.  VERTICES: the walk
 * again; a voxel's vertices are the bits of its 7-bit edge mask, placed in the definition's order; a voxel that owns a vertex also
 * records the number of its first one and the mask in the scratch.  TRIANGLES: the walk again, a launch of its own because it reads
 * scratch that other workgroups wrote; a thread checks its cell, runs the six tetrahedra through the definition's table and names each
 * vertex through the scratch record of the corner voxel that owns the edge; its triangles are placed by their count.
 *
 * A scratch record is read only for an edge that carries a vertex, and such an edge's owner writes its record in the same call: records
 * of voxels without a vertex are never written and never read, so what an earlier call left in the scratch does not matter.
 * No atomics, no workgroup waits on another: the result is bit-identical under any schedule.  A tile whose offset is already past the
 * caller's capacity leaves at once -- a vertices tile only when, in addition, no triangle tile that still writes can name its vertices.
 * A mesh of more than kMeshMaxVertices vertices writes nothing (the host refuses it from the counts).
 */
#include "dvo_launch.h"
#include "dvo_tsdf_walk.h"

namespace dvo {
using namespace dvo_tsdf;

/* the corner words of voxel a's cell; false: a is past the volume or its own weight is below min_weight (it owns no vertex and is the
 * first corner of no valid cell) */
__device__ __forceinline__ bool mesh_voxel(const unsigned *__restrict__ words, const VolumeConst &vc, long long n, long long a, int min_weight,
                                           unsigned w[8], int &x, int &y, int &z) {
    if (a >= n) return false;
    if (word_w(words[a]) < min_weight) return false;
    walk_xyz(vc, (unsigned)a, x, y, z);
    mesh_corner_words(words, vc, x, y, z, (size_t)a, w);
    return true;
}

/* counts of one voxel: vertices in the low 16 bits, triangles in the high ones (a tile has at most 7 * 2048 and 12 * 2048) */
__global__ __launch_bounds__(kBlock) void tsdf_mesh_count_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                 unsigned long long *__restrict__ vcounts, unsigned long long *__restrict__ tcounts) {
    const long long base = walk_base();
    unsigned mine = 0;
    for (int pass = 0; pass < kExtractPasses; pass++) {
        unsigned w[8];
        int x, y, z;
        if (!mesh_voxel(words, vc, n, walk_voxel(base, pass), min_weight, w, x, y, z)) continue;
        const int inside8 = mesh_cell_inside(w, min_weight);
        mine += (unsigned)__popc(mesh_edge_mask(w, min_weight)) + ((unsigned)(inside8 < 0 ? 0 : mesh_cell_triangles(inside8)) << 16);
    }
    const unsigned *wave_sum = walk_wave_sums(mine);                         /* a wave: at most 7 * 512 and 12 * 512, no carry between the halves */
    if (threadIdx.x == 0) {
        unsigned v = 0, t = 0;
        for (int k = 0; k < kWalkWaves; k++) { v += wave_sum[k] & 0xFFFFu; t += wave_sum[k] >> 16; }
        vcounts[blockIdx.x] = v;
        tcounts[blockIdx.x] = t;
    }
}

/* one workgroup: the walk's scan over both count arrays; totals = {vertices, triangles} */
__global__ __launch_bounds__(kBlock) void tsdf_mesh_scan_kernel(unsigned long long *__restrict__ vcounts, unsigned long long *__restrict__ tcounts, unsigned nb, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long part[kBlock];
    walk_scan(vcounts, nb, part, totals);
    __syncthreads();
    walk_scan(tcounts, nb, part, totals + 1);
}

template <bool COLOUR>
__device__ __forceinline__ void tsdf_mesh_vertices_body(const unsigned *__restrict__ words, const unsigned long long *__restrict__ colours,
                                                        const VolumeConst &vc, long long n, int min_weight,
                                                        const unsigned long long *__restrict__ vcounts,
                                                        const unsigned long long *__restrict__ tcounts, const MeshScratch &scratch,
                                                        float *__restrict__ xyz, unsigned char *__restrict__ rgb, long long vertex_capacity,
                                                        long long triangle_capacity) {
    if (vcounts[gridDim.x] > (unsigned long long)kMeshMaxVertices) return;
    const long long base = walk_base();
    unsigned long long at = vcounts[blockIdx.x];
    /* a cell names vertices of voxels up to nx ny + nx + 1 words ahead of it: the first triangle tile that can name this tile's */
    const long long reach = (long long)vc.nx * vc.ny + vc.nx + 1;
    const unsigned first_user = base > reach ? (unsigned)((base - reach) / kExtractTile) : 0u;
    /* the same for the whole workgroup: no vertex of this tile is inside the buffer, and no triangle that is written names one */
    if (at >= (unsigned long long)vertex_capacity && tcounts[first_user] >= (unsigned long long)triangle_capacity) return;
    for (int pass = 0; pass < kExtractPasses; pass++) {
        const long long a = walk_voxel(base, pass);
        unsigned w[8];
        int x = 0, y = 0, z = 0;
        const unsigned mask = mesh_voxel(words, vc, n, a, min_weight, w, x, y, z) ? mesh_edge_mask(w, min_weight) : 0u;
        unsigned in_wave;
        const unsigned before = walk_before_mask<kMeshEdges>(mask, in_wave);
        unsigned long long o = walk_place(at, before, in_wave);
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
                        if constexpr (COLOUR) {
                            unsigned char c3[3];
                            mesh_vertex_colour(w[0], w[mesh_dir_corner(d)], colours[a], colours[a + (long long)mesh_corner_step(vc, mesh_dir_corner(d))], c3);
                            rgb[3 * o] = c3[0]; rgb[3 * o + 1] = c3[1]; rgb[3 * o + 2] = c3[2];
                        }
                    }
                    o++;
                }
        }
    }
}

__global__ __launch_bounds__(kBlock) void tsdf_mesh_vertices_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                    const unsigned long long *__restrict__ vcounts,
                                                                    const unsigned long long *__restrict__ tcounts, MeshScratch scratch,
                                                                    float *__restrict__ xyz, long long vertex_capacity, long long triangle_capacity) {
    tsdf_mesh_vertices_body<false>(words, nullptr, vc, n, min_weight, vcounts, tcounts, scratch, xyz, nullptr, vertex_capacity, triangle_capacity);
}
/* the same with colour (dvo_tsdf_colour.h): two colour words read and three bytes written per vertex inside the buffer */
__global__ __launch_bounds__(kBlock) void tsdf_mesh_vertices_colour_kernel(const unsigned *__restrict__ words, const unsigned long long *__restrict__ colours,
                                                                           VolumeConst vc, long long n, int min_weight,
                                                                           const unsigned long long *__restrict__ vcounts,
                                                                           const unsigned long long *__restrict__ tcounts, MeshScratch scratch,
                                                                           float *__restrict__ xyz, unsigned char *__restrict__ rgb,
                                                                           long long vertex_capacity, long long triangle_capacity) {
    tsdf_mesh_vertices_body<true>(words, colours, vc, n, min_weight, vcounts, tcounts, scratch, xyz, rgb, vertex_capacity, triangle_capacity);
}

__global__ __launch_bounds__(kBlock) void tsdf_mesh_triangles_kernel(const unsigned *__restrict__ words, VolumeConst vc, long long n, int min_weight,
                                                                     const unsigned long long *__restrict__ vcounts,
                                                                     const unsigned long long *__restrict__ tcounts, MeshScratch scratch,
                                                                     int *__restrict__ tri, long long triangle_capacity) {
    if (vcounts[gridDim.x] > (unsigned long long)kMeshMaxVertices) return;
    const long long base = walk_base();
    unsigned long long at = tcounts[blockIdx.x];
    if (at >= (unsigned long long)triangle_capacity) return;      /* the same for the whole workgroup: everything from here on is beyond the buffer */
    for (int pass = 0; pass < kExtractPasses; pass++) {
        const long long a = walk_voxel(base, pass);
        unsigned w[8];
        int x, y, z;
        const int inside8 = mesh_voxel(words, vc, n, a, min_weight, w, x, y, z) ? mesh_cell_inside(w, min_weight) : -1;
        const unsigned mine = inside8 < 0 ? 0u : (unsigned)mesh_cell_triangles(inside8);
        unsigned in_wave;
        const unsigned before = walk_before_count(mine, in_wave);
        unsigned long long o = walk_place(at, before, in_wave);
        if (mine)
            mesh_cell_emit(inside8,
                           [&](int corner, int d) { return mesh_scratch_vertex(scratch, a + (long long)mesh_corner_step(vc, corner), d); },
                           [&](int i0, int i1, int i2) {
                               if (o < (unsigned long long)triangle_capacity) { tri[3 * o] = i0; tri[3 * o + 1] = i1; tri[3 * o + 2] = i2; }
                               o++;
                           });
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

/* the same four launches with the colour variant of the vertices kernel */
int launch_tsdf_mesh_colour(const unsigned *words, const unsigned long long *colours, const VolumeConst &vc, int min_weight, unsigned long long *counts,
                            const MeshScratch &scratch, unsigned long long *totals, float *xyz, unsigned char *rgb, long long vertex_capacity, int *tri,
                            long long triangle_capacity, void *stream) {
    if (!words || !colours || !counts || !mesh_scratch_ok(scratch) || !totals || vertex_capacity < 0 || triangle_capacity < 0 || min_weight < 1 ||
        (vertex_capacity > 0 && (!xyz || !rgb)) || (triangle_capacity > 0 && !tri))
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
    hipLaunchKernelGGL(dvo::tsdf_mesh_vertices_colour_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, colours, vc, n, min_weight, vcounts,
                       tcounts, scratch, xyz, rgb, vertex_capacity, triangle_capacity);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::tsdf_mesh_triangles_kernel, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, words, vc, n, min_weight, vcounts, tcounts, scratch,
                       tri, triangle_capacity);
    return (int)hipGetLastError();
}

}  // namespace dvo_tsdf
