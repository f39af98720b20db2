/*
 * dvo_tsdf_launch.h -- internal interface between the depth-fusion host code (dvo_capi_tsdf.cpp) and its kernels (dvo_tsdf_map.hip,
 * dvo_tsdf_raycast.hip, dvo_tsdf_mesh.hip).  Not installed; plain structs only.  The definitions are dvo_tsdf_map.h, dvo_tsdf_raycast.h,
 * dvo_tsdf_mesh.h and, for the colour variants of all three, dvo_tsdf_colour.h.
 */
#ifndef DVO_TSDF_LAUNCH_H_
#define DVO_TSDF_LAUNCH_H_

#include "dvo_tsdf_map.h"
#include "dvo_tsdf_raycast.h"
#include "dvo_tsdf_mesh.h"
#include "dvo_tsdf_colour.h"

namespace dvo_tsdf {

constexpr int kIntegrateLaunches = 1;              /* == DVO_TSDF_INTEGRATE_LAUNCHES */
constexpr int kExtractLaunches = 3;                /* == DVO_TSDF_EXTRACT_LAUNCHES */
constexpr int kBlock = 256;                        /* threads of every workgroup here */
constexpr int kRun = 4;                            /* words one thread of the integrate kernel owns: one 16-byte access */
constexpr int kExtractPasses = 8;                  /* an extract workgroup walks kExtractPasses * kBlock consecutive voxels */
constexpr int kExtractTile = kExtractPasses * kBlock;

/* One volume of an integrate call.  Its words are pool[off .. off + n); its threads own the 16-byte groups of the POOL (not of the
 * volume) from group_first = off / 4 on, so that a group is one aligned access whatever `off` is; the words of a group that lie outside
 * the volume -- in its first and last group -- belong to a neighbour and are not touched.  Workgroups block_first .. block_first + nblocks
 * of the launch are the volume's; its frames are frames[frame_first .. frame_first + frame_count), in list order */
struct DeviceVolume {
    long long off, n;
    VolumeConst vc;
    int frame_first, frame_count;
    unsigned block_first, nblocks;
};
inline unsigned integrate_blocks(long long off, long long n) {
    const long long groups = (off + n + kRun - 1) / kRun - off / kRun;
    return (unsigned)((groups + kBlock - 1) / kBlock);
}
/* ONE launch for every listed volume and frame (vols, frames: device arrays); returns the hipError_t */
int launch_tsdf_integrate(unsigned *pool, const DeviceVolume *vols, int n_vols, const Frame *frames, const FrameConst &fc, unsigned total_blocks,
                          void *stream);
/* the same with colour: colours = the colour pool (the voxel pool's layout, 8 bytes per voxel), images[k] = the image of frames[k] (a
 * device array of device pointers), all of image_format.  ONE launch */
int launch_tsdf_integrate_colour(unsigned *pool, unsigned long long *colours, const DeviceVolume *vols, int n_vols, const Frame *frames,
                                 const void *const *images, int image_format, const FrameConst &fc, unsigned total_blocks, void *stream);

/* the points of one volume (words: pool + off).  THREE launches: count per workgroup, scan of the counts by one workgroup, write in
 * definition order.  counts: extract_blocks(n) + 1 words of 8 bytes; out: 16 bytes {n_points, 0} then min(capacity, n_points) points */
inline unsigned extract_blocks(long long n) { return (unsigned)((n + kExtractTile - 1) / kExtractTile); }
int launch_tsdf_extract(const unsigned *words, const VolumeConst &vc, int min_weight, unsigned long long *counts, unsigned char *out,
                        long long capacity, void *stream);

/* ---- ray casting (dvo_tsdf_raycast.hip) ---- */
constexpr int kRaycastLaunches = 1;                /* == DVO_RAYCAST_LAUNCHES */
/* One thread per pixel.  A wave owns kRayWaveW x kRayWaveH pixels (lane = x + kRayWaveW * y inside it), a workgroup kRayWavesX x
 * kRayWavesY waves: square per-wave tiles keep a wave's rays in neighbouring voxels (profiles/tsdf_raycast: 8 x 8 against 64 x 1) */
constexpr int kRayWaveW = 8, kRayWaveH = 8;
constexpr int kRayWavesX = 2, kRayWavesY = 2;
constexpr int kRayTileW = kRayWaveW * kRayWavesX, kRayTileH = kRayWaveH * kRayWavesY;
static_assert(kRayWaveW * kRayWaveH == 64 && kRayWavesX * kRayWavesY * 64 == kBlock, "a workgroup is kBlock threads in whole waves");

/* One view of a ray-cast call: its camera, its volume (words: pool[off ..)) and where its images go (device memory: depth rows x cols of
 * the call's format, normals 3 rows x cols floats or NULL, image rows x cols of the call's image format in a colour call).  The same for a
 * whole workgroup */
struct DeviceView {
    RayCamera cam;
    RayVolume rv;
    long long off;
    void *depth;
    float *normals;
    void *image;
};
inline unsigned raycast_tiles(int rows, int cols) {
    return (unsigned)((cols + kRayTileW - 1) / kRayTileW) * (unsigned)((rows + kRayTileH - 1) / kRayTileH);
}
/* ONE launch for every listed view (views: a device array); returns the hipError_t */
int launch_tsdf_raycast(const unsigned *pool, const DeviceView *views, int n_views, const RayConst &rc, void *stream);
/* the same with colour: every view's `image` is set; colours = the colour pool.  ONE launch */
int launch_tsdf_raycast_colour(const unsigned *pool, const unsigned long long *colours, const DeviceView *views, int n_views, const RayConst &rc,
                               int image_format, void *stream);

/* ---- the triangle mesh (dvo_tsdf_mesh.hip) ---- */
constexpr int kMeshLaunches = 4;                   /* == DVO_MESH_LAUNCHES */
/* The per-voxel scratch of a mesh call: for every voxel that owns a vertex, the number of its first vertex and its 7-bit edge mask, in
 * two arrays of one block -- 4 n bytes of numbers, then n bytes of masks: 5 bytes per voxel (profiles/tsdf_mesh: against one 8-byte
 * record per voxel).  Records of voxels that own no vertex are never written and never read */
struct MeshScratch {
    int *first;
    unsigned char *mask;
};
inline size_t mesh_scratch_bytes(long long n) { return 5 * (size_t)n; }
inline MeshScratch mesh_scratch_at(unsigned char *block, long long n) {
    MeshScratch s;
    s.first = reinterpret_cast<int *>(block); s.mask = block + 4 * (size_t)n;
    return s;
}
inline bool mesh_scratch_ok(const MeshScratch &s) { return s.first && s.mask; }
DVO_TSDF_HD void mesh_scratch_store(const MeshScratch &s, long long a, int first, unsigned mask) {
    s.first[a] = first; s.mask[a] = (unsigned char)mask;
}
/* the number of the vertex on owned edge d of voxel a */
DVO_TSDF_HD int mesh_scratch_vertex(const MeshScratch &s, long long a, int d) { return mesh_vertex_number(s.first[a], s.mask[a], d); }
/* the mesh of one volume (words: pool + off).  FOUR launches: count per workgroup, scan of both count arrays by one workgroup, vertices
 * and scratch, triangles.  counts: 2 * (extract_blocks(n) + 1) words of 8 bytes; totals: 16 bytes {n_vertices, n_triangles}; xyz, tri:
 * device memory for vertex_capacity and triangle_capacity entries of 12 bytes (NULL with capacity 0) */
int launch_tsdf_mesh(const unsigned *words, const VolumeConst &vc, int min_weight, unsigned long long *counts, const MeshScratch &scratch,
                     unsigned long long *totals, float *xyz, long long vertex_capacity, int *tri, long long triangle_capacity, void *stream);
/* the same with colour: colours = the volume's colour words, rgb = device memory for vertex_capacity entries of 3 bytes (NULL with
 * capacity 0), written by the vertices kernel.  FOUR launches */
int launch_tsdf_mesh_colour(const unsigned *words, const unsigned long long *colours, const VolumeConst &vc, int min_weight, unsigned long long *counts,
                            const MeshScratch &scratch, unsigned long long *totals, float *xyz, unsigned char *rgb, long long vertex_capacity, int *tri,
                            long long triangle_capacity, void *stream);

}  // namespace dvo_tsdf
#endif
