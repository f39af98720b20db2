/*
 * dvo_esdf_launch.h -- internal interface between the distance-field host code (dvo_capi_tsdf.cpp) and its kernels (dvo_esdf.hip), and
 * the shape of their launches as pure host arithmetic.  Not installed; plain structs only.  The definition is dvo_esdf.h.
 *
 * An update is kEsdfUpdateLaunches launches whatever the list: pass x fused with the classification (TSDF pool -> ESDF pool), pass y
 * (ESDF pool -> scratch), pass z (scratch -> ESDF pool).  Every launch covers every listed volume: a workgroup finds its volume by its
 * number, as the integrate kernel does.
 */
#ifndef DVO_ESDF_LAUNCH_H_
#define DVO_ESDF_LAUNCH_H_

#include "dvo_esdf.h"

namespace dvo_tsdf {

constexpr int kEsdfUpdateLaunches = 3;             /* == DVO_ESDF_UPDATE_LAUNCHES */
constexpr int kEsdfBlock = 256;                    /* threads of every workgroup here: four waves */
constexpr int kEsdfWaves = kEsdfBlock / 64;
/* Pass x: a wave owns one whole x-row and walks it in chunks of kEsdfRowChunk voxels, one per lane; a chunk's site flags are one 64-bit
 * ballot, a row's at most kEsdfRowChunks of them.  A workgroup owns kEsdfWaves consecutive rows */
constexpr int kEsdfRowChunk = 64;
constexpr int kEsdfRowChunks = kMaxDim / kEsdfRowChunk;
/* Passes y and z: a workgroup owns kEsdfRowChunk consecutive x (one per lane, so that every access of a wave is one contiguous run) times
 * kEsdfColumnTile consecutive positions along the pass's axis, kEsdfColumnTile / kEsdfWaves of them per wave */
constexpr int kEsdfColumnTile = 32;
static_assert(kEsdfRowChunk == 64 && kEsdfRowChunks * kEsdfRowChunk == kMaxDim && kEsdfColumnTile % kEsdfWaves == 0, "a lane per x, whole waves");

/* One volume of an update.  TSDF and ESDF words: pool[off .. off + n); its scratch words: scratch[scratch_off ..).  Workgroups
 * first[p] .. first[p] + esdf_blocks(p, ...) of launch p are the volume's */
struct EsdfVolume {
    long long off, scratch_off;
    int nx, ny, nz, pad_;
    unsigned first[3], pad2_;
};
DVO_TSDF_HD long long esdf_x_chunks(int nx) { return (nx + kEsdfRowChunk - 1) / kEsdfRowChunk; }
DVO_TSDF_HD long long esdf_tiles(int n) { return (n + kEsdfColumnTile - 1) / kEsdfColumnTile; }
/* the workgroups of pass p (0: x, 1: y, 2: z) for one volume */
inline long long esdf_blocks(int pass, int nx, int ny, int nz) {
    if (pass == 0) return ((long long)ny * nz + kEsdfWaves - 1) / kEsdfWaves;
    if (pass == 1) return esdf_x_chunks(nx) * esdf_tiles(ny) * nz;
    return esdf_x_chunks(nx) * esdf_tiles(nz) * ny;
}
/* THREE launches for every listed volume (vols: a device array, blocks[p]: the workgroups of launch p); returns the hipError_t */
int launch_esdf_update(const unsigned *pool, unsigned *esdf, unsigned *scratch, const EsdfVolume *vols, int n_vols, int min_weight, int sites,
                       const unsigned blocks[3], void *stream);
/* esdf_metres() of `count` consecutive words.  ONE launch */
int launch_esdf_distances(const unsigned *words, long long count, double voxel_size, float *out, void *stream);
/* esdf_query_point() of `count` points (xyz, out: device memory).  ONE launch */
int launch_esdf_query(const unsigned *words, const VolumeConst &vc, int count, const double *xyz, dvo_esdf_sample *out, void *stream);

}  // namespace dvo_tsdf
#endif
