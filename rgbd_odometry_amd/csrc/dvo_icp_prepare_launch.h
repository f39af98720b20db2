/*
 * dvo_icp_prepare_launch.h -- internal interface between the host code of dvo_icp_prepare (dvo_capi_icp.cpp) and its kernels
 * (dvo_icp_prepare.hip).  Not installed; plain structs only.  The definition is dvo_icp_prepare.h.
 */
#ifndef DVO_ICP_PREPARE_LAUNCH_H_
#define DVO_ICP_PREPARE_LAUNCH_H_

#include "dvo_icp_prepare.h"

namespace dvo_icp {

constexpr int kPrepareLaunches = 2;                /* == DVO_ICP_PREPARE_LAUNCHES: the filter kernel, the normals kernel */
/* A filter workgroup owns a tile of kTileRows x kTileCols output pixels of one image, one thread per pixel: a wave is one row of the
 * tile, so its loads and stores of a row are one contiguous run.  The tile and its halo are staged in LDS as doubles: at the largest
 * radius (kTileRows + 12) x (kTileCols + 12) x 8 bytes = 17 KiB */
constexpr int kTileCols = 64;
constexpr int kTileRows = 16;
constexpr int kFilterBlock = kTileCols * kTileRows;
constexpr int kStageMost = (kTileRows + 2 * kPrepareMaxRadius) * (kTileCols + 2 * kPrepareMaxRadius);
constexpr int kNormalsBlock = 256;                 /* threads of a normals workgroup: 256 consecutive pixels of one image */

/* one image of a call on the device */
struct PrepareImage {
    const void *depth;
    float *depth_out;
    float *normals_out;                            /* NULL: the call has none */
    long long pad_;
    double K[4];
};
inline unsigned filter_tiles(int rows, int cols) {
    return (unsigned)((rows + kTileRows - 1) / kTileRows) * (unsigned)((cols + kTileCols - 1) / kTileCols);
}
inline unsigned normals_blocks(int rows, int cols) { return (unsigned)(((size_t)rows * (size_t)cols + kNormalsBlock - 1) / kNormalsBlock); }

/* The filter of every image, then -- with_normals -- their normals: 1 or kPrepareLaunches launches; images: a device array of `count`.
 * Returns the hipError_t */
int launch_icp_prepare(const PrepareImage *images, const dvo_icp_prepare_params &fp, int count, int depth_format, int rows, int cols, bool with_normals,
                       void *stream);

}  // namespace dvo_icp
#endif
