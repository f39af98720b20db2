/*
 * dvo_tsdf_raycast.hip -- ray casting of fused volumes into depth and normal maps (include/dvo_amd.h, "from the map back to depth").
 * dvo_tsdf_raycast.h is the definition; the kernel calls its per-ray function pixel() as it is.
 *
 * ONE launch for a whole view list.  A thread owns one pixel of one view; a wave owns a kRayWaveW x kRayWaveH pixel tile and a
 * workgroup kRayWavesX x kRayWavesY of them, so the 64 rays of a wave walk through neighbouring voxels and their eight-word gathers
 * fall into few lines (dvo_tsdf_launch.h has the shape, profiles/tsdf_raycast the measurement against a 64 x 1 row per wave).
 * Workgroups are numbered view by view, tiles row-major inside a view; tiles at the right and lower border are partial and their
 * threads outside the image leave at once.  The view record is the same for a whole workgroup and is read through a uniform index
 * (scalar loads).  Every pixel is one thread's and the kernel only reads the pool: no atomics, no workgroup waits on another, and the
 * images are bit-identical under any schedule and any batch.
 *
 * Work is skipped only where the definition's result cannot change (see the end of the header's comment): sample() reads the first
 * corner word and leaves on a weight below min_weight before the other seven are fetched, and pixel(..., clipped = true) marches only
 * the samples of clip(): those that can lie inside the volume's box.
 */
#include "dvo_launch.h"
#include "dvo_tsdf_launch.h"

namespace dvo {
using namespace dvo_tsdf;

template <bool COLOUR>
__device__ __forceinline__ void tsdf_raycast_body(const unsigned *__restrict__ pool, const unsigned long long *__restrict__ cpool,
                                                  const DeviceView *__restrict__ views, const RayConst &rc, int image_format, unsigned tiles_x,
                                                  unsigned tiles_per_view) {
    const unsigned vi = blockIdx.x / tiles_per_view, tile = blockIdx.x - vi * tiles_per_view;
    const unsigned ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const DeviceView &V = views[vi];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = (int)tx * kRayTileW + (wave % kRayWavesX) * kRayWaveW + lane % kRayWaveW;
    const int v = (int)ty * kRayTileH + (wave / kRayWavesX) * kRayWaveH + lane / kRayWaveW;
    if (u >= rc.cols || v >= rc.rows) return;
    const RayCamera cam = V.cam;
    const RayVolume rv = V.rv;
    if constexpr (COLOUR) pixel_colour(pool + V.off, cpool + V.off, rv, cam, rc, u, v, true, V.depth, V.normals, V.image, image_format);
    else pixel(pool + V.off, rv, cam, rc, u, v, true, V.depth, V.normals);
}

__global__ __launch_bounds__(kBlock) void tsdf_raycast_kernel(const unsigned *__restrict__ pool, const DeviceView *__restrict__ views, RayConst rc,
                                                              unsigned tiles_x, unsigned tiles_per_view) {
    tsdf_raycast_body<false>(pool, nullptr, views, rc, 0, tiles_x, tiles_per_view);
}
/* the same with colour (dvo_tsdf_colour.h): one 8-corner gather of colour words per hit pixel on top */
__global__ __launch_bounds__(kBlock) void tsdf_raycast_colour_kernel(const unsigned *__restrict__ pool, const unsigned long long *__restrict__ cpool,
                                                                     const DeviceView *__restrict__ views, RayConst rc, int image_format,
                                                                     unsigned tiles_x, unsigned tiles_per_view) {
    tsdf_raycast_body<true>(pool, cpool, views, rc, image_format, tiles_x, tiles_per_view);
}
}  // namespace dvo

namespace dvo_tsdf {

int launch_tsdf_raycast(const unsigned *pool, const DeviceView *views, int n_views, const RayConst &rc, void *stream) {
    if (!pool || !views || n_views < 1 || rc.rows < 1 || rc.cols < 1) return (int)hipErrorInvalidValue;
    const unsigned tiles_x = (unsigned)((rc.cols + kRayTileW - 1) / kRayTileW), tiles = raycast_tiles(rc.rows, rc.cols);
    const unsigned long long blocks = (unsigned long long)tiles * (unsigned long long)n_views;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::tsdf_raycast_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, pool, views, rc, tiles_x, tiles);
    return (int)hipGetLastError();
}

int launch_tsdf_raycast_colour(const unsigned *pool, const unsigned long long *colours, const DeviceView *views, int n_views, const RayConst &rc,
                               int image_format, void *stream) {
    if (!pool || !colours || !views || n_views < 1 || rc.rows < 1 || rc.cols < 1 || !image_format_ok(image_format)) return (int)hipErrorInvalidValue;
    const unsigned tiles_x = (unsigned)((rc.cols + kRayTileW - 1) / kRayTileW), tiles = raycast_tiles(rc.rows, rc.cols);
    const unsigned long long blocks = (unsigned long long)tiles * (unsigned long long)n_views;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dvo::tsdf_raycast_colour_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, pool, colours, views, rc,
                       image_format, tiles_x, tiles);
    return (int)hipGetLastError();
}

}  // namespace dvo_tsdf
