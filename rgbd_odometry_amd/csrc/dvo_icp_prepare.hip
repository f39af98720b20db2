/*
 * dvo_icp_prepare.hip -- the front end of the frame-to-model alignment (include/dvo_amd.h, "preparing a depth frame"): the bilateral
 * filter of the depth image and the normals of the now frame.  dvo_icp_prepare.h is the definition; the kernels call its filter_taps()
 * and normal_pixel() as they are.
 *
 * TWO launches per call, for every listed image at once; a kernel boundary stands between the filtered image and its normals.
 *   The filter kernel.  One thread per output pixel; a workgroup owns a tile of kTileRows x kTileCols pixels of one image -- a wave is
 *   one row of 64, one contiguous run of the image -- and stages the tile with its halo of `radius` in LDS as DECODED metres, so the
 *   division of a 16-bit millimetre by 1000 and the hole test of a float happen once per staged pixel and not once per tap.  A hole
 *   and a pixel outside the image are staged as +infinity: |inf - Dc| * range_scale is no bin, so the range test of the definition
 *   skips them with the compare it makes anyway.  Each thread then runs the taps in the definition's order, in registers: nothing is
 *   summed across lanes.  The spatial weight of a tap is the same for every lane: the table travels in the kernel's argument block,
 *   widened to words (SpatialWords), and a tap's weight is one scalar load.  The range table is indexed per lane and sits in LDS.
 *   The normals kernel.  One thread per pixel: five reads of the filtered image (the neighbours come from the cache), three floats
 *   written.
 * The images are only read, the outputs only written; no atomics, no workgroup waits on another.
 */
#include "dvo_launch.h"
#include "dvo_icp_prepare_launch.h"

namespace dvo {
using namespace dvo_icp;

/* the taps of a staged tile: `at` is the centre */
struct TileTap {
    const double *tile;
    int pitch, at;
    __device__ bool operator()(int dy, int dx, double *D) const {
        *D = tile[at + dy * pitch + dx];
        return true;
    }
};

/* dvo_icp_prepare_params.spatial, one word per weight */
struct SpatialWords { unsigned w[13 * 13]; };

__global__ __launch_bounds__(kFilterBlock) void icp_filter_kernel(const PrepareImage *__restrict__ images, dvo_icp_prepare_params fp, SpatialWords spatial,
                                                                  int format, int rows, int cols, unsigned tiles_per_image, unsigned tiles_x) {
    __shared__ double tile[kStageMost];
    __shared__ unsigned short range[kRangeBins];
    const unsigned img = blockIdx.x / tiles_per_image, tl = blockIdx.x - img * tiles_per_image;
    const unsigned tile_y = tl / tiles_x, tile_x = tl - tile_y * tiles_x;
    const void *depth = images[img].depth;
    float *out = images[img].depth_out;
    const int r = fp.radius, pitch = kTileCols + 2 * r, staged = (kTileRows + 2 * r) * pitch;
    const int x0 = (int)tile_x * kTileCols - r, y0 = (int)tile_y * kTileRows - r;
    if (threadIdx.x < kRangeBins) range[threadIdx.x] = fp.range[threadIdx.x];
    for (int i = threadIdx.x; i < staged; i += kFilterBlock) {
        const int ty = i / pitch, tx = i - ty * pitch, y = y0 + ty, x = x0 + tx;
        double D = __builtin_huge_val(), m;
        if (y >= 0 && y < rows && x >= 0 && x < cols && metres(depth, format, (size_t)y * (size_t)cols + (size_t)x, &m)) D = m;
        tile[i] = D;
    }
    __syncthreads();
    const int lx = threadIdx.x & (kTileCols - 1), ly = threadIdx.x / kTileCols;
    const int u = x0 + r + lx, v = y0 + r + ly;
    if (u >= cols || v >= rows) return;
    const int at = (ly + r) * pitch + lx + r;
    const double Dc = tile[at];
    float f = 0.0f;
    if (Dc < __builtin_huge_val()) {
        const TileTap tap = {tile, pitch, at};
        f = filter_taps(r, fp.range_scale, spatial.w, range, Dc, tap);
    }
    out[(size_t)v * (size_t)cols + (size_t)u] = f;
}

__global__ __launch_bounds__(kNormalsBlock) void icp_normals_kernel(const PrepareImage *__restrict__ images, double edge_max, int rows, int cols,
                                                                    unsigned blocks_per_image) {
    const unsigned img = blockIdx.x / blocks_per_image, blk = blockIdx.x - img * blocks_per_image;
    const size_t px = (size_t)blk * kNormalsBlock + threadIdx.x;
    if (px >= (size_t)rows * (size_t)cols) return;
    const PrepareImage &I = images[img];
    const double K[4] = {I.K[0], I.K[1], I.K[2], I.K[3]};
    const int v = (int)(px / (size_t)cols), u = (int)(px - (size_t)v * (size_t)cols);
    float n[3];
    (void)normal_pixel(I.depth_out, rows, cols, K, edge_max, u, v, n);
    float *q = I.normals_out + 3 * px;
    q[0] = n[0]; q[1] = n[1]; q[2] = n[2];
}
}  // namespace dvo

namespace dvo_icp {

int launch_icp_prepare(const PrepareImage *images, const dvo_icp_prepare_params &fp, int count, int depth_format, int rows, int cols, bool with_normals,
                       void *stream) {
    if (!images || count < 1 || !prepare_params_ok(&fp) || !format_ok(depth_format) || !shape_ok(rows, cols)) return (int)hipErrorInvalidValue;
    const unsigned tiles = filter_tiles(rows, cols), tiles_x = (unsigned)((cols + kTileCols - 1) / kTileCols), blocks = normals_blocks(rows, cols);
    if ((unsigned long long)tiles * (unsigned long long)count > 0x7FFFFFFFull || (unsigned long long)blocks * (unsigned long long)count > 0x7FFFFFFFull)
        return (int)hipErrorInvalidValue;
    dvo::SpatialWords spatial;
    for (int k = 0; k < 13 * 13; k++) spatial.w[k] = fp.spatial[k];
    hipLaunchKernelGGL(dvo::icp_filter_kernel, dim3(tiles * (unsigned)count), dim3(kFilterBlock), 0, (hipStream_t)stream, images, fp, spatial, depth_format,
                       rows, cols, tiles, tiles_x);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !with_normals) return (int)e;
    hipLaunchKernelGGL(dvo::icp_normals_kernel, dim3(blocks * (unsigned)count), dim3(kNormalsBlock), 0, (hipStream_t)stream, images, fp.edge_max, rows, cols,
                       blocks);
    return (int)hipGetLastError();
}

}  // namespace dvo_icp
