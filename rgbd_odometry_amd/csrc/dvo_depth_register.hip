/*
 * dvo_depth_register.hip -- depth registration of the frame stage (include/dvo_amd.h, "depth registration"; host side
 * dvo_capi_depth.cpp; the definition is dvo_depth_register.h, whose per-pixel function splat() both kernels of this file and the host
 * builder share).  Two launches per registration, whatever the number of images (DVO_DEPTH_REGISTER_LAUNCHES):
 *
 *   depth_scatter_kernel   one thread per raw depth pixel of every image of the call, lanes along u: a wave of 64 neighbouring pixels
 *                          of one depth row lands on one or a few contiguous segments of a colour row.  Image i is registered under
 *                          rig[i] (the resident per-pair table, offset to the call's first pair) from src[i] (the call's address
 *                          table).  No-return atomic min (relaxed, agent scope) into image i's 32-bit z-buffer.  Measured
 *                          against a variant that took its minima in an LDS window per 64 x 4 source tile first and then made
 *                          one global atomic per non-empty window word: this kernel 0.69 ms, the window 1.84 ms per 256 VGA
 *                          images (profiles/depth_register/README.md) -- the direct form is the one kept.
 *   depth_resolve_kernel   z-buffer -> 16-bit millimetres (0xFFFFFFFF -> 0), eight pixels per thread with 16-byte loads and stores,
 *                          and 0xFFFFFFFF back into the z-buffer: it is armed for the next call, the steady state needs no fill.
 *
 * Bounds: splat() clips a footprint to [0, cols) x [0, rows), rows * cols <= zstride, the image index is below count; a thread reads
 * src[i][p] only for p < depth_rows * depth_cols of its rig; the resolve covers count * zstride words, a multiple of 8.
 */
#include "dvo_launch.h"
#include "dvo_depth_register.h"

namespace dvo {

namespace {
constexpr int DR_BLOCK = 256;
constexpr unsigned DR_EMPTY = 0xFFFFFFFFu;
}  // namespace

__global__ void __launch_bounds__(DR_BLOCK)
depth_scatter_kernel(const dvo_depth_rig *__restrict__ rig, const void *const *__restrict__ src, int depth_format, unsigned blocks_per_image,
                     int rows, int cols, size_t zstride, unsigned *__restrict__ z) {
    const unsigned img = blockIdx.x / blocks_per_image;
    const dvo_depth_rig &g = rig[img];
    const size_t p = (size_t)(blockIdx.x - img * blocks_per_image) * DR_BLOCK + threadIdx.x;
    if (p >= (size_t)g.depth_rows * (size_t)g.depth_cols) return;
    double Z;
    if (depth_format == dvo_depth::kFormatU16 ? !dvo_depth::metres_u16(static_cast<const unsigned short *>(src[img])[p], &Z)
                                              : !dvo_depth::metres_f32(static_cast<const float *>(src[img])[p], &Z))
        return;
    dvo_depth::Splat s;
    if (!dvo_depth::splat(g, (int)(p / (size_t)g.depth_cols), (int)(p % (size_t)g.depth_cols), Z, rows, cols, &s)) return;
    unsigned *zi = z + (size_t)img * zstride;
    for (int y = s.y0; y < s.y1; y++)
        for (int x = s.x0; x < s.x1; x++)
            (void)__hip_atomic_fetch_min(zi + (size_t)y * cols + x, s.q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(DR_BLOCK)
depth_resolve_kernel(unsigned *__restrict__ z, unsigned short *__restrict__ out, size_t n8) {
    const size_t w = (size_t)blockIdx.x * DR_BLOCK + threadIdx.x;
    if (w >= n8) return;
    uint4 *zp = reinterpret_cast<uint4 *>(z) + 2 * w;
    const uint4 a = zp[0], b = zp[1];
    auto mm = [](unsigned v) { return v == DR_EMPTY ? 0u : v; };      /* a written word is 1 .. 65535 */
    uint4 o;
    o.x = mm(a.x) | (mm(a.y) << 16); o.y = mm(a.z) | (mm(a.w) << 16);
    o.z = mm(b.x) | (mm(b.y) << 16); o.w = mm(b.z) | (mm(b.w) << 16);
    reinterpret_cast<uint4 *>(out)[w] = o;
    const uint4 e = make_uint4(DR_EMPTY, DR_EMPTY, DR_EMPTY, DR_EMPTY);
    zp[0] = e; zp[1] = e;
}

size_t depth_register_stride(int rows, int cols) { return ((size_t)rows * cols + 7) / 8 * 8; }

hipError_t launch_depth_register(const dvo_depth_rig *rig, const void *const *src, int depth_format, int count, size_t max_depth_px,
                                 int rows, int cols, unsigned *z, unsigned short *out, hipStream_t s) {
    if (count < 1 || rows < 1 || cols < 1 || max_depth_px < 1 || !rig || !src || !z || !out) return hipErrorInvalidValue;
    if (depth_format != dvo_depth::kFormatF32 && depth_format != dvo_depth::kFormatU16) return hipErrorInvalidValue;
    const size_t zstride = depth_register_stride(rows, cols);
    const size_t bpi = (max_depth_px + DR_BLOCK - 1) / DR_BLOCK, n8 = zstride / 8 * (size_t)count, rblocks = (n8 + DR_BLOCK - 1) / DR_BLOCK;
    if (bpi * (size_t)count > 0x7fffffffu || rblocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(depth_scatter_kernel, dim3((unsigned)(bpi * count)), dim3(DR_BLOCK), 0, s, rig, src, depth_format, (unsigned)bpi, rows, cols,
                       zstride, z);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(depth_resolve_kernel, dim3((unsigned)rblocks), dim3(DR_BLOCK), 0, s, z, out, n8);
    return hipGetLastError();
}

}  // namespace dvo
