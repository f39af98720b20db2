/*
 * dvo_launch.h -- internal interface between the C-ABI host code (dvo_capi.cpp)
 * and the HIP kernels (dvo_kernels.hip).  Not installed; plain structs only.
 */
#ifndef DVO_LAUNCH_H_
#define DVO_LAUNCH_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dvo_device_math.h"

struct dvo_depth_rig;         /* include/dvo_amd.h, dvo_depth_register.h */

namespace dvo {
/* Kernel launches issued by the calling host thread (dvo_tracker_get_stats reports the difference over one step).  Every launch of
 * the library goes through hipLaunchKernelGGL, redefined below to count; thread-local, so a context's keep-warm thread does not count. */
inline thread_local unsigned long long g_kernel_launches = 0;
}  // namespace dvo
#ifdef hipLaunchKernelGGL
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...)                               \
    do {                                                                  \
        ++dvo::g_kernel_launches;                                         \
        hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__);            \
    } while (0)
#endif

#define DVO_LEVELS 8          /* == DVO_MAX_LEVELS of include/dvo_amd.h */
#define DVO_NACC 29           /* == DVO_NUM_ACC */
#define DVO_NACC_PAD 32
/* where the fused kernel reads the now level of a (pair, level) from */
enum { DVO_TEXMODE_GLOBAL16 = 0, DVO_TEXMODE_LDS16 = 1, DVO_TEXMODE_PAL4 = 2,
       DVO_TEXMODE_EXACT_RAN = 0x100 /* flag: a wave of the packed kernel took the literal-division fallback at this level */,
       DVO_TEXMODE_PT4 = 0x200       /* flag: the level's reference points were read in their 4-byte form */,
       DVO_TEXMODE_E2_SHIFT = 12, DVO_TEXMODE_E2_MAX = 0xffff /* bits 12..27: iterations of the level whose energy came from the exact sweep (round 6) */,
       DVO_TEXMODE_RANKS_LDS = 0x400 /* flag (with DVO_TEXMODE_PAL4): the level's ranks were looked up in an LDS copy of the whole level (round 5) */,
       DVO_TEXMODE_FINAL_FUSED = 0x800 /* flag: the level's final outputs were written by its last, residual-only sweep at the best iterate before it; the separate pass was skipped */,
       DVO_TEXMODE_PT4_DIRECT = 0x10000000 /* flag (with DVO_TEXMODE_PT4): the 4-byte points in LDS were in the direct form (dvo_points_direct.h) */ };

namespace dvo {

/* One pyramid level of every pair of a context ("slab" layout in HBM):
 *   tex : n_pairs x tex_stride texels {DT, gx, gy, 0} (16 B / pixel), pixel (yy,xx) of pair p at
 *         tex[p*tex_stride + texel_index(yy, xx, tiles_per_col)]   (tiled, see dvo_device_math.h)
 *   pts : n_pairs x pt_cap x 3 floats, point i of pair p at pts[(p*pt_cap + i)*3]
 *         (the reference's 3xN column-major SpaceCordList, 12 B / point)
 *   N   : n_pairs ints                                                          */
struct LevelSlab {
    const float4 *tex;
    const float *pts;
    const uint2 *cpts;      /* compact points {xx | yy << 16, Z}, pt_cap per pair; valid where the host says so (Schedule.compact) */
    const unsigned *cidx;   /* index of each compact point in the 3 x N list (block order -> reference order), pt_cap per pair */
    const unsigned *cpt4;   /* 4-byte points (pt4_decode), pt_cap per pair */
    const unsigned *chdr;   /* chunk headers of the 4-byte points, pt_cap / 64 per pair */
    const int *pt4_ok;      /* per pair: the 4-byte list is valid (NULL: never built) */
    const int *N;
    size_t tex_stride;      /* texels per pair */
    int pt_cap;             /* points per pair (capacity) */
    int rows, cols;
    /* compact form of the now level (dvo_palette.h); pal_n[p] > 0: pair p has one (its palette size), <= 0: it has not */
    const unsigned *p4;     /* n_pairs x p4_stride rank words */
    const float2 *pal;      /* n_pairs x DVO_PAL_MAX palette entries {DT value, weight} */
    const int *pal_n;       /* n_pairs (NULL: never built) */
    size_t p4_stride;       /* dwords per pair */
};
struct LevelSet { LevelSlab l[DVO_LEVELS]; };

struct Schedule {
    int n_levels;
    int iters[DVO_LEVELS];
    int e_off[DVO_LEVELS];   /* offset of level l inside a pair's energy block */
    int e_stride;            /* floats per pair = sum iters */
    int last_level;          /* smallest l with iters[l] > 0 (its outputs survive, SolveDVO.cpp:2102) */
    int flags;
    int alias_mod;           /* diagnostics: data of pair p % alias_mod (0 = off) */
    int lds_points;          /* reference points kept resident in LDS per workgroup (3 words each, 2 when compact) */
    int lds_bytes;           /* dynamic LDS of the launch (dvo_fused.hip splits it per level between points and the now level) */
    int no_lds_tex;          /* diagnostics: never stage the now level into LDS */
    int no_p4;               /* diagnostics: never read the compact form of a now level (dvo_palette.h) */
    int team;                /* workgroups per pair of the packed kernel (1 = none; > 1: team mode, see dvo_fused.hip) */
    int n_pairs_launch;      /* pairs of this launch (team mode maps workgroups to pairs itself) */
    int force_e2;            /* tests (engine_variant 5): the energy certificate always fails -> every iteration takes the exact sweep of the residuals */
    int force_exact;         /* tests: every wave takes the literal-division fallback of the packed kernel (accumulate_points_exact) */
    int compact;             /* every pair/level of this launch has a compact point list: read 8 B / point instead of 12 */
    int no_pt4;              /* never read the 4-byte form of a reference list (a list encoded against a level of another height) */
    int no_pt4_direct;       /* tests (engine_variant 6): 4-byte points keep their block-relative form in LDS */
    int final_blk;           /* host bookkeeping: the final outputs of this launch are stored in the compact lists' (block) order */
    unsigned team_epoch0;    /* team mode: tags of this launch's records start above every tag an earlier launch left in the buffer (no memset between launches) */
};

#define DVO_TILED_SOLO_MAX_DEFAULT 6144     /* tiled / wide schedule: levels of at most this many points run as one launch (dvo_fused.hip) */

struct Intrinsics {
    float fx, fy, cx, cy;
    int interp;              /* dvo_params.interpolate_dt, travels with the camera model to every kernel */
    int pad_;
    /* per-pair camera models (the multi-stream trackers' per-stream calibration): {fx, fy, cx, cy} of pair p at pair_K[p]; NULL =
     * every pair uses fx .. cy above.  Read through pair_intrinsics by the kernels that run many pairs in one launch */
    const float4 *pair_K;
};
/* the camera model of `pair` (wave-uniform at every call site): one load per workgroup and level, its values pinned to scalar
 * registers, so that nothing derived from them occupies a vector register */
__device__ __forceinline__ Intrinsics pair_intrinsics(const Intrinsics &K, int pair) {
    if (!K.pair_K) return K;
    const float4 k = K.pair_K[pair];
    Intrinsics r = K;
    r.fx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(k.x)));
    r.fy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(k.y)));
    r.cx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(k.z)));
    r.cy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(k.w)));
    r.pair_K = nullptr;
    return r;
}

struct Outputs {
    double *poses;           /* n_pairs x 12 : R[9] col-major, t[3] */
    float *energy;           /* n_pairs x e_stride */
    int *best_idx;           /* n_pairs x DVO_LEVELS */
    float *ratio;            /* n_pairs x DVO_LEVELS */
    float *final_eps;        /* n_pairs x final_cap */
    float *final_reproj;     /* n_pairs x 3*final_cap */
    int *final_N;            /* n_pairs */
    int final_cap;
    double *H;               /* DVO_FLAG_NORMAL_MATRIX: n_pairs x e_stride x 21 (upper triangle of sum w J J^T per iterate), else NULL */
    double *team_buf;        /* team mode: n_pairs x 2 x 16 x 8 records of 16 bytes {value, tag} (partial sums of the members, double-buffered; tags of earlier launches are all below Schedule.team_epoch0 + 1) */
    unsigned *team_cnt;      /* (unused by the kernel; the int after n_pairs entries is the error flag) */
    int *team_err;           /* set to 1 by a member that gave up waiting (members not co-resident) */
    int *tex_mode;           /* n_pairs x DVO_LEVELS: where the fused kernel read the now level from (DVO_TEXMODE_*), inspection */
    const int *order;        /* launch order of the pairs (longest first): workgroup b aligns pair first_pair + order[b]; NULL = b */
};

hipError_t launch_pack_texels(const float *dt, const float *gx, const float *gy, float4 *out,
                              int rows, int cols, hipStream_t s);
/* compact form of now levels [first_pair, first_pair+count) of one pyramid level from their 16-byte texels (dvo_palette.hip) */
size_t palette_work_ints(int count);        /* scratch of one launch_palette_build over `count` images */
hipError_t launch_palette_build(const float4 *tex, size_t tex_stride, int rows, int cols, unsigned *p4, size_t p4_stride,
                                float2 *pal, int *pal_n, int first_pair, int count, unsigned *work, hipStream_t s);
bool fused_uses_compact(int points_in_flight, int interp);
hipError_t launch_replicate_level(float4 *tex, const unsigned char *src_has_tex /* device, n_src flags, or NULL = all */, size_t tex_stride, float *pts,
                                  uint2 *cpts, unsigned *cidx, unsigned *cpt4, unsigned *chdr, int *pt4_ok, int pt_cap, int *N, int n_src, int dst_first,
                                  int dst_count, hipStream_t s);
/* 4-byte twins of the compact lists of pairs [first_pair, first_pair + count): encode, decode with pt4_decode, compare with the
 * 8-byte form; pt4_ok[pair] = 1 only if every point survives */
/* a caller's 3xN list -> {xx | yy << 16, Z} where every point verifies bit for bit (dvo_frames.hip); *fail is set otherwise */
hipError_t launch_points_recover_compact(const float *xyz, int N, int level, const Intrinsics &K, uint2 *compact, unsigned *cidx, int *fail, hipStream_t s);
hipError_t launch_points4_build(const uint2 *cpts, const int *N, int pt_cap, int rows, unsigned *cpt4, unsigned *chdr, int *pt4_ok,
                                int first_pair, int count, hipStream_t s);
/* the same for pairs map[0 .. count).y (index-list form, dvo_tracker.hip) */
hipError_t launch_points4_build_list(const uint2 *cpts, const int *N, int pt_cap, int rows, unsigned *cpt4, unsigned *chdr, int *pt4_ok,
                                     const int2 *map, int count, hipStream_t s);
/* final outputs stored in block order -> the reference's order: out[cidx[i]] = in[i] */
hipError_t launch_final_permute(const unsigned *cidx, const float *fe_blk, const float *fr_blk, int n, float *fe, float *fr, hipStream_t s);
/* the compact now form of slots [dst_first, dst_first+dst_count) <- that of pair (p - dst_first) % n_src */
hipError_t launch_replicate_compact(unsigned *p4, size_t p4_stride, float2 *pal, int *pal_n, int n_src, int dst_first,
                                    int dst_count, hipStream_t s);
hipError_t launch_align_fused(int block_threads, int points_in_flight, const LevelSet &lv,
                              const Schedule &sc, const Intrinsics &K, const DevParams &prm,
                              const Outputs &out, int first_pair, int n_pairs, hipStream_t s);
/* the same schedule on two points per lane in packed float32 (dvo_fused.hip); needs sc.compact */
hipError_t launch_align_fused2(int block_threads, const LevelSet &lv, const Schedule &sc, const Intrinsics &K,
                               const DevParams &prm, const Outputs &out, int first_pair, int n_pairs, hipStream_t s);
size_t fused2_static_lds(int block_threads, bool with_h = false);
/* per-point dump at a float pose (inspection) */
hipError_t launch_eval_points(const LevelSlab &L, int pair, int level, const Intrinsics &K,
                              const float *Rf, const float *tf,
                              float *reproj, float *J, float *eps, float *w, int *vis, hipStream_t s);
/* 29 accumulators at a float pose: partials [nblocks x 32] then acc[32] */
hipError_t launch_accumulate(const LevelSlab &L, int pair, int level, const Intrinsics &K,
                             const float *Rf, const float *tf, int first_point, int n_points,
                             double *partials, int nblocks, double *acc, hipStream_t s);
int accumulate_blocks_for(int n_points);
/* host-driven iteration: optimiser state (opaque, pose_state_bytes() each) in HBM */
size_t pose_state_bytes();
hipError_t launch_iter_begin(void *state, const DevParams &prm, const double *Rt12, float *energy, int max_iters, hipStream_t s);
hipError_t launch_iter_accumulate(const LevelSlab &L, int pair, int level, const Intrinsics &K, const void *state,
                                  int first_point, int n_points, double *partials, int nblocks, double *acc,
                                  hipStream_t s);
hipError_t launch_iter_update(void *state, const DevParams &prm, int itr, int n_total, const double *acc,
                              float *energy, hipStream_t s);
hipError_t launch_iter_step_fused(const LevelSlab &L, int pair, int level, const Intrinsics &K, void *state,
                                  const DevParams &prm, int itr, int n_points, double *partials, int nblocks,
                                  float *energy, hipStream_t s);
hipError_t launch_iter_end(void *state, double *Rt12, int *best_idx, float *ratio, hipStream_t s);
/* one launch per iteration (round 4, dvo_kernels.hip: tiled_step_kernel): pending update of iteration itr - 1 (apply_prev) from the
 * reduced sums acc_in and the state st_in -> st_out, this rank's point range at the new pose, the 32 sums of the launch in acc_out */
int tiled_step_blocks(int n_points, int n_cu);
hipError_t launch_tiled_step(const LevelSlab &L, int pair, int level, const Intrinsics &K, const DevParams &prm, const void *st_in,
                             void *st_out, const double *acc_in, int itr, int apply_prev, int n_total, int first_point, int n_points,
                             double *partials, unsigned *ticket, double *acc_out, float *energy, int nblocks,
                             double *H_prev /* NULL: the 21 H sums are not formed; else: where H of iterate itr - 1 goes (21 doubles) */, hipStream_t s);
/* the same launch with the packed point loop over the compact list (dvo_fused.hip: tiled_step_pk_kernel) */
hipError_t launch_tiled_step_pk(const LevelSlab &L, int pair, int level, const Intrinsics &K, const void *st_in, void *st_out,
                                const double *acc_in, int itr, int apply_prev, int n_total, int first_point, int n_points,
                                double *partials, unsigned *ticket, double *acc_out, float *energy, int nblocks, double *H_prev, hipStream_t s);
/* a small level of the schedule as ONE launch of one workgroup: all its iterations, then what launch_tiled_finish does (dvo_fused.hip) */
hipError_t launch_tiled_level_solo(const LevelSlab &L, int pair, int level, const Intrinsics &K, const void *st_in, void *st_out, int iters,
                                   int n_points, float *energy, double *Rt12, int *best_idx, float *ratio, float *next_energy,
                                   int next_iters, hipStream_t s);
hipError_t launch_tiled_finish(const void *st_in, void *st_out, const DevParams &prm, const double *acc_in, int itr_last, int n_total,
                               float *energy, double *Rt12, int *best_idx, float *ratio, double *H_last, float *next_energy, int next_iters,
                               hipStream_t s);      /* next_iters > 0: also what iter_begin does for the next level (its energies: next_energy) */
/* finalEpsilons / finalReprojections of points [first, first+n) at the best iterate kept in `state` (host-driven / tiled paths) */
hipError_t launch_final_outputs_state(const LevelSlab &L, int pair, int level, const Intrinsics &K, const void *state,
                                      int first_point, int n_points, float *final_eps, float *final_reproj, int *final_N,
                                      hipStream_t s);
hipError_t launch_unpack_texels(const float4 *tex, int rows, int cols, float *dt, float *gx, float *gy, hipStream_t s);
/* one wave asleep for `us` microseconds of real time (dvo_set_keep_warm) */
hipError_t launch_keep_warm(int us, hipStream_t s);
/* SE(3) helpers on one lane (property tests) */
hipError_t launch_se3_exp(const double *psi, double *Rt12, hipStream_t s);
hipError_t launch_se3_log(const double *Rt12, double *psi, hipStream_t s);
hipError_t launch_rotationize(double *R9, hipStream_t s);

/* ---- per-frame preprocessing (dvo_frames.hip).  Every launcher is batched over g.count same-geometry
 * images; image b of a buffer is at base + b*stride (in elements of that buffer). ---- */
struct ImgBatch { int rows, cols, count; };

/* host-format image -> resident column-major grey (u8) / depth (f32 mm).  dtype: 0 u8, 1 u16, 2 f32 */
hipError_t launch_import_grey(const void *src, int dtype, int row_major, size_t src_stride,
                              unsigned char *grey, size_t stride, ImgBatch g, hipStream_t s);
hipError_t launch_import_depth(const void *src, int dtype, int row_major, size_t src_stride,
                               float *depth_mm, size_t stride, ImgBatch g, hipStream_t s);
/* row f2: full-resolution camera image (+ depth, may be NULL) row-major -> pyramid level decimated by 2^shift.
 * CamSrc: the images of a launch in their sensor format (dvo_amd.h): image i at img + i * img_stride BYTES, rows x cols x {3, 3, 1} bytes
 * for img_fmt DVO_CAM_BGR8 / _RGB8 / _MONO8; depth i at depth + i * depth_stride PIXELS of depth_fmt DVO_DEPTH_F32 (metres, or sensor
 * units with depth_raw) / DVO_DEPTH_U16 (millimetres).  The kernels convert in registers.
 * SrcTab (round 6): DEVICE arrays of image pointers, one per image of the launch; non-NULL = the images are read where they are (camera
 * frames already in HBM) instead of at base + i * stride */
struct CamSrc { const unsigned char *img; size_t img_stride; int img_fmt; const void *depth; size_t depth_stride; int depth_fmt; };
struct SrcTab { const void *const *bgr; const void *const *depth; };
/* per-image undistortion maps of a camera-level launch (the tracker's per-stream calibration): image i of the launch is remapped with
 * xy[i] / frac[i], no remap where xy[i] is NULL.  NULL tables: the launch's one map (umap_xy / umap_frac) for every image */
struct UmapTab { const short2 *const *xy; const unsigned short *const *frac; };
hipError_t launch_gather_images(const void *const *src, int count, void *dst, size_t bytes, size_t stride, hipStream_t s, int max_wgs_per_image = 64);
hipError_t launch_camera_level(const CamSrc &src, int src_rows, int src_cols, int shift, const short2 *umap_xy, const unsigned short *umap_frac,
                               int depth_raw, unsigned char *grey, float *depth_mm, size_t stride, ImgBatch g, hipStream_t s, SrcTab tab = {nullptr, nullptr},
                               UmapTab utab = {nullptr, nullptr});
hipError_t launch_camera_levels(const CamSrc &src, int src_rows, int src_cols,
                                int n, const int *shift, const int *rows, const int *cols, const short2 *umap_xy, const unsigned short *umap_frac,
                                int depth_raw, unsigned char *const *grey, float *const *depth_mm, const size_t *stride, int count, hipStream_t s,
                                SrcTab tab = {nullptr, nullptr}, UmapTab utab = {nullptr, nullptr});
/* levels 1 .. n of a pyramid as nearest-neighbour decimations of its level 0 (valid when camera_levels_decimate_ok: no clamped index) */
bool camera_levels_decimate_ok(int n_levels, const int *rows, const int *cols);
hipError_t launch_camera_decimate_levels(const unsigned char *grey0, const float *depth0, size_t stride0, int rows0, int cols0, int n,
                                         const int *rows, const int *cols, unsigned char *const *grey, float *const *depth, const size_t *stride,
                                         int count, hipStream_t s);
/* row f1: cv::Canny(grey, low/high as squared integer thresholds, 3, L2).  work: canny_work_ints() ints;
 * edge out: 0/255 u8 */
size_t canny_work_ints(int rows, int cols, int count);
/* Canny of all pyramid levels of the same images in four launches (dvo_frames.hip) */
size_t canny_levels_work_ints(int n, const int *rows, const int *cols, int count);
bool canny_levels_ok(int n, const int *rows, const int *cols, unsigned char *const *edge, const size_t *edge_stride);
hipError_t launch_canny_levels(int n, const int *rows, const int *cols, const unsigned char *const *grey, const size_t *grey_stride,
                               unsigned char *const *edge, const size_t *edge_stride, int count, int low, int high, int *work, hipStream_t s);
hipError_t launch_canny(const unsigned char *grey, size_t stride, ImgBatch g, int low, int high, int *work,
                        unsigned char *edge, size_t edge_stride, hipStream_t s);
hipError_t launch_count_edges(const unsigned char *edge, size_t n, int *out, hipStream_t s);
/* edge mask -> distance transform -> the now level's resident form (SolveDVO.cpp:1768-1795, :1063-1098), for pairs
 * first_pair .. first_pair + g.count - 1.  p4 != NULL: the COMPACT form (dvo_palette.h) is written natively from the integer
 * squared distances -- p4 / pal / pal_n are the level's slabs (indexed by pair), tex_out (already offset to first_pair) only
 * receives the 16-byte texels of images the compact form cannot hold (pal_n < 0 then).  p4 == NULL: 16-byte texels of every
 * image.  work: edt_work_ints() ints */
/* launch_edges_to_now for all pyramid levels of the same images at once (dvo_frames.hip) */
bool edt_levels_ok(int n, const int *rows, const int *cols);
size_t edt_levels_work_ints(int n, const int *rows, const int *cols, int count);
hipError_t launch_edges_to_now_levels(int n, const int *rows, const int *cols, const unsigned char *const *edge, const size_t *edge_stride, int count,
                                      int *work, float4 *const *tex_out, const size_t *tex_stride, unsigned *const *p4, const size_t *p4_stride,
                                      float2 *const *pal, int *const *pal_n, int first_pair, hipStream_t s,
                                      bool only_texels = false /* only the pass that writes 16-byte texels (for images without a compact form); work as left by a full run */);
/* caller-supplied float images -> compact form (see dvo_frames.hip); work: float_level_work_ints() ints */
size_t float_level_work_ints(int rows, int cols);
hipError_t launch_float_level_to_compact(const float *dt, const float *gx, const float *gy, int rows, int cols, int *work,
                                         unsigned *p4, size_t p4_stride, float2 *pal, int *pal_n, int pair, hipStream_t s);
size_t edt_work_ints(int rows, int cols, int count);
hipError_t launch_edges_to_now(const unsigned char *edge, size_t edge_stride, ImgBatch g, int *work,
                               float4 *tex_out, size_t tex_stride, unsigned *p4, size_t p4_stride, float2 *pal, int *pal_n,
                               int first_pair, hipStream_t s, bool only_texels = false);
/* 16-byte texels of pairs [first_pair, first_pair + count) decoded from their compact form (pairs without one are skipped) */
hipError_t launch_p4_decode_texels(const unsigned *p4, size_t p4_stride, const float2 *pal, const int *pal_n, float4 *tex,
                                   size_t tex_stride, int rows, int cols, int first_pair, int count, hipStream_t s);
/* selectedPts + enlistRefEdgePts (SolveDVO.cpp:1230-1264, :224-264).  col_counts: (cols+2) ints per image;
 * after the count pass col_counts[cols] and [cols+1] hold N.  edge: int32 or u8 (>0 = edge).
 * blk_counts (may be NULL): enlist_block_ints(rows, cols) ints per image -- per (pixel column, 16-row segment) counts in
 * block order; with it the compact twin list is written in 16x16-block order (dvo_frames.hip), the 3xN float list and uv
 * always in the reference's order. */
size_t enlist_block_ints(int rows, int cols);
hipError_t launch_enlist_count(const void *edge, int edge_is_u8, size_t edge_stride, const float *depth_mm,
                               size_t depth_stride, ImgBatch g, int *col_counts, int *blk_counts, hipStream_t s,
                               const int2 *map = nullptr /* index-list form: image b = slot map[b].x of the bases */);
hipError_t launch_enlist_write(const void *edge, int edge_is_u8, size_t edge_stride, const float *depth_mm,
                               size_t depth_stride, ImgBatch g, int level, const Intrinsics &K, const int *col_counts,
                               const int *blk_counts, float *xyz, size_t xyz_stride,
                               uint2 *compact /* same stride in points / 3, or nullptr */, unsigned *cidx /* likewise */,
                               float *uv, int capacity, int *N_dst, hipStream_t s,
                               const int2 *map = nullptr /* index-list form: slot map[b].x -> pair map[b].y; xyz / compact / cidx /
                                                            N_dst are the slabs' bases */);

/* ---- ignore masks of the frame stage (dvo_frame_masks.hip; include/dvo_amd.h "ignore masks") ----
 * The keep planes of one mask are one allocation: level l at off[l] (a multiple of 16), rows[l] * cols[l] bytes, column-major, 0 / 255 */
size_t mask_levels_bytes(int n, const int *rows, const int *cols, size_t *off);
/* ONE launch: the rows x cols mask (device, row-major, non-zero = ignore) -> keep[l] of every level (dvo_mask_levels.h is the definition) */
hipError_t launch_mask_levels(const unsigned char *mask, int rows, int cols, int n, int first_shift, int margin, const int *lrows,
                              const int *lcols, unsigned char *const *keep, hipStream_t s);
/* ONE launch for all levels and all `count` images: edge[l] + i * edge_stride[l] &= the plane tab[i * DVO_LEVELS + l] (device table; a NULL
 * entry leaves the image's level as it is) */
hipError_t launch_edge_mask_levels(int n, const int *rows, const int *cols, unsigned char *const *edge, const size_t *edge_stride, int count,
                                   const unsigned char *const *tab, hipStream_t s);

/* ---- depth registration of the frame stage (dvo_depth_register.hip; include/dvo_amd.h "depth registration") ----
 * One image's z-buffer words and output pixels: rows * cols rounded up to 8 (every 16-bit output image starts on a 16-byte boundary) */
size_t depth_register_stride(int rows, int cols);
/* TWO launches (scatter, resolve) for all `count` images: image i (device, src[i]: a device table of device addresses, depth_format
 * DVO_DEPTH_*) under rig[i] (device table) -> out + i * stride, rows x cols 16-bit millimetres, row-major, 0 = hole
 * (dvo_depth_register.h is the definition).  z: count * stride words that hold 0xFFFFFFFF, and hold it again afterwards.
 * max_depth_px: the largest depth_rows * depth_cols among the rigs */
hipError_t launch_depth_register(const ::dvo_depth_rig *rig, const void *const *src, int depth_format, int count, size_t max_depth_px,
                                 int rows, int cols, unsigned *z, unsigned short *out, hipStream_t s);

/* ---- photometric Gauss-Newton (dvo_photo.hip): RGBDOdometry's engine ---- */
hipError_t launch_photo_select(const unsigned char *grey, int rows, int cols, double grad_threshold,
                               int *col_work /* 2*(cols+1) ints: counts | offs; offs[cols] = n, counts[cols] = last pixel selected */,
                               hipStream_t s);
hipError_t launch_photo_fill(const unsigned char *grey, const float *depth, int rows, int cols, int level,
                             double fx, double fy, double cx, double cy, int fixed, double grad_threshold, int capacity,
                             const int *col_work /* as launch_photo_select left it */, double *J, int *sel, double *zref, float *gref,
                             double *A36, int *n_out, hipStream_t s);
hipError_t launch_photo_gauss_newton(const double *J, const int *sel, const double *zref, const float *gref, const int *n_dev,
                                     const double *A36, const unsigned char *grey_now, int rows, int cols, int level,
                                     double fx, double fy, double cx, double cy, int fixed, int max_iters, double eps_stop,
                                     double *T16, double *eps_norms, int *updates, double *eps_dump, hipStream_t s);
/* index-list forms (the multi-stream engine, dvo_capi_photo_streams.cpp): per entry a stream, whose data sit in per-stream slabs,
 * and the frame-store slot of its latest frame */
struct PhotoEntry {
    int stream, slot;
    int flags;                /* Gauss-Newton: 1 = start from T = I (the stream took a new reference this tick) */
    int pad;
};
struct PhotoLevelSlab {       /* one pyramid level of every stream: stream s at J + s*cap*6, sel / zref / gref + s*cap, A + s*36, n + s */
    double *J, *zref, *A;
    int *sel, *n;
    float *gref;
    int *work;                /* select scratch: work_stride ints per stream, counts[cols + 1] | offs[cols + 1] as launch_photo_select */
    size_t work_stride;
    int cap;                  /* rows of J per stream: min(max_jacobian_size, rows * cols) */
    const unsigned char *grey;   /* frame store level: image of slot q at grey / depth + q * npx */
    const float *depth;
    size_t npx;
    int rows, cols;
};
struct PhotoSlabs { PhotoLevelSlab l[DVO_LEVELS]; };
struct PhotoRun { int n_run; int levels[DVO_LEVELS]; };
struct PhotoOut {             /* what one Gauss-Newton launch gives back per entry: ONE device-to-host read for the whole list */
    double T[16];
    double norms[64];         /* n_run x iterations, -1 where not run */
    int updates[DVO_LEVELS];
};
/* select: counts + scans of level `level` for every entry (ONE launch per stage); info[(k * DVO_LEVELS + level) * 2] = {n, last pixel
 * selected} of entry k.  fill: J, sel, zref, gref, A, n of every entry from its scan.  Gauss-Newton: ONE launch, one workgroup per entry,
 * every level of `run` in order. */
hipError_t launch_photo_select_list(const PhotoEntry *list, int n, const PhotoLevelSlab &L, int level, double grad_threshold, int *info,
                                    hipStream_t s);
hipError_t launch_photo_fill_list(const PhotoEntry *list, int n, const PhotoLevelSlab &L, int level, double fx, double fy, double cx,
                                  double cy, int fixed, double grad_threshold, hipStream_t s, const double *k_tab = nullptr);
hipError_t launch_photo_gauss_newton_list(const PhotoEntry *list, int n, const PhotoSlabs &S, const PhotoRun &run, double fx, double fy,
                                          double cx, double cy, int fixed, int max_iters, double eps_stop, double *T_all, PhotoOut *out,
                                          hipStream_t s, const double *k_tab = nullptr);

/* ---- multi-stream tracker (dvo_tracker.hip, include/dvo_amd.h "many camera streams") ---------------------------------------
 * One entry per stream listed in a step: stream id (= pair) and the host's part of the key-frame rule. */
struct TrackerEntry {
    int stream;
    int flags;                /* DVO_TRK_* below */
};
enum { DVO_TRK_FORCED = 1,    /* (nFrame - lastRefFrame) == keyFrameEvery (SolveDVO.cpp:2155-2160) */
       DVO_TRK_MAY_SWITCH = 2 /* lastRefFrame != nFrame - 1 (:2198) */ };
/* What a step reads back per listed stream (one D2H for all of them) */
struct TrackerOut {
    double pose[12];          /* R (column-major) + t of the pair's device pose */
    float b_cap, ratio;       /* Laplacian scale of finalEpsilons (0 without them), visible ratio of the finest level that ran */
    int n_points, event;      /* N of that level; 0 = ordinary, 2..5 = reasonForChange of a key-frame switch */
};
struct TrackerRule {
    int adaptive;             /* evaluate the three exits of :2129-2152 */
    float lap_thresh, ratio_thresh;
    int min_points;
};
/* one workgroup per entry: signals + key-frame rule + the pose gather.  eps / cidx may be NULL (no b_cap); cidx != NULL: eps are in the
 * compact list's (block) order and are put in list order first, through `scratch` (scratch_stride floats per entry) */
hipError_t launch_tracker_signals(const TrackerEntry *list, int count, const double *poses, const float *ratio, int last_level,
                                  const int *n_points, const float *eps, const unsigned *cidx, int eps_stride, int cidx_stride,
                                  float *scratch, int scratch_stride, TrackerRule rule, TrackerOut *out, hipStream_t s);
/* entries whose event is >= 2 (a key-frame switch): the pair's device pose becomes the identity (SolveDVO.cpp:2210-2211) */
hipError_t launch_tracker_reset_switched(const TrackerEntry *list, const TrackerOut *out, int count, double *poses, hipStream_t s);
/* pairs list[i].stream for i in [0, count): the device pose becomes the identity (first frame of a stream) */
hipError_t launch_tracker_reset_listed(const TrackerEntry *list, int count, double *poses, hipStream_t s);
/* entries whose event is >= 2: their pose after the re-run goes to out[i].pose */
hipError_t launch_tracker_gather_switched(const TrackerEntry *list, int count, const double *poses, TrackerOut *out, hipStream_t s);
/* The pose information of a listed stream (dvo_tracker_info.hip): the engine's accumulators at the stream's device pose on the finest
 * level that ran -- a separate array beside TrackerOut, read back only by a tracker that asked for it */
struct TrackerInfo {
    double H[21];             /* upper triangle of sum w J J^T, row-major */
    double g[6];              /* J^T W eps */
    double sum_eps2;          /* the correctly rounded exact sum */
    int n_visible, level;
};
/* one 512-thread workgroup per entry whose (out[i].event >= 2) == switched: info[i] of stream list[i].stream at poses + 12 * stream,
 * from the compact point list and the compact now form of level `level` (use_p4 false: 16-byte texels always); other entries' records
 * are left as they are */
hipError_t launch_tracker_information(const TrackerEntry *list, const TrackerOut *out, int switched, int count, const double *poses,
                                      const LevelSlab &L, int level, const Intrinsics &K, bool use_p4, TrackerInfo *info, hipStream_t s);

/* The debug views of a listed stream (dvo_tracker_views.hip): the residue histogram record, read back like TrackerInfo; the two BGR8
 * images stay in HBM */
#define DVO_VIEW_HIST_BINS 260
struct TrackerViewRecord {
    unsigned hist[DVO_VIEW_HIST_BINS];      /* hist[(int)eps_i + 1] over every point of the list (processResidueHistogram, SolveDVO.cpp:1403-1410) */
    int n_points, level;
};
/* TWO launches over entries [0, count) of the list: entries below n_aligned whose (out[i].event >= 2) == switched, and -- with
 * switched = 0 -- the entries from n_aligned on (streams on their first frame: backgrounds and the zero record only).  Stream p's images
 * are written at views + p * view_stride (reprojections on the distance transform) and views + view_plane + p * view_stride (residue
 * heat map on the grey image of frame-store slot slots[i], column-major at grey + slot * grey_npx); view_stride is a multiple of 4 */
hipError_t launch_tracker_views(const TrackerEntry *list, const TrackerOut *out, const int *slots, int n_aligned, int count, int switched,
                                const double *poses, const LevelSlab &L, int level, const Intrinsics &K, bool use_p4,
                                const unsigned char *grey, size_t grey_npx, unsigned char *views, size_t view_stride, size_t view_plane,
                                TrackerViewRecord *rec, hipStream_t s);

/* ---- key-frame archive of the multi-stream tracker (dvo_tracker_archive.hip; include/dvo_amd.h "key-frame archive") ----------
 * A ring of slots in HBM.  Slot s holds, per level l, a reference list in the forms the index-list alignment reads -- the compact
 * 8-byte points, their 4-byte twins with chunk headers and the twins' validity -- plus cidx (block order -> the 3 x N list's order, for
 * dvo_tracker_archive_get_points), the counts, the camera model the list was enlisted under, the stream and the frame number. */
struct ArchiveHeader {
    int N[DVO_LEVELS];
    int pt4_ok[DVO_LEVELS];
    float4 K;                 /* fx, fy, cx, cy */
    int stream, pad_;
    long long frame;
};
struct ArchiveLevel {         /* slot s at base + s * cap (chdr: s * (cap / 64)); cap is a multiple of 64 */
    uint2 *cpts;
    unsigned *cidx, *cpt4, *chdr;
    int cap, pad_;
};
struct ArchiveView {
    ArchiveLevel l[DVO_LEVELS];
    ArchiveHeader *hdr;
    int n_levels, n_slots;
};
struct ArchiveStore { int pair, slot; long long frame; float4 K; };      /* pair's reference lists -> slot */
/* ONE launch: for every entry the lists of pair e.pair of `src` (every level below A.n_levels) go to slot e.slot.  A list longer than
 * the slot's capacity is the host's to refuse beforehand; the kernel clamps all the same */
hipError_t launch_archive_store(const ArchiveStore *entries, int count, const LevelSet &src, const ArchiveView &A, hipStream_t s);
/* a slot's list of one level as the 3 x N floats of dvo_get_ref_level: xyz[3 * cidx[i] ..] = the expanded compact point i */
hipError_t launch_archive_decode(const ArchiveView &A, int slot, int level, float *xyz, int capacity, hipStream_t s);
/* one candidate of dvo_tracker_match: slot -> the reference lists of pair `dst` of the match context, the now levels of pair `now_pair`
 * of the tracker's context -> those of `dst`, pose -> dst's device pose */
struct ArchiveLoad {
    int slot, now_pair, dst, tex_mask;      /* tex_mask bit l: the host knows that the 16-byte texels of level l are real (no compact form, or a partial or refused one); bit 8 + l: it does not know, the destination has memory and the device decides (pal_n) */
    double pose[12];
};
/* ONE launch for all candidates and levels.  dst_* are the match context's slabs (same level geometry as `now`); dst_K may be NULL */
struct ArchiveDst {
    struct Lv {
        uint2 *cpts; unsigned *cidx, *cpt4, *chdr; int *pt4_ok, *N; int pt_cap;
        int tex_dense;        /* every pair's 16-byte texels have memory behind them (a sparse slab: only where tex_mask says so) */
        float4 *tex; unsigned *p4; float2 *pal; int *pal_n;
    } l[DVO_LEVELS];
    double *poses;
    float4 *pair_K;
};
hipError_t launch_archive_load(const ArchiveLoad *cands, int count, const ArchiveView &A, const LevelSet &now, const ArchiveDst &dst, hipStream_t s);
/* the score of a candidate: the engine's accumulators of slot `slot`'s list of one level against the now level of pair `now_pair`, at
 * the pose poses + 12 * pose_idx narrowed to float */
struct ScoreCand { int slot, now_pair, pose_idx, pad_; };
struct ScoreRecord {
    double H[21];             /* upper triangle of sum w J J^T, row-major */
    double g[6];
    double sum_eps2;
    int n_visible, n_points;
};
/* ONE launch, one 512-thread workgroup per candidate (dvo_tracker_info.h: the walk of the information kernel) */
hipError_t launch_archive_score(const ScoreCand *cands, int count, const double *poses, const ArchiveView &A, const LevelSlab &now, int level,
                                const Intrinsics &K, bool use_p4, ScoreRecord *out, hipStream_t s);

/* ---- depth verification of a candidate (dvo_tracker_verify.hip; include/dvo_amd.h "depth verification") -----------------------
 * The depth plane of one pyramid level in the frame store: slot f at depth + f * npx, column-major float millimetres */
struct VerifyDepth {
    const float *depth;
    size_t npx;
    int n_slots, rows, cols, pad_;
};
/* slot `slot`'s list against the depth plane of frame-store slot `frame_slot`, at the pose poses + 12 * pose_idx narrowed to float */
struct VerifyCand { int slot, frame_slot, pose_idx, pad_; };
struct VerifyTol { float tol_mm, tol_rel, min_depth_mm, max_depth_mm; };      /* the layout of dvo_tracker_verify_params */
/* the layout of dvo_tracker_verify_record: integers only, one value whatever the order of the reduction */
struct VerifyRecord {
    int n_points, n_visible, n_depth, n_agree, n_front, n_behind;
    unsigned long long sum_abs_q4;      /* sum over agreeing points of (unsigned)(min(|r|, 65535) * 16): 1/16 mm */
};
/* ONE launch, one 512-thread workgroup per candidate.  A candidate whose indices are outside A.n_slots / D.n_slots gets the zero record */
hipError_t launch_archive_verify(const VerifyCand *cands, int count, const double *poses, const ArchiveView &A, const VerifyDepth &D, int level,
                                 const Intrinsics &K, const VerifyTol &T, VerifyRecord *out, hipStream_t s);

/* ---- place descriptors of the archive (dvo_tracker_places.hip; include/dvo_amd.h "place descriptors") -------------------------
 * One descriptor per archived key frame beside the ring: row s of `desc` belongs to slot s, `stride` bytes (a multiple of 16) of
 * which the first D = rows * cols of the descriptor level are the brightness-normalised grey image and the rest is 128.  mark[s] != 0:
 * the row holds the descriptor of the slot's current key frame. */
#define DVO_PLACE_MAX_D 19200       /* 120 x 160: a distance stays below 2^23, a tile of PLACE_TQ query rows fits the LDS */
#define DVO_PLACE_NONE 0xFFFFFFFFu  /* the distance of an excluded slot */
struct PlaceView {
    unsigned char *desc;
    int *mark;
    int n_slots, stride, D, pad_;
};
/* the grey image of one pyramid level in the frame store: slot f at grey + f * npx, column-major bytes */
struct PlaceGrey {
    const unsigned char *grey;
    size_t npx;
    int n_slots, pad_;
};
struct PlaceEntry { int frame_slot, row; };       /* frame-store slot -> descriptor row (= archive slot) */
/* ONE launch, one workgroup per entry: the descriptor of frame-store slot e.frame_slot -> row e.row, mark[e.row] = 1.  An entry whose
 * indices are outside G.n_slots / P.n_slots is skipped */
hipError_t launch_place_store(const PlaceEntry *entries, int count, const PlaceGrey &G, const PlaceView &P, hipStream_t s);
/* one query: the current frame of a stream against the archive */
struct PlaceQuery {
    int frame_slot;           /* frame-store slot of the stream's current frame */
    int stream;
    int own_slot;             /* archive slot of the stream's current key frame, -1: none */
    int pad_;
    long long frame;          /* the current frame's number */
    float4 K;                 /* the stream's camera model: slots under another one are excluded */
};
/* what the selection writes per query and rank: the layout of dvo_tracker_place */
struct PlaceOut { long long key_id, frame; int stream; unsigned distance; };
/* TWO launches.  The first computes the queries' descriptors in LDS (the code of the store's kernel) and writes the n x P.n_slots
 * matrix `dist` of distances, DVO_PLACE_NONE for a slot that is empty, has no descriptor or is excluded for the query (another camera
 * model; own_slot; the query's own stream with frame - slot frame < min_gap, min_gap > 0).  The second, one workgroup per query, picks
 * the k smallest (distance, id) of the row: out[q * k + j], then n_found[q]; the rest of a row is {-1, -1, -1, DVO_PLACE_NONE}.
 * Slot s holds id id_base + ((s - id_base) mod n_slots), id_base = next id - n_slots. */
hipError_t launch_place_query(const PlaceQuery *queries, int n, int k, long long min_gap, long long id_base, const PlaceGrey &G,
                              const PlaceView &P, const ArchiveHeader *hdr, unsigned *dist, PlaceOut *out, int *n_found, hipStream_t s);

/* the shift search of dvo_tracker_place_shifts: archive slot `slot`'s stored row against the descriptor of frame-store slot `frame_slot` */
#define DVO_PLACE_SHIFT_MAX_R 8     /* == DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS */
struct PlaceShiftCand { int slot, frame_slot; };
/* the layout of dvo_tracker_place_shift */
struct PlaceShiftOut { int dy, dx; unsigned sad, sad_zero, sad_second; int area; };
/* ONE launch, one workgroup per candidate: the table of the (2 radius + 1)^2 SADs over the window of rows x cols (rows * cols == P.D,
 * column-major) in LDS, then the best shift under the order (SAD, |dy| + |dx|, dy, dx) and the smallest SAD at Chebyshev distance >= 2
 * from it.  A candidate whose indices are outside P.n_slots / G.n_slots, or a geometry that does not fit, leaves its record unwritten */
hipError_t launch_place_shifts(const PlaceShiftCand *cands, int n, int rows, int cols, int radius, const PlaceGrey &G, const PlaceView &P,
                               PlaceShiftOut *out, hipStream_t s);

/* ---- export and import of the archive (dvo_tracker_archive_blob.hip; the blob's format: dvo_archive_blob.h) --------------------
 * One key frame of a blob: record `record` of the table, its payload at payload_offset, and the slot of the ring it comes from (export)
 * or goes to (import; -1: it is not copied).  N are the counts the payload is laid out with. */
struct BlobEntry {
    long long origin_id, origin_frame;
    unsigned long long payload_offset, payload_bytes;
    int slot, origin_stream;
    int has_desc;             /* export: the slot's descriptor is written; import: the payload's descriptor is taken */
    int record;
    int N[DVO_LEVELS];
};
/* ONE launch: the listed slots -> the payloads and the records of the table in `blob` (a device buffer; the host has zeroed the table:
 * the payload checksums are added into it).  The header is the host's */
hipError_t launch_archive_export(const BlobEntry *entries, int count, const ArchiveView &A, const PlaceView &P, unsigned char *blob, hipStream_t s);
/* ONE launch: sums[i] += the checksum of entry i's payload in `blob` (the host has zeroed sums) */
hipError_t launch_archive_blob_sums(const BlobEntry *entries, int count, const unsigned char *blob, unsigned long long *sums, hipStream_t s);
/* ONE launch: the payloads of the entries with slot >= 0 -> their slots: lists, ArchiveHeader (stream -1) and, where P has descriptors,
 * the slot's descriptor row and mark (mark 0 for an entry without has_desc) */
hipError_t launch_archive_import(const BlobEntry *entries, int count, const unsigned char *blob, const ArchiveView &A, const PlaceView &P,
                                 hipStream_t s);

}  // namespace dvo
#endif
