/*
 * dvo_amd.h -- C ABI of the MI355X-native dense RGB-D edge-alignment engine.
 *
 * Drop-in boundary for ONE hot path of mpkuse/rgbd_odometry: the per-level pose
 * iteration loop SolveDVO::runIterations and its coarse-to-fine schedule.  The
 * reference has no plugin / FFI layer; the seam is the private method
 *   SolveDVO::runIterations          include/SolveDVO.h:228-230, src/SolveDVO.cpp:619-1017
 * and its helpers
 *   computeJacobianOfNowFrame        include/SolveDVO.h:312,     src/SolveDVO.cpp:306-414
 *   getReprojectedEpsilons           include/SolveDVO.h:313,     src/SolveDVO.cpp:425-462
 * called from SolveDVO::loop (src/SolveDVO.cpp:2097-2104, :2220-2227) and
 * casualTestFunction (:2426).  INTEGRATION.md shows the patch that makes the
 * reference's SolveDVO call these entry points.
 *
 * Conventions (identical to the reference's Eigen members):
 *   - images are COLUMN-major rows x cols float32, element (yy,xx) at yy + xx*rows
 *     (Eigen::MatrixXf; now_distance_transform / now_DT_gradientX/Y, SolveDVO.h:279-282)
 *   - reference edge points are 3 x N column-major float32 in metres
 *     (SpaceCordList, SolveDVO.h:137,304), in the column-major scan order of
 *     enlistRefEdgePts (SolveDVO.cpp:237-239)
 *   - pose is (R 3x3 column-major double, t 3 double), "now in ref":
 *     P_now = R^T (P_ref - t)  (SolveDVO.cpp:330); in/out like cR,cT
 *   - intrinsics are the LEVEL-0 K; level l uses diag(s,s,1)*K, s = 2^-l (:334-337)
 *
 * Ownership: the caller owns every host buffer (borrowed for the duration of the
 * call); the context owns all device memory.  One context per host thread and
 * HIP stream; calls on one context are not re-entrant.
 * Errors: int status (0 = DVO_OK); dvo_last_error() gives the message.  The
 * reference's behaviour on the same conditions is assert->abort (SolveDVO.h:124).
 * There is NO CPU fallback: without a HIP device every compute entry point
 * returns DVO_ERR_NO_DEVICE.
 */
#ifndef DVO_AMD_H_
#define DVO_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVO_MAX_LEVELS 8
#define DVO_NUM_ACC 29      /* 21 H (upper triangle, row-major) + 6 g + sum eps^2 + n_visible */

enum {
    DVO_OK = 0,
    DVO_ERR_INVALID = 1,     /* bad argument */
    DVO_ERR_NO_DEVICE = 2,   /* no HIP device / runtime */
    DVO_ERR_HIP = 3,         /* HIP runtime error, see dvo_last_error */
    DVO_ERR_STATE = 4,       /* data for the requested pair/level not set */
    DVO_ERR_NOMEM = 5
};

/* flags for the align entry points */
enum {
    DVO_FLAG_FINAL_OUTPUTS = 1,   /* also produce finalEpsilons / finalReprojections (SolveDVO.cpp:1002-1003) */
    DVO_FLAG_IDENTITY_START = 2,  /* start from cR=I, cT=0 instead of the stored pose: what the reference does
                                     on a keyframe switch (SolveDVO.cpp:2210-2211); enqueue form only */
    DVO_FLAG_NORMAL_MATRIX = 4    /* also accumulate H = sum_i w_i J_i^T J_i (21 sums, double) in every iteration of the fused launch
                                     and keep it per iterate (dvo_get_level_normal_matrix): the other 21 of the "21+6" normal-equation
                                     accumulators.  The reference's update never forms H (SolveDVO.cpp:777 uses g only; the pattern is
                                     SolvePnP.cpp:168-182), so poses / energies are unchanged; costs throughput */
};

/* Every literal of SolveDVO::runIterations as a runtime parameter; defaults are
 * the reference's values (file:line in the comments). */
typedef struct dvo_params {
    double beta;               /* heavy-ball BETA = 0.5                       SolveDVO.cpp:653 */
    double precond_rot;        /* PFactor = .5, P = diag(1,1,1,.5,.5,.5)      :724-730 */
    double reg_lambda;         /* regularizationLambda = 0.05                 :742 */
    double step_a;             /* 9.0     stepLength = 9.0*1.0E-2/(...)       :773 */
    double step_b;             /* 1.0E-2                                      :773 */
    int    step_decay_after;   /* 5  : (itr>5) ? (itr-4) : 1                  :773 */
    int    step_decay_offset;  /* 4                                           :773 */
    float  trust_radius;       /* trustRegionHyperSphereRadius = 0.003 (float member) :25 */
    float  psi_norm_stop;      /* psiNormTerminationThreshold  = 1.0E-7 (float member) :24 */
    int    enable_rotationize; /* __ENABLE_ROTATIONIZE__       SolveDVO.h:107 */
    int    enable_l2_reg;      /* __ENABLE_L2_REGULARIZATION   SolveDVO.h:112 */
    int    interpolate_dt;     /* __INTERPOLATE_DISTANCE_TRANSFORM (off in the reference, SolveDVO.h:97): eps from
                                  SolveDVO::interpolate (:1285-1308) instead of the nearest lookup (:446) */
    int    block_threads;      /* engine tuning: threads per workgroup of the fused kernel (256/512/1024; 0 = chosen from the
                                  point-list sizes and the batch size) */
    int    points_in_flight;   /* engine tuning: reference points per lane and pipeline stage (1/2/4; 0 = default 1) */
    int    engine_variant;     /* engine tuning / diagnostics: 0 = auto; 1 = always the one-point-per-lane fused kernel;
                                  2 = packed kernel, but never stage a now level into LDS; 3 = packed kernel with every wave
                                  forced through its literal-division fallback (tests); 4 = packed kernel, but never the
                                  compact form of a now level (dvo_now_prepare); 5 = packed kernel with every iteration's energy
                                  taken from the exact sweep (dvo_get_level_energy_sweeps; tests); 6 = packed kernel, but 4-byte
                                  reference points keep their block-relative form in LDS (dvo_get_level_points4_direct; tests) */
    int    lds_point_bytes;    /* engine tuning: LDS bytes per workgroup for the level's resident point list
                                  (0 = auto from block_threads, < 0 = none) */
    int    debug_alias_mod;    /* diagnostics only: if > 0, pair p reads the inputs of pair p % debug_alias_mod
                                  (shrinks the HBM working set without changing the arithmetic); 0 = off */
    int    canny_threshold1;   /* cv::Canny(img, edge, 150, 100, 3, true): the two thresholds (order-free, the detector */
    int    canny_threshold2;   /* swaps them), SolveDVO.cpp:1704,1764; used by the dvo_frame* entry points; 0,0 = 150,100 */
    int    team_size;          /* engine tuning: workgroups per frame pair of the fused launch when there are fewer pairs than compute
                                  units (each takes a contiguous share of every level's points; sums exchanged through L2 once per
                                  iteration, identical update on every member).  0 = auto (from the point counts and the number of pairs:
                                  at most 32 = one XCD; a single pair with >= 100 k points: 64 / 128 over all XCDs, two-stage exchange),
                                  1 = off, k = force k (<= 32, or 64 / 128 / 256 for a single pair) */
} dvo_params;

typedef struct dvo_ctx dvo_ctx;

/* ---- lifecycle ------------------------------------------------------------ */
int  dvo_params_default(dvo_params *p);
/* One frame pair, current HIP device.  Mirrors constructing a SolveDVO (SolveDVO.cpp:5-70). */
int  dvo_create(const dvo_params *p, dvo_ctx **out);
/* n_pairs independent frame pairs resident at once (batch / throughput mode). */
int  dvo_create_batch(const dvo_params *p, int n_pairs, dvo_ctx **out);
int  dvo_destroy(dvo_ctx *ctx);
const char *dvo_last_error(const dvo_ctx *ctx);      /* ctx may be NULL: last creation error */
int  dvo_num_pairs(const dvo_ctx *ctx);
/* Launch on an existing HIP stream (hipStream_t as void*; NULL = the HIP null stream, which is
 * what torch.cuda.current_stream().cuda_stream reports for torch's default stream).
 * dvo_use_own_stream() switches back to the context's private non-blocking stream. */
int  dvo_set_stream(dvo_ctx *ctx, void *hip_stream);
int  dvo_use_own_stream(dvo_ctx *ctx);
int  dvo_synchronize(dvo_ctx *ctx);
/* Single camera stream (the reference's loop: one frame every ~30 ms, SolveDVO.cpp:1945): between frames the GPU is idle.  A
 * process that only ever submits such sparse work can find the GPU parked at its lowest clocks and never raise them -- every
 * 0.5 ms alignment then takes 15-30 ms (measured: profiles/r03_single_stream).  dvo_set_keep_warm2 starts a host thread of the
 * context that keeps ONE wave busy on a stream of its own: launches of busy_us microseconds of real time, pause_us apart
 * (pause_us = 0: back to back); busy_us = 0 stops it.  dvo_set_keep_warm(period_us) = a 5 us launch every period_us.  Off by
 * default: a batch workload never idles.  DVO_KEEP_WARM="busy_us,pause_us" in the environment switches it on for every new
 * context.  (The alternative is an administrator pinning the performance level with rocm-smi; this needs no privileges.) */
int  dvo_set_keep_warm2(dvo_ctx *ctx, int busy_us, int pause_us);
int  dvo_set_keep_warm(dvo_ctx *ctx, int period_us);

/* ---- inputs ----------------------------------------------------------------
 * setCameraMatrix (SolveDVO.cpp:88-126): level-0 fx, fy, cx, cy as floats. */
int  dvo_set_intrinsics(dvo_ctx *ctx, float fx, float fy, float cx, float cy);

/* _ref_edge_3d[level] (SolveDVO.h:304) of pair `pair`: 3 x N floats. */
int  dvo_set_ref_level(dvo_ctx *ctx, int level, const float *xyz_3xN, int N);
int  dvo_set_ref_level_pair(dvo_ctx *ctx, int pair, int level, const float *xyz_3xN, int N);

/* now_distance_transform / now_DT_gradientX / now_DT_gradientY [level]
 * (SolveDVO.h:279-282), column-major rows x cols.  All pairs of one context
 * must use the same rows x cols per level. */
int  dvo_set_now_level(dvo_ctx *ctx, int level, const float *dt, const float *gx, const float *gy,
                       int rows, int cols);
int  dvo_set_now_level_pair(dvo_ctx *ctx, int pair, int level, const float *dt, const float *gx,
                            const float *gy, int rows, int cols);
/* Same, from DEVICE pointers (e.g. torch tensors); asynchronous on the context stream. */
int  dvo_set_ref_level_device(dvo_ctx *ctx, int pair, int level, const float *d_xyz_3xN, int N);
int  dvo_set_now_level_device(dvo_ctx *ctx, int pair, int level, const float *d_dt, const float *d_gx,
                              const float *d_gy, int rows, int cols);

/* computeDistTransfrmOfNow after the Canny step (SolveDVO.cpp:1768-1795) + imageGradient (:1063-1098) on
 * the GPU: edge (uint8, >0 = edge pixel, column-major rows x cols, host pointer) -> exact Euclidean
 * distance transform -> cv::normalize(0,255,NORM_MINMAX) (:1774) -> [-.5 0 .5] gradients with a
 * reflect-101 border (:1077-1090) -> resident now level.  1 byte per pixel crosses PCIe instead of 12.
 * (the Canny detector itself stays with the caller.) */
int  dvo_set_now_level_from_edges(dvo_ctx *ctx, int pair, int level, const unsigned char *edge, int rows, int cols);
/* The planar DT / gradient images of a resident now level (host outputs, rows*cols floats each, any may
 * be NULL). */
int  dvo_get_now_level(dvo_ctx *ctx, int pair, int level, float *dt, float *gx, float *gy);

/* The resident reference point list of a level (3 x N floats, host output of `capacity` points; *N_out = N). */
int  dvo_get_ref_level(dvo_ctx *ctx, int pair, int level, float *xyz_out, int capacity, int *N_out);

/* Batch set-up helper: pair slot p in [dst_first, dst_first+dst_count) becomes a device-side copy of
 * pair (p - dst_first) % n_src (all levels that are set), one launch per level.  dst_first = 0 leaves the
 * sources in place and fills the rest of the range cyclically. */
int  dvo_replicate_pairs(dvo_ctx *ctx, int n_src, int dst_first, int dst_count);

/* selectedPts + enlistRefEdgePts (SolveDVO.cpp:1230-1264, :224-264) on the GPU:
 * edge (int32, >0 = edge) and depth_mm (f32), column-major rows x cols, host
 * pointers.  Builds the 3xN list in the reference's column-major scan order and
 * installs it as the ref level of `pair`.  xyz_out / uv_out (host, capacity
 * points) may be NULL.  *N_out receives N. */
int  dvo_set_ref_level_from_images(dvo_ctx *ctx, int pair, int level, const int32_t *edge,
                                   const float *depth_mm, int rows, int cols,
                                   float *xyz_out, float *uv_out, int capacity, int *N_out);

/* ---- the hot path -----------------------------------------------------------
 * SolveDVO::runIterations (SolveDVO.cpp:619-1017) for pair 0.
 *   R[9], t[3]        in/out   cR, cT
 *   energy[max_iters] out      energyAtEachIteration (zero after an early exit, :634)
 *   final_eps[N]      out/NULL finalEpsilons
 *   final_reproj[3N]  out/NULL finalReprojections (3 x N column-major, row 2 = z*(1/z))
 *   best_idx          out      bestEnergyIndex (-1 if no iterate was accepted)
 *   visible_ratio     out      finalVisibleRatio */
int  dvo_run_iterations(dvo_ctx *ctx, int level, int max_iters, double *R, double *t,
                        float *energy, float *final_eps, float *final_reproj,
                        int *best_idx, float *visible_ratio);
int  dvo_run_iterations_pair(dvo_ctx *ctx, int pair, int level, int max_iters, double *R, double *t,
                             float *energy, float *final_eps, float *final_reproj,
                             int *best_idx, float *visible_ratio);

/* The level schedule of SolveDVO::loop (SolveDVO.cpp:2097-2104) fused into one
 * launch: for f = n_levels-1 .. 0: if iters[f] > 0: runIterations(f, iters[f], R, t).
 * Synchronous; R (9*n_pairs) and t (3*n_pairs) are in/out for pairs
 * [first_pair, first_pair+n_pairs). */
int  dvo_align_pyramid(dvo_ctx *ctx, int n_levels, const int *iters, int flags, double *R, double *t);
int  dvo_align_batch(dvo_ctx *ctx, int first_pair, int n_pairs, int n_levels, const int *iters,
                     int flags, double *R, double *t);

/* Asynchronous form: poses stay device-resident between calls (the reference
 * carries cR_64/cT_64 from frame to frame, SolveDVO.cpp:2102). */
int  dvo_set_poses(dvo_ctx *ctx, int first_pair, int n_pairs, const double *R, const double *t);
int  dvo_align_batch_enqueue(dvo_ctx *ctx, int first_pair, int n_pairs, int n_levels,
                             const int *iters, int flags);
int  dvo_get_poses(dvo_ctx *ctx, int first_pair, int n_pairs, double *R, double *t);   /* synchronises */
/* The same with every rotation written row by row: R_rows[9*p + 3*i + j] is element (i, j) of pair first_pair + p (dvo_get_poses
 * and every other entry point store R column-major).  For callers that keep row-major matrices: no transpose afterwards. */
int  dvo_get_poses_rows(dvo_ctx *ctx, int first_pair, int n_pairs, double *R_rows, double *t);

/* Per-level outputs of the last align call for `pair` (synchronises).
 * energy: iters[level] floats; any pointer may be NULL. */
int  dvo_get_level_report(dvo_ctx *ctx, int pair, int level, float *energy, int n_energy,
                          int *best_idx, float *visible_ratio);
/* H = sum_i w_i J_i^T J_i (6x6 symmetric, row-major, tangent order [translation(3), rotation(3)] like psi) at iterate
 * `itr` of `level` of the last align call made with DVO_FLAG_NORMAL_MATRIX; itr < 0 = the best iterate (:696).  With g
 * (not kept) it is the Gauss-Newton system of the reference's residual; H^-1 scaled by the residual variance is the usual
 * covariance estimate of the aligned pose. */
int  dvo_get_level_normal_matrix(dvo_ctx *ctx, int pair, int level, int itr, double *H36);
/* finalEpsilons / finalReprojections of the last level run (needs DVO_FLAG_FINAL_OUTPUTS). */
int  dvo_get_final_outputs(dvo_ctx *ctx, int pair, float *final_eps, float *final_reproj, int capacity,
                           int *N_out);

/* ---- host-driven iteration: one very large frame, or one frame tiled over several GPUs --------
 * runIterations (SolveDVO.cpp:619-1017) opened up at the only point where its per-point work
 * couples: the sum.  Per iteration the caller runs
 *     dvo_iter_accumulate(points [first, first+n) of this GPU's shard) -> 32 doubles on the device
 *     [all-reduce of those doubles over the GPUs that share the frame: RCCL, ncclSum]
 *     dvo_iter_update(the reduced sums)        -- the reference's 6-DoF update, on the device
 * The grid of the accumulate kernel spans all CUs, so this is also the path for frames whose
 * point lists are too long for one workgroup (1920x1080, 4096x3072).  All calls except
 * dvo_iter_begin/_end are asynchronous on the context stream.
 *   d_acc32: DEVICE pointer to 32 doubles: [0..20] H upper triangle, [21..26] g, [27] sum eps^2 as this GPU added it,
 *            [28] visible points, [29..31] the three 32-bit limbs of the EXACT sum of eps^2 (integers below 2^53 on a grid of
 *            2^-68: sums of them over shards are exact in any order; dvo_iter_update rounds the exact total once and takes the
 *            energy from that -- the same float on every rank and for every sharding; [27] is used only if a residual was
 *            outside [2^-11, 2^12), which no normalised distance is).
 *   n_total: number of reference points of the level over ALL shards (visible ratio, :457).
 * After an early termination (:877) later dvo_iter_update calls are no-ops, like the reference's break. */
int  dvo_iter_begin(dvo_ctx *ctx, int pair, int level, int max_iters, const double *R, const double *t);
int  dvo_iter_accumulate(dvo_ctx *ctx, int pair, int level, int first_point, int n_points, double *d_acc32);
int  dvo_iter_update(dvo_ctx *ctx, int pair, int level, int itr, int n_total, const double *d_acc32);
int  dvo_iter_end(dvo_ctx *ctx, int pair, int level, double *R, double *t, float *energy /*[max_iters] or NULL*/,
                  int *best_idx, float *visible_ratio);

/* The same loop for ONE GPU, enqueued from C: the level schedule of SolveDVO::loop with every iteration
 * spread over all CUs (frames whose point lists are too long for one workgroup).  Synchronous; per-level
 * energies / best index / ratio afterwards through dvo_get_level_report.  flags: DVO_FLAG_FINAL_OUTPUTS
 * (finalEpsilons / finalReprojections of the last level, SolveDVO.cpp:703-704, :1002-1003 -> dvo_get_final_outputs) and / or
 * DVO_FLAG_NORMAL_MATRIX (H = sum w J J^T of every iterate -> dvo_get_level_normal_matrix; + 40 % on every launch).
 * One launch per iteration (the update of an iteration rides at the head of the next launch), replayed as a graph. */
int  dvo_align_pyramid_wide(dvo_ctx *ctx, int pair, int n_levels, const int *iters, int flags, double *R, double *t);

/* ---- tiled mode from C: one large frame sharded over the GPUs of a node (BASELINE configs[4]) ----------
 * The same loop with the all-reduce done by RCCL over xGMI and everything enqueued from C on the context stream -- what a
 * C++ node calls (one process or thread per GPU, each with its own context and its rank's ncclComm_t):
 *     dvo_tiled_attach(ctx, comm, rank, world, NULL);           once
 *     dvo_align_pyramid_tiled(ctx, 0, n_levels, iters, flags, R, t);   per frame pair; every rank gets the same pose
 * Each rank must hold the SAME inputs for `pair` (full reference lists and now pyramid); rank r processes the contiguous
 * index range r of every level's list, the 32 sums are all-reduced (ncclDouble, ncclSum) per iteration, and every rank
 * executes the identical update.  nccl_comm: the caller's ncclComm_t.  rccl_library: path of the RCCL library the
 * communicator was created with; NULL = the RCCL already loaded in the process, else librccl.so.1.  libdvo_amd.so has no
 * link-time dependency on RCCL.  Replaces the reference seam include/SolveDVO.h:228-230 for frames one GPU cannot hold
 * or does not finish fast enough (break-even: DESIGN.md section 5). */
int  dvo_tiled_attach(dvo_ctx *ctx, void *nccl_comm, int rank, int world, const char *rccl_library);
int  dvo_tiled_detach(dvo_ctx *ctx);
/* flags: DVO_FLAG_FINAL_OUTPUTS and / or DVO_FLAG_NORMAL_MATRIX (H = sum w J J^T travels in the same 32 all-reduced doubles and is
 * kept per iterate: dvo_get_level_normal_matrix; without it the 21 slots are zeros).  One kernel + one ncclAllReduce per
 * iteration, the whole schedule captured once and replayed as a graph (dvo_tiled_graph_replayed).
 * With DVO_FLAG_FINAL_OUTPUTS every rank computes finalEpsilons / finalReprojections (SolveDVO.cpp:703-704,
 * :1002-1003) of ITS shard of the last level's list, at the points' own indices: dvo_get_final_outputs then returns arrays in
 * which only [first, first + count) of dvo_tiled_shard is filled in on this rank -- the caller concatenates the shards
 * (SURVEY.md 8e).  Thread safety: contexts of different GPUs may be driven from different host threads of one process
 * (each entry point makes the context's device current; the attachment registry is locked); one context is still
 * one-thread-at-a-time. */
int  dvo_align_pyramid_tiled(dvo_ctx *ctx, int pair, int n_levels, const int *iters, int flags, double *R, double *t);
/* the contiguous index range of `level`'s reference list this rank works on */
int  dvo_tiled_shard(dvo_ctx *ctx, int pair, int level, int *first, int *count);
/* inspection: *graph_replayed = 1 if the last dvo_align_pyramid_tiled replayed its captured graph (one kernel + one ncclAllReduce
 * per iteration, no host work in between), 0 if the schedule was submitted launch by launch (the runtime refused to capture the
 * collective, a world of more than one rank without DVO_TILED_GRAPH_MULTIRANK, or the legacy null stream) */
int  dvo_tiled_graph_replayed(dvo_ctx *ctx, int *graph_replayed);
/* inspection: bit l of *levels_mask = 1 if level l of the last dvo_align_pyramid_wide / _tiled schedule that was ENQUEUED (a replayed
 * graph keeps the mask of its capture) ran the packed two-points-per-lane step kernel over the compact list (round 5; lists built by
 * the engine's own reference-point kernels have one), 0 for the one-point-per-lane kernel over the 3 x N list (caller-supplied
 * lists, dvo_params.interpolate_dt);
 * *solo_mask (may be NULL): the levels among them that ran as ONE launch of one workgroup for all their iterations (levels of at most
 * DVO_TILED_SOLO_MAX = 6144 points; over several ranks every rank runs such a level whole, without a collective) */
int  dvo_wide_packed_levels(dvo_ctx *ctx, int *levels_mask, int *solo_mask);
/* round 6: *levels_mask = the levels of the last dvo_align_pyramid_wide that ran inside ONE launch of the fused kernel in team mode (the
 * coarse levels of a large frame: levels of at most DVO_WIDE_TEAM_MAX = 200 000 points from the coarsest down, when finer ones remain for
 * the step launches); 0 when the schedule ran as step launches only */
int  dvo_wide_team_levels(dvo_ctx *ctx, int *levels_mask);

/* ---- inspection (used by the parity tests) ---------------------------------
 * One evaluation of computeJacobianOfNowFrame + getReprojectedEpsilons at the
 * given pose (cast to float exactly as SolveDVO.cpp:673-674).  Host outputs, any
 * may be NULL: reproj 3xN, J Nx6 row-major, eps[N], w[N], visible[N]. */
int  dvo_eval_points(dvo_ctx *ctx, int pair, int level, const double *R, const double *t,
                     float *reproj, float *J, float *eps, float *w, int *visible);
/* The 29 accumulators of one iteration at the given pose:
 * acc[0..20] = upper triangle of sum_i w_i J_i J_i^T, acc[21..26] = g = J^T W eps
 * (SolveDVO.cpp:777), acc[27] = sum eps_i^2 (the correctly rounded exact sum: no order of additions enters), acc[28] = number of
 * visible points. */
int  dvo_accumulate(dvo_ctx *ctx, int pair, int level, const double *R, const double *t,
                    double *acc29);
/* Device SE(3) helpers exposed for property tests (same code the kernels use). */
int  dvo_device_se3_exp(dvo_ctx *ctx, const double *psi6, double *R, double *t);
int  dvo_device_se3_log(dvo_ctx *ctx, const double *R, const double *t, double *psi6);
int  dvo_device_rotationize(dvo_ctx *ctx, double *R);

/* Where the fused kernel read the now level of (pair, level) from in the last batch launch that used the packed kernel:
 * 0 = 16-byte texels gathered from HBM/L2, 1 = the level's texels staged once per level into LDS ("LDS-staged image
 * tiles": the reference re-copies the three images every iteration, SolveDVO.cpp:310,316-317,427) -- taken when the whole
 * level fits beside its point list; 2 = the level's compact form (below); -1 = not run.  Inspection / tests. */
int  dvo_get_level_texel_mode(dvo_ctx *ctx, int pair, int level, int *mode);
/* *ran = 1 if, at that level of that launch, a wave of the packed kernel took its literal-division fallback (a reference point
 * whose reprojected z left the range the fast reciprocal is proven exact on, or dvo_params.engine_variant = 3).  Tests. */
int  dvo_get_level_exact_fallback(dvo_ctx *ctx, int pair, int level, int *ran);
/* *n = the iterations of that level of that launch whose energy came from the exact sweep (round 6).  The energy is defined without an
 * order of summation: E = (float)sqrt(S), S = the correctly rounded double of the exact sum of eps^2 (SolveDVO.cpp:689, :1310-1312 is a
 * float norm whose order is Eigen's).  The packed kernel adds eps^2 in its own order and certifies that no order could have rounded to
 * another float; where it cannot (about N 2^-28 of the iterations of an N-point level) every wave sweeps the residuals once more into
 * exact 32-bit limbs.  dvo_params.engine_variant = 5 sends every iteration that way (tests).  The kernels whose sums travel between
 * launches or ranks (tiled mode) carry the limbs always: they report 0. */
int  dvo_get_level_energy_sweeps(dvo_ctx *ctx, int pair, int level, int *n);
/* *used = 1 if that level's reference points were read in their 4-byte form (engine detail: block-relative pixel + depth in
 * whole millimetres + chunk headers, validated bit for bit against the 8-byte list when the list is built; taken for lists
 * longer than what fits in LDS, where the per-iteration stream of the rest dominates the memory requests).  Tests. */
int  dvo_get_level_points4(dvo_ctx *ctx, int pair, int level, int *used);
/* *used = 1 if the part of that level's 4-byte points that lives in LDS was held there in the direct form (engine detail: pixel column
 * | pixel row << 10 | millimetres << 19, made once per level while the list is staged, so that the level's sweeps decode a point
 * without block arithmetic or chunk headers; the same float bits).  Taken when the now level has at most 1024 columns and 512 rows and
 * every staged depth is below 8192 mm; 0 otherwise, with dvo_params.engine_variant = 6, and wherever dvo_get_level_points4 says 0.
 * Tests. */
int  dvo_get_level_points4_direct(dvo_ctx *ctx, int pair, int level, int *used);
/* *fused = 1 if that level's final outputs (DVO_FLAG_FINAL_OUTPUTS, the last level of the schedule) were written by the level's last
 * sweep, at the best of the iterates before the last one, and the separate pass over the level was skipped because the last iterate
 * did not become the best (engine detail, the outputs are the same bits either way).  0 at every other level, after an early stop,
 * for a one-iteration level, with DVO_FLAG_NORMAL_MATRIX, and on the kernels other than the packed fused one.  Tests. */
int  dvo_get_level_final_fused(dvo_ctx *ctx, int pair, int level, int *fused);
/* Kept for the C ABI: always 0.  (Round 5 measured an LDS copy of a coarse level's whole rank image and did not take it.) */
int  dvo_get_level_ranks_in_lds(dvo_ctx *ctx, int pair, int level, int *used);

/* Shape the engine chose for the last fused (batch) launch: threads per workgroup (256: two workgroups per compute unit,
 * 512 / 1024: one), workgroups per frame pair (team mode, 1 = none), packed = 1: the two-points-per-lane kernel.  Inspection. */
int  dvo_get_last_launch_shape(dvo_ctx *ctx, int *block_threads, int *team_size, int *packed);
/* dvo_align_batch_enqueue walks every pair of its request to validate it and to plan the launch.  A context remembers what such a
 * full pass decided; a later call with the same range, schedule and flags, on a context none of whose inputs or settings were
 * written in between (poses and other device data do not count), goes straight to the launch.  Counted since creation: calls that
 * took the full pass, calls served from memory.  DVO_LAUNCH_MEMO in the environment when the context is made: off = never
 * remember, verify = every remembered launch is checked against a full pass (DVO_ERR_STATE on a difference).  Inspection. */
int  dvo_get_enqueue_counts(dvo_ctx *ctx, unsigned long long *full_passes, unsigned long long *memo_hits);

/* Compact form of resident now levels (engine detail, results are bit-identical with or without it).  The three images the
 * reference keeps per now level (dist transform :1768-1795, its imageGradient :1063-1098; the weight :1047-1053 is a function
 * of the first) are redundant: a pixel is described by the rank of its distance value among the image's distinct values and
 * the ranks of its four neighbours -- 4 bytes per pixel, 24 pixels per 128-byte memory line instead of 8: half the memory
 * requests of the alignment kernel.
 *   NATIVE (round 3): a now level produced by the engine's own distance transform (dvo_set_now_level_from_edges,
 *     dvo_frames_as_now, the now_first_pair argument of the upload calls) is written in this form and in no other: the integer
 *     squared distances are ranked through a presence bitmap (no hashing, sorting or verification pass), the 16-byte texels are
 *     never written (17 instead of 45 bytes of HBM traffic per pixel) and are decoded on demand for the entry points that read
 *     them (dvo_get_now_level, dvo_eval_points, the host-driven / tiled iteration).  Images the form cannot hold (more than
 *     8191 distinct distances, a pixel further than 511 pixels from every edge, a rank step beyond +-127) get 16-byte texels
 *     from the same launch instead.
 *   GENERIC: for caller-supplied float images (dvo_set_now_level) the engine derives the form from the 16-byte texels and
 *     VERIFIES per pixel that it reproduces {DT, gx, gy, w} bit for bit, keeping the 16-byte form for that pair and level
 *     otherwise (gradients that are not imageGradient(DT), more than 4095 distinct values, ...).  That build reads the level
 *     twice and costs about four and a half alignments of the same pair, so the engine makes it by itself only for a now level
 *     that has already been aligned DVO_COMPACT_NOW_AFTER times; dvo_now_prepare builds it now for the given pairs.
 * dvo_params.engine_variant = 4 (or DVO_COMPACT_NOW=off in the environment) disables both: 16-byte texels everywhere. */
#define DVO_COMPACT_NOW_AFTER 16
int  dvo_now_prepare(dvo_ctx *ctx, int first_pair, int count);
/* DIRECT (round 3): with on != 0, dvo_set_now_level / _pair / _device build the compact form from the three float images at
 * installation: the unit of a normalised exact distance transform is its smallest positive value s; d2 = round((DT / s)^2) per
 * pixel is accepted only if (float)sqrt(d2) * s reproduces DT bit for bit; the native builder's rank pass then writes the words,
 * and the caller's gx / gy are compared bit for bit with what the kernel will decode.  Any positive scale is accepted; a DT that
 * is no exact transform (-1) or gradients that are not imageGradient(DT) (-4) leave the pair on its 16-byte texels (written in
 * any case) and to the policy above.  Four single-image launches, about 40 us per 640x480 level -- against 98 us of PCIe for the
 * three images, or 4 us for the texels alone when they come from device memory: OFF by default, worth it only for a now level
 * that is aligned many times (DVO_DIRECT_COMPACT=on / off in the environment overrides the call). */
int  dvo_set_direct_compact(dvo_ctx *ctx, int on);
/* palette_size: > 0 number of palette entries of the compact form, 0 not built (yet / stale),
 * < 0 no compact form: -1 negative/inf/nan value, -2 too many distinct values (generic builder: 4095), -3 rank step beyond
 * +-127, -4 gradient is not imageGradient(DT), -5 weight is not getWeightOf(DT), -6 image narrower than 2 pixels, -7 a pixel
 * further than 511 pixels from every edge.  Round 5: the engine's own distance transform no longer refuses an image for -2 / -3 /
 * -7 -- it writes a PARTIAL compact form (the lowest 4094 ranks; the other pixels are looked up in the image's 16-byte texels,
 * which such an image also gets) and dvo_get_now_compact_partial says so; float images handed in directly keep those refusals. */
int  dvo_get_now_compact_info(dvo_ctx *ctx, int pair, int level, int *palette_size);
int  dvo_get_now_compact_partial(dvo_ctx *ctx, int pair, int level, int *partial);

/* Kept for the C ABI: the library has no phase cycle counters; fills out64[0..63] with zeros. */
int  dvo_debug_stamps(dvo_ctx *ctx, int pair, unsigned long long *out64);

/* ---- measurement support ------------------------------------------------------
 * Algorithmic (compulsory) bytes of one alignment of `pair` under the given
 * schedule: sum_l [12*rows*cols + 12*N_l] over levels with iters>0, + 16*N_last
 * when DVO_FLAG_FINAL_OUTPUTS. */
int  dvo_algorithmic_bytes(dvo_ctx *ctx, int pair, int n_levels, const int *iters, int flags,
                           uint64_t *bytes);
/* Sum over levels of iters[l]*N_l (point-iterations) for `pair`. */
int  dvo_point_iterations(dvo_ctx *ctx, int pair, int n_levels, const int *iters, uint64_t *count);

/* ---- frames in (SURVEY.md section 8f rows f1 + f2) ----------------------------------------------------
 * Everything between the camera / the RGBDFramePyd message and the hot path, on the GPU:
 *   row f2  camTopic2PublisherPyD.cpp:73-77,322-347   depth m -> mm u16 (0 -> 1), INTER_NEAREST pyramid, BGR2GRAY
 *   row f1  SolveDVO.cpp:1679-1799                     Canny(150,100,3,L2) -> distance transform -> normalise ->
 *                                                      gradients (now side); :1700-1712 + :1230-1264 + :224-264
 *                                                      Canny -> selectedPts -> enlistRefEdgePts (ref side)
 * A context holds a FRAME STORE of `n_slots` frames (grey, depth in mm, Canny edge map per level, all in
 * HBM).  A stored frame can be installed as the now frame and/or as the reference frame of any pair without
 * another upload -- what setRcvdFrameAsNowFrame / setRcvdFrameAsRefFrame / setPrevFrameAsRefFrame
 * (SolveDVO.cpp:535-618) do with host copies.  All slots share one pyramid geometry.
 * Frame-store calls are batched: `count` consecutive slots per call, one kernel launch per stage and level. */
enum { DVO_PIX_U8 = 0, DVO_PIX_U16 = 1, DVO_PIX_F32 = 2 };
enum { DVO_LAYOUT_COL_MAJOR = 0,    /* Eigen (im_n[level].data()): (yy,xx) at yy + xx*rows */
       DVO_LAYOUT_ROW_MAJOR = 1 };  /* cv::Mat / sensor_msgs::Image: (yy,xx) at yy*cols + xx */
enum { DVO_UPLOAD_ASYNC = 1,        /* do not wait for the copies: with DVO_UPLOAD_DIRECT the host buffers stay borrowed until dvo_synchronize() */
       DVO_UPLOAD_DEPTH_RAW = 2,    /* dvo_frames_upload_cameras: the depth images are already in sensor units (what a mono16 depth topic
                                       carries, as float): no x1000, no rounding, no 0 -> 1 -- what the rgbdSubsc node works on.
                                       Without an undistortion map every float is stored as it is (a NaN stays a NaN).  Under a map
                                       the remap's output is the publisher's 16-bit image, saturate_cast<ushort>(cvRound(sum of
                                       the four weighted taps)): a sum that is NaN (a NaN tap, even at weight 0), infinite or at or
                                       beyond 2^31 in magnitude yields 0, as cvRound's INT_MIN does; other sums round half to even
                                       and saturate to [0, 65535] */
       DVO_UPLOAD_DIRECT = 4 };     /* DMA straight out of the caller's buffers.  Only for buffers that are pinned, or at least never
                                       unmapped while the context lives (a pool the caller keeps).  Default (round 3): the images are first
                                       copied into the engine's own pinned mirror (~0.1 ms per 640x480 frame) and the caller's memory is
                                       free again when the call returns.  Why: the HIP runtime registers pageable source buffers with the
                                       driver; when the application later frees them (free -> munmap of a large block), the driver stalls
                                       the process's GPU queues for 14-33 ms -- measured on the C++ file replay, whose loader allocates
                                       and frees a pyramid per frame: 24 ms per frame instead of 0.6 (profiles/r03_single_stream) */
enum { DVO_UPLOAD_MAPPED = 16 };    /* dvo_frames_upload_cameras / _pyramids: the images sit in PINNED host memory the GPU can address (hipHostMalloc,
                                       hipHostRegister'ed + mapped, torch pin_memory): a kernel pulls them over PCIe -- one launch per 32
                                       images at the full link rate (56 GB/s measured) instead of one DMA per image (38 GB/s: the
                                       per-copy submission cost) -- in the same double-buffered chunks as the DMA path, so the pull of
                                       chunk k+1 overlaps the preprocessing of chunk k.  Borrowing rules as for DVO_UPLOAD_DIRECT */
/* Pinned host memory the GPU can address, for callers that do not link the HIP runtime themselves (a ROS node's image pool):
 * what DVO_UPLOAD_MAPPED wants.  NULL when the allocation fails.  Free with dvo_host_free_mapped, never with free(). */
void *dvo_host_alloc_mapped(size_t bytes);
void  dvo_host_free_mapped(void *p);
enum { DVO_UPLOAD_DEVICE = 8 };     /* dvo_frames_upload_cameras: the image pointers are DEVICE pointers of this context's GPU (a decoder or
                                       a camera driver that lands frames in HBM): device-to-device copies into the landing buffer, no PCIe.
                                       The buffers stay borrowed until the call returns (until dvo_synchronize() with DVO_UPLOAD_ASYNC) */

typedef struct dvo_image {          /* one single-channel host image */
    const void *data;
    int rows, cols;
    int dtype;                      /* DVO_PIX_* : grey U8 or F32 (values 0..255), depth U16 (mm) or F32 (mm) */
    int layout;                     /* DVO_LAYOUT_* */
} dvo_image;

/* (re)size the frame store; default on first use: min(2*n_pairs + 2, 64) slots */
int  dvo_frames_reserve(dvo_ctx *ctx, int n_slots);
/* the pyramids of `count` frames as the dvo node receives them (RGBDFramePyd: framemono[] mono8 + dframe[] mono16,
 * imageArrivedCallBack SolveDVO.cpp:490-534) or as the class holds them (im_n/dim_n: F32 column-major).
 * grey[f*n_levels + l], depth[f*n_levels + l]; depth may be NULL (frames that will only ever be "now" frames).
 * U16 depth gets the node's 0 -> 1 treatment (:514); F32 depth is taken as is.  Runs Canny per level.
 * now_first_pair >= 0: slot first_slot+i is also installed as the now frame of pair now_first_pair+i (as
 * dvo_frames_as_now would), chunk by chunk in the shadow of the next chunk's host-to-device copies; -1: no. */
int  dvo_frames_upload_pyramids(dvo_ctx *ctx, int first_slot, int count, int n_levels,
                                const dvo_image *grey, const dvo_image *depth, int now_first_pair, int flags);
/* cv::undistort of the pyramid publisher (camTopic2PublisherPyD.cpp:88-107, :306-308), applied to BOTH images of every
 * frame given to dvo_frames_upload_cameras from now on (the depth image after its conversion to 16-bit millimetres, as the
 * publisher does): K4 = fx, fy, cx, cy and D5 = k1, k2, p1, p2, k3 of the sensor_msgs/CameraInfo the publisher listens to
 * (:52-61), rows x cols = the camera's resolution.  OpenCV 2.4 semantics: fixed-point bilinear remap (5 fraction bits),
 * zero outside the source.  K4 = D5 = NULL switches it off again (the publisher's behaviour without a camera-info topic).
 * The map is built once per call on the host.
 * Refused with DVO_ERR_INVALID, the map in force unchanged: only one of K4 and D5, rows or cols < 1, fx or fy zero, any of the
 * nine numbers NaN or infinite.  A finite calibration that throws u*32 or v*32 of a pixel beyond an int gets cvRound's INT_MIN
 * there, like OpenCV 2.4 on x86: source pixel (0, 0) with fraction 0 after the cast to short. */
int  dvo_frames_set_undistort(dvo_ctx *ctx, int rows, int cols, const double *K4, const double *D5);
/* the same map on the host, no device and no context needed: xy[2 * (i*cols + j)] = {x, y} integer source pixel of output pixel
 * (i, j), frac[i*cols + j] = fy*32 + fx (5-bit fractions).  DVO_ERR_INVALID on the arguments dvo_frames_set_undistort refuses. */
int  dvo_undistort_map_host(int rows, int cols, const double *K4, const double *D5, short *xy, unsigned short *frac);
/* camera frames: full-resolution BGR8 (rows x cols x 3, row-major) + depth in metres (F32 row-major, may be NULL);
 * level l is decimated by 2^(first_shift + l) (the reference publishes first_shift = 1: 320x240 .. 40x30).
 * Builds the pyramid on the device, then as above. */
int  dvo_frames_upload_cameras(dvo_ctx *ctx, int first_slot, int count, const unsigned char *const *bgr8,
                               const float *const *depth_m, int rows, int cols, int n_levels, int first_shift,
                               int now_first_pair, int flags);
/* The same for camera frames in the formats sensors and ROS image topics deliver, converted in registers by the level kernels: no
 * BGR or float copy of a frame is made on the host or the device, and only the frame's real bytes cross the link (640x480: BGR8 + float
 * depth 2.15 MB, BGR8 + 16-bit depth 1.54 MB, mono8 + 16-bit depth 0.92 MB).  Each format is DEFINED by the (BGR8, float depth) input
 * it stands for; the stored levels are bit-equal to dvo_frames_upload_cameras on that input, with or without an undistortion map:
 *   DVO_CAM_BGR8    rows x cols x 3 bytes, row-major (bgr8)
 *   DVO_CAM_RGB8    rows x cols x 3 bytes (rgb8): BGR8 with channels 0 and 2 exchanged
 *   DVO_CAM_MONO8   rows x cols bytes (mono8): value g stands for BGR8 (g, g, g), whose grey value is g (1868 + 9617 + 4899 = 2^14);
 *                   under a map this is the 8-bit one-channel cv::undistort (the same BilinearTab_i weights, (sum + 2^14) >> 15)
 *   DVO_DEPTH_F32   float, row-major: metres, or sensor units with DVO_UPLOAD_DEPTH_RAW (dvo_frames_upload_cameras)
 *   DVO_DEPTH_U16   16-bit, row-major, ONE UNIT = ONE MILLIMETRE (mono16 of a PrimeSense-class driver; other scales, e.g. TUM's 5000
 *                   per metre, are not supported: rescale them before the upload).  Value v with DVO_UPLOAD_DEPTH_RAW stands for the
 *                   float (float)v with DVO_UPLOAD_DEPTH_RAW -- the mono16 image as the rgbdSubsc node receives it, holes stay 0;
 *                   without the flag it stands for (float)(v == 0 ? 1 : v) with DVO_UPLOAD_DEPTH_RAW -- the publisher's depth16
 *                   after setTo(1, depth16 == 0) (camTopic2PublisherPyD.cpp:77-78): 0 -> 1 before the remap, as on the metres path
 * image[i] / depth[i]: image i in image_format / depth_format (depth may be NULL: no depth, whatever depth_format says).
 * dvo_frames_upload_cameras(...) is this call with (DVO_CAM_BGR8, DVO_DEPTH_F32).  Frames in HBM (DVO_UPLOAD_DEVICE) are read in place
 * when every image is 4-byte aligned and every depth image 8-byte (U16) or 16-byte (F32) aligned; others take one landing copy.
 * Refused with DVO_ERR_INVALID, nothing changed: an unknown format, and everything dvo_frames_upload_cameras refuses. */
enum { DVO_CAM_BGR8 = 0, DVO_CAM_RGB8 = 1, DVO_CAM_MONO8 = 2 };
enum { DVO_DEPTH_F32 = 0, DVO_DEPTH_U16 = 1 };
int  dvo_frames_upload_cameras_fmt(dvo_ctx *ctx, int first_slot, int count, const void *const *image, int image_format,
                                   const void *const *depth, int depth_format, int rows, int cols, int n_levels, int first_shift,
                                   int now_first_pair, int flags);
/* ---- ignore masks: pixels that are not the world (the robot's own arm or bumper, a bonnet, an overlay, vignetted corners) -----
 * A mask is rows x cols bytes, row-major like a bgr8 image, NON-ZERO = "ignore this pixel", in the geometry of the frames as they are
 * stored (with an undistortion map: the undistorted image).  Per pyramid level l (s = first_shift + l, rows_l x cols_l as the uploads
 * size it) it becomes a KEEP PLANE:
 *   footprint   level pixel (y, x) stands for the camera pixels Y in [y 2^s, (y+1) 2^s), X in [x 2^s, (x+1) 2^s), clipped to the image
 *               (the block whose first pixel the INTER_NEAREST pyramid samples); where a rounded-up level size leaves nothing after the
 *               clipping, for the clamped pixel rows - 1 / cols - 1.  Camera pixels at or beyond rows_l 2^s / cols_l 2^s belong to none.
 *   drop0       some mask byte of the footprint is non-zero
 *   drop        some drop0 within `margin` LEVEL pixels in both directions (a square window, clipped to the level)
 *   keep        drop ? 0 : 255, column-major (y + x * rows_l) like every plane of the frame store
 * The margin is in level pixels because Canny's support is: a pixel's edge decision reads grey values within radius 2 (3 x 3 Sobel plus
 * the non-maximum comparison of the neighbours), so margin 2 keeps every edge that the masked pixels influenced out; 2 is the
 * recommendation, 0 is allowed, DVO_MASK_MAX_MARGIN the maximum.
 * EFFECT: after Canny, edge_l &= keep_l in the frame store, for every level of every frame that is uploaded as the now frame of a pair
 * with a mask (now_first_pair >= 0 in dvo_frames_upload_cameras / _fmt / _pyramids -- the rule the per-pair undistortion maps follow).
 * Everything that reads the stored edge map sees the masked edges: the now level's distance transform, the reference lists
 * (dvo_frames_as_ref), dvo_frame_get_level and its n_edges, the tracker's archive and views.  NOTHING ELSE changes: grey and depth
 * planes, place descriptors, the depth dvo_tracker_verify reads and the photometric engine (dvo_photo_* reads grey) are untouched, and so
 * are frames already in the store and reference lists already extracted.  Zeroing the depth instead only removes reference points: the
 * region's edges would still attract reprojected points in the now frame's distance transform. */
#define DVO_MASK_MAX_MARGIN 8
#define DVO_FRAMES_MASK_LAUNCHES 1  /* launches a chunk of an upload adds when at least one of its pairs has a mask (all levels, all images);
                                       an upload in which no listed pair has a mask issues exactly the launches, copies and synchronisations
                                       of a context that never had one.  No upload ever uploads a mask or a table */
/* The keep planes on the host, no device and no context needed (the definition; the device planes are byte-equal).  keep_out[l]:
 * level_rows[l] * level_cols[l] bytes; level_rows / level_cols (may be NULL) receive the level sizes.  DVO_ERR_INVALID, nothing written:
 * rows or cols < 1, mask, keep_out or a keep_out[l] NULL, n_levels outside [1, DVO_MAX_LEVELS], first_shift < 0, an empty level, margin
 * outside [0, DVO_MASK_MAX_MARGIN]. */
int  dvo_mask_levels_host(int rows, int cols, const unsigned char *mask, int n_levels, int first_shift, int margin,
                          unsigned char *const *keep_out, int *level_rows, int *level_cols);
/* Give pair `pair` (-1: every pair, all sharing ONE device copy of the planes) the mask; mask = NULL removes it (the other arguments
 * are then not looked at).  Takes effect with the next upload that lists the pair.  The call waits for the context stream, uploads the
 * camera-resolution mask, builds the level planes on the device (ONE launch) and uploads the per-pair table: two synchronisations.
 * Refused with DVO_ERR_INVALID, every mask in force unchanged: pair outside [-1, n_pairs), and with a mask what dvo_mask_levels_host
 * refuses.  An upload that lists a pair whose mask was built for another level geometry (n_levels or a level's size) is refused with
 * DVO_ERR_INVALID before anything is changed: the store keeps its frames. */
int  dvo_frames_set_pair_mask(dvo_ctx *ctx, int pair, int rows, int cols, const unsigned char *mask, int n_levels, int first_shift,
                              int margin);
/* inspection: the resident keep plane of one level (one copy, one synchronisation); keep_out may be NULL (sizes only), else capacity >=
 * rows * cols bytes.  DVO_ERR_STATE if the pair has no mask, DVO_ERR_INVALID for a pair or level out of range or a short buffer. */
int  dvo_frames_get_pair_mask_level(dvo_ctx *ctx, int pair, int level, unsigned char *keep_out, int capacity, int *rows, int *cols);
/* ---- depth registration: a raw depth image in the DEPTH camera's frame -> depth in the colour camera's pixel grid ----------------
 * RealSense, Azure Kinect and Orbbec class sensors deliver depth in the IR camera's frame: another resolution, an optical centre
 * 15-75 mm beside the colour camera's.  A RIG says how the two cameras sit; a registration turns raw depth images into what a driver
 * with hardware registration would publish as mono16: rows x cols 16-bit millimetres in the colour image's pixel grid, 0 = hole,
 * consumed as DVO_DEPTH_U16 without DVO_UPLOAD_DEPTH_RAW.  The target is the colour image AS IT IS UPLOADED, before the pair's
 * cv::undistort (the upload remaps both images afterwards): hence Dc5 is applied FORWARD, in closed form, no iteration.
 * Per depth pixel (v, u) with raw value r, all in IEEE double, in this order, nothing fused:
 *   1. Z: DVO_DEPTH_U16: r == 0 is no measurement, else Z = r / 1000.0; DVO_DEPTH_F32 (metres): r finite and > 0, Z = r.
 *   2. project(a, b): X = ((a - cxd) Z) / fxd, Y = ((b - cyd) Z) / fyd; Xc = R00 X + R01 Y + R02 Z + tx (left to right; Yc, Zc likewise);
 *      invalid unless Zc > 0; x = Xc / Zc, y = Yc / Zc; with has_Dc5: r2 = x x + y y, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *      xd = x rad + (2 p1 x y + p2 (r2 + 2 x x)), yd = y rad + (p1 (r2 + 2 y y) + 2 p2 x y); uc = fxc x + cxc, vc = fyc y + cyc.
 *   3. the centre (u, v) and the corners (u - 0.5, v - 0.5), (u + 0.5, v + 0.5) are projected at the pixel's own Z; the pixel is
 *      dropped if one of them is invalid or a corner coordinate is not finite or at or beyond 2^30 in magnitude.
 *   4. q = rint(Zc_centre 1000.0), half to even; dropped unless 1 <= q <= 65535.
 *   5. footprint: x0 = ceil(min of the corners' uc), x1 = min(ceil(max of them), x0 + DVO_DEPTH_SPLAT_MAX), rows likewise, clipped to
 *      the image; half-open: colour pixel x is covered iff x0 <= x < x1.
 *   6. out = min(out, q) over the footprint; a pixel nothing covered is 0.
 * Properties: an identity rig with equal intrinsics returns its input; a fronto-parallel plane is registered without holes, up- or
 * down-scaled; with a baseline the foreground wins and leaves an occlusion shadow of holes; slanted surfaces under rotation leave
 * isolated one-pixel cracks.  The registered depth is worst at depth discontinuities -- where the edges are: the foreground is dilated
 * by up to one pixel.  Holes are harmless downstream (0 -> 1 mm at the upload, selectedPts drops depths <= 100 mm).
 * Kc4 / Dc5 are the caller's to keep consistent with the undistortion of the pair (dvo_frames_set_undistort and the per-stream form).
 * OUT OF SCOPE: a distorted depth camera; hole filling or inpainting; colour-to-depth alignment; depth scales other than millimetres
 * and metres; overlap of the staging copies with preprocessing; DVO_UPLOAD_MAPPED and DVO_UPLOAD_DIRECT sources; the photometric
 * streams engine (dvo_photo_streams_*). */
#ifndef DVO_DEPTH_RIG_DEFINED_
#define DVO_DEPTH_RIG_DEFINED_
#define DVO_DEPTH_SPLAT_MAX 8
typedef struct dvo_depth_rig {
    int    depth_rows, depth_cols;   /* geometry of the raw depth image */
    double Kd4[4];                   /* depth camera fx, fy, cx, cy: pinhole, taken as undistorted */
    double R[9];                     /* column-major like every R of this header */
    double t[3];                     /* metres: X_colour = R X_depth + t */
    double Kc4[4];                   /* colour camera fx, fy, cx, cy of the colour image AS IT IS UPLOADED */
    int    has_Dc5;                  /* 1: Dc5 = k1, k2, p1, p2, k3 of the colour camera, applied FORWARD */
    double Dc5[5];
} dvo_depth_rig;
#endif
#define DVO_DEPTH_REGISTER_LAUNCHES 2   /* per dvo_frames_register_depth, whatever count is; a constant of the build */
/* The definition on the host, no device and no context needed (the device result is byte-equal).  depth: depth_rows x depth_cols of the
 * rig, row-major, in depth_format (DVO_DEPTH_*); out: rows * cols, row-major.  DVO_ERR_INVALID, nothing written: a NULL argument; rows,
 * cols, depth_rows or depth_cols < 1; an unknown depth format; a focal length of Kd4 or Kc4 that is not positive; any number of the rig
 * (Dc5 included, whatever has_Dc5 says) that is not finite; has_Dc5 other than 0 or 1.  R is taken as given: it is not checked for
 * orthogonality. */
int  dvo_depth_register_host(const dvo_depth_rig *rig, const void *depth, int depth_format, int rows, int cols, unsigned short *out);
/* Give pair `pair` (-1: every pair) the rig, for colour images of rows x cols; rig = NULL removes it (rows and cols are then not looked
 * at).  The call waits for the context stream and uploads the rig table: a registration never uploads it.  Refused with
 * DVO_ERR_INVALID, every rig in force unchanged: pair outside [-1, n_pairs), and with a rig what dvo_depth_register_host refuses. */
int  dvo_frames_set_pair_depth_rig(dvo_ctx *ctx, int pair, const dvo_depth_rig *rig, int rows, int cols);
/* Register `count` raw depth images: depth[i] (depth_format, the geometry of its rig) under the rig of pair first_pair + i.  The
 * results go into a pool of 16-bit images the context owns in HBM, each on a 16-byte boundary, so that dvo_frames_upload_cameras_fmt(
 * ..., DVO_UPLOAD_DEVICE) with DVO_DEPTH_U16 reads them in place; d_out[i] (d_out may be NULL) receives their device addresses.  They
 * stay valid until the next registration on the context.
 * flags: 0 -- the depth pointers are host memory, copied through a pinned mirror of the context: the caller's buffers are free on
 * return; DVO_UPLOAD_DEVICE -- the raw images are read where they are and stay borrowed until the context stream has passed this call
 * (dvo_synchronize); DVO_UPLOAD_ASYNC may be combined with either (the call never waits for its own work).
 * Asynchronous on the context stream: DVO_DEPTH_REGISTER_LAUNCHES launches (a scatter with one thread per raw depth pixel that takes
 * atomic minima in a 32-bit z-buffer, a resolve that narrows it to 16 bits and arms it again), one small copy of the address table,
 * and with host sources one copy of the images.  No host synchronisation except where the pools have to grow (first call, a larger
 * count or geometry): the pinned staging has two slots used in turn, so a call refills the slot whose copies were queued two calls
 * earlier, and waits for them only if the host has run that far ahead of the device.  An upload of the registered images on this
 * context that cannot read them in place (a colour image that is not 4-byte aligned) is ordered behind the registration by the
 * library; a caller that reads them on a stream of its own orders that stream behind the context stream itself.
 * Refused, nothing changed and the previous registered images still readable: DVO_ERR_STATE a listed pair without a rig;
 * DVO_ERR_INVALID a pair range outside the context, a NULL image, an unknown depth format, flags other than the above, listed pairs
 * whose rigs were set for different colour geometries. */
int  dvo_frames_register_depth(dvo_ctx *ctx, int first_pair, int count, const void *const *depth, int depth_format, int flags,
                               const unsigned short **d_out);
/* inspection: the registered image of `pair` from the last registration (one copy, one synchronisation); out may be NULL (sizes only),
 * else capacity >= rows * cols pixels.  DVO_ERR_STATE if the pair has no registered image, DVO_ERR_INVALID for a pair out of range or
 * a short buffer. */
int  dvo_frames_get_registered_depth(dvo_ctx *ctx, int pair, unsigned short *out, int capacity, int *rows, int *cols);
/* computeDistTransfrmOfNow (SolveDVO.cpp:1740-1799): slot first_slot+i becomes the now frame of pair first_pair+i.
 * Asynchronous on the context stream. */
int  dvo_frames_as_now(dvo_ctx *ctx, int first_slot, int first_pair, int count);
/* computeDistTransfrmOfRef's edge map + preProcessRefFrame (:269-303): slot first_slot+i becomes the reference
 * frame of pair first_pair+i.  N_out[i*n_levels + l] (may be NULL) receives the point counts.  Needs intrinsics
 * and depth.  One host synchronisation (the point counts size the slabs). */
int  dvo_frames_as_ref(dvo_ctx *ctx, int first_slot, int first_pair, int count, int *N_out);
/* inspection: geometry and resident images of one stored level (host outputs, column-major, any may be NULL) */
int  dvo_frame_get_level(dvo_ctx *ctx, int slot, int level, int *rows, int *cols, unsigned char *grey,
                         float *depth_mm, unsigned char *edge, int *n_edges);
int  dvo_frames_num_levels(const dvo_ctx *ctx);

/* ---- many camera streams: the tracker of SolveDVO::loop for K streams at once -----------------------------------------
 * A tracker owns K independent streams (a multi-camera rig, a fleet, the replay of many sequences).  Each has its own reference
 * frame, previous frame, warm-start pose, frame counter and lastRefFrame, and follows the loop of SolveDVO::loop with
 * __NEW__REF_UPDATE (SolveDVO.cpp:1970-2241) exactly as dvo_amd::SolveDVO::processFirstFrame / processFrame do for one camera:
 * the same poses, key-frame events and reasons, bit for bit.  One dvo_tracker_step advances any subset of the streams by one frame.
 *
 * Layout: one context of K pairs (stream s = pair s) and a frame store of 2K slots: stream s keeps its frames in slot bank*K + s,
 * the bank alternating from frame to frame so that the previous frame stays resident for a key-frame switch.  The reference extraction
 * and the alignment take any set of streams in one call (index-list forms of their kernels: the set need not be consecutive).  The
 * frame stage (upload + pyramid + Canny + now level) is one batched call per RUN of listed streams that are consecutive and write the
 * same bank: a step that lists every stream of a rig is one run, whatever K is; a stream that skipped an odd number of ticks writes
 * the other bank than its neighbours and splits the run (dvo_tracker_get_stats counts the runs).  With dvo_params.engine_variant = 1 or
 * interpolate_dt (the one-point-per-lane kernel, which has no index-list form) the alignment, too, is one launch per run.
 *
 * A step, in order: upload of the listed frames (each installed as its stream's now frame); the reference extraction of the streams
 * on their first frame (event 1, pose = identity: processFirstFrame); one alignment per run of the other streams from their last
 * estimate; ONE launch of the signals kernel that evaluates the key-frame rule on the device (dvo_tracker.hip) and gathers the
 * poses; one read of {pose, event, signals} per listed stream -- the only host synchronisation of an ordinary step.  Streams that
 * switch key frame then get their previous frame as reference (dvo_frames_as_ref: one more synchronisation for the point counts),
 * the identity pose and ONE re-run alignment launch for all of them, and their poses are read once more.
 * Bit-identity of the poses with a one-pair context needs the same launch shape on both sides (dvo_params.block_threads and
 * team_size fixed, e.g. 512 and 1): the pose update takes double sums whose order follows the workgroup and team size, which the
 * engine otherwise picks from the batch size.  Every float32 per-point quantity and every energy is identical under any shape; the
 * poses then agree to the rounding of those double sums. */
typedef struct dvo_tracker dvo_tracker;
typedef struct dvo_tracker_params {
    int   iters[DVO_MAX_LEVELS];  /* iterationsConfig (SolveDVO.cpp:30-33): iterations per level, level 0 finest; default 50 each */
    int   key_frame_every;        /* (nFrame - lastRefFrame) == 5 forces a key frame (:2155-2160) */
    int   adaptive;               /* 0 (default): the live rule only; 1: also the three exits the reference has commented out
                                     (:2129-2152), evaluated like dvo_amd::SolveDVO::adaptiveKeyFrames */
    float laplacian_b_thresh;     /* laplacianThreshExitCond = 3.0    (:22-23): b_cap above it -> reason 2 */
    float visible_ratio_thresh;   /* ratio_of_visible_pts_thresh = 0.8: visible ratio below it -> reason 3 */
    int   min_points;             /* 50: fewer points in the finest level that ran -> reason 4 */
    int   rows, cols;             /* camera frame (level -1 of the pyramid: dvo_frames_upload_cameras); default 480 x 640 */
    int   n_levels, first_shift;  /* level l is the camera frame decimated by 2^(first_shift + l); default 4, 1 (320x240 .. 40x30) */
    int   points_capacity[DVO_MAX_LEVELS];  /* reference points per stream and level to reserve at creation (0 = grow on demand): a
                                     reference list longer than the slab makes the engine reallocate and copy the slabs of ALL K
                                     streams in the middle of a step (counted in dvo_tracker_get_stats) */
} dvo_tracker_params;
int  dvo_tracker_params_default(dvo_tracker_params *tp);
/* p: engine parameters (NULL = defaults); tp NULL = defaults.  Fails with DVO_ERR_NO_DEVICE without a HIP device (no CPU fallback). */
int  dvo_tracker_create(const dvo_params *p, int max_streams, const dvo_tracker_params *tp, dvo_tracker **out);
int  dvo_tracker_destroy(dvo_tracker *tr);
const char *dvo_tracker_last_error(const dvo_tracker *tr);       /* tr may be NULL: last creation error */
/* the handle-wide camera model: required before the first step; it is the default of every stream without one of its own.  The
 * handle-wide undistortion is dvo_frames_set_undistort(dvo_tracker_context(tr), rows, cols, K4, D5) */
int  dvo_tracker_set_intrinsics(dvo_tracker *tr, float fx, float fy, float cx, float cy);
/* Per-stream calibration: a rig whose cameras have different calibrations runs in ONE handle (one launch sequence and one host
 * synchronisation per tick, as for a uniform rig).  A stream's own setting wins over the handle-wide one; a stream without one follows
 * the handle-wide setters, whenever they are called.
 *   set_stream_intrinsics: fx, fy, cx, cy of the camera frame (as dvo_tracker_set_intrinsics).
 *   set_stream_undistort:  cv::undistort of the stream's frames with K4 = {fx, fy, cx, cy}, D5 = {k1, k2, p1, p2, k3} (as
 *                          dvo_frames_set_undistort), the map built for the tracker's rows x cols; both NULL: this stream's frames
 *                          are taken as already undistorted.  Streams with the same (K4, D5) share one device map, freed when its
 *                          last stream changes or the handle is destroyed.  Frames of dvo_tracker_step only (step_pyramids takes
 *                          its frames as they are).
 *   clear_stream_camera:   back to the handle-wide intrinsics and undistortion.
 * When: only while the stream is at its start -- never stepped since creation or since dvo_tracker_reset_stream.  Otherwise
 * DVO_ERR_STATE and nothing changes (the stream's reference points were enlisted under its current camera model).
 * Refused with DVO_ERR_INVALID, nothing changed: a stream outside [0, max_streams), fx or fy not positive, only one of K4 and D5,
 * a NaN or an infinity in K4 or D5.
 * The calls wait for the handle's stream and upload the stream tables once; a step never uploads them. */
int  dvo_tracker_set_stream_intrinsics(dvo_tracker *tr, int stream, float fx, float fy, float cx, float cy);
int  dvo_tracker_set_stream_undistort(dvo_tracker *tr, int stream, const double *K4, const double *D5);
int  dvo_tracker_clear_stream_camera(dvo_tracker *tr, int stream);
/* Per-stream ignore mask ("ignore masks" above: dvo_frames_set_pair_mask for pair = stream with the tracker's rows, cols, n_levels and
 * first_shift): rows x cols bytes, non-zero = ignore; NULL removes it; stream = -1: every stream (one device copy).  Allowed at any time:
 * it takes effect with the stream's next frame; frames already in the store and the current reference list keep what they have.  A step
 * in which a listed stream has a mask costs DVO_FRAMES_MASK_LAUNCHES more launches per run and no more synchronisations; a step in which
 * none has costs what it costs without the feature.  Refused with DVO_ERR_INVALID, nothing changed: a stream outside [-1, max_streams),
 * margin outside [0, DVO_MASK_MAX_MARGIN].  The call itself waits for the handle's stream (two synchronisations, one launch). */
int  dvo_tracker_set_stream_mask(dvo_tracker *tr, int stream, const unsigned char *mask, int margin);
/* the stream starts over: its next frame is a first frame (event 1); its calibration and its mask stay, the calibration may now be changed */
int  dvo_tracker_reset_stream(dvo_tracker *tr, int stream);
/* Advance streams[0..count) by one frame each.  Frames as dvo_frames_upload_cameras takes them: bgr8[i] (rows x cols x 3, row-major)
 * and depth_m[i] (F32 metres, row-major) of stream streams[i]; flags: DVO_UPLOAD_DEVICE / DVO_UPLOAD_MAPPED / DVO_UPLOAD_DIRECT /
 * DVO_UPLOAD_DEPTH_RAW with the meaning they have there (buffers are borrowed until the call returns).  Outputs per listed stream i:
 * R_rel[9i..] (column-major, like cR_64) and t_rel[3i..] = the key-frame relative pose, event[i] = 0 ordinary, 1 first frame of the
 * stream (it becomes reference and key frame, pose = identity), 2..5 the reasonForChange of a key-frame switch (the most recent
 * frame became the key frame, the pose is the re-run's).  Refused with DVO_ERR_INVALID, state unchanged: a stream outside
 * [0, max_streams), a stream listed twice, count outside [1, max_streams], rows / cols other than the tracker's. */
int  dvo_tracker_step(dvo_tracker *tr, int count, const int *streams, const unsigned char *const *bgr8, const float *const *depth_m,
                      int rows, int cols, int flags, double *R_rel, double *t_rel, int *event);
/* dvo_tracker_step with the frames in sensor formats (dvo_frames_upload_cameras_fmt: image[i] in image_format, depth[i] in
 * depth_format; DVO_DEPTH_U16 without DVO_UPLOAD_DEPTH_RAW is what the pyramid publisher makes of a mono16 depth topic).  Poses, events,
 * signals and the step's launch and synchronisation counts equal those of dvo_tracker_step on the input the formats stand for;
 * dvo_tracker_step is this call with (DVO_CAM_BGR8, DVO_DEPTH_F32).  Also refused with DVO_ERR_INVALID: an unknown format. */
int  dvo_tracker_step_fmt(dvo_tracker *tr, int count, const int *streams, const void *const *image, int image_format,
                          const void *const *depth, int depth_format, int rows, int cols, int flags, double *R_rel, double *t_rel, int *event);
/* Per-stream depth rig ("depth registration" above: dvo_frames_set_pair_depth_rig for pair = stream, the colour geometry being the
 * tracker's rows x cols); NULL removes it.  Kc4 and Dc5 are the caller's to keep consistent with dvo_tracker_set_stream_undistort: the
 * registration targets the colour image as it is uploaded, the stream's undistortion then remaps both images.  When: only while the
 * stream is at its start, like its calibration (DVO_ERR_STATE otherwise, nothing changed).  Refused with DVO_ERR_INVALID, nothing
 * changed: a stream outside [0, max_streams), and what dvo_depth_register_host refuses in a rig.  The call waits for the handle's
 * stream and uploads the rig table once; a step never uploads it.
 * Out of scope: a distorted depth camera, hole filling, colour-to-depth alignment, depth scales other than millimetres and metres,
 * overlap of the staging copies with preprocessing, DVO_UPLOAD_MAPPED / DVO_UPLOAD_DIRECT sources, the photometric streams engine. */
int  dvo_tracker_set_stream_depth_rig(dvo_tracker *tr, int stream, const dvo_depth_rig *rig);
/* dvo_tracker_step_fmt for UNREGISTERED depth: image[i] is the colour image (rows x cols, the tracker's), depth[i] the raw depth image
 * of stream streams[i] in the geometry of the stream's rig (depth_format: DVO_DEPTH_U16 millimetres or DVO_DEPTH_F32 metres).  Per run
 * of the step the depth images are registered on the device (one dvo_frames_register_depth: DVO_DEPTH_REGISTER_LAUNCHES launches) and
 * uploaded from there as DVO_DEPTH_U16 device sources; host colour images are staged into a pool of the handle by the pinned-mirror
 * copy the upload would have made, so that both sources are read in place.  flags: 0 (host memory) or DVO_UPLOAD_DEVICE; everything
 * else is refused with DVO_ERR_INVALID, DVO_UPLOAD_DEPTH_RAW included.
 * CONTRACT: poses, events and signals are those of dvo_tracker_step_fmt fed dvo_depth_register_host's output as DVO_DEPTH_U16, bit
 * for bit.  With DVO_UPLOAD_DEVICE a step costs that step's launches plus DVO_DEPTH_REGISTER_LAUNCHES per run, and no more host
 * synchronisations.  Also refused: what dvo_tracker_step_fmt refuses; with DVO_ERR_STATE, state unchanged, a listed stream without
 * a rig. */
int  dvo_tracker_step_raw_depth(dvo_tracker *tr, int count, const int *streams, const void *const *image, int image_format,
                                const void *const *depth, int depth_format, int rows, int cols, int flags,
                                double *R_rel, double *t_rel, int *event);
/* The same with the frames as pyramids (dvo_frames_upload_pyramids: grey[i*n_levels + l], depth[i*n_levels + l]), e.g. the
 * OpenCV-XML frames of the reference's publisher; level l must have the tracker's level-l geometry. */
int  dvo_tracker_step_pyramids(dvo_tracker *tr, int count, const int *streams, const dvo_image *grey, const dvo_image *depth,
                               int flags, double *R_rel, double *t_rel, int *event);
/* What the last step's first alignment of `stream` produced on the finest level that ran: lastLaplacianB (b_cap; 0 unless
 * tp.adaptive, which is when finalEpsilons are produced), lastVisibleRatio, lastNumPoints of dvo_amd::SolveDVO.  Host memory, no
 * device access.  DVO_ERR_STATE if the stream has not been aligned yet. */
int  dvo_tracker_get_signals(dvo_tracker *tr, int stream, float *b_cap, float *visible_ratio, int *n_points);
/* The 6x6 information matrix of every pose the tracker returns: what a pose-graph back end, a filter or a PoseWithCovariance needs
 * beside the pose.  Off by default; while it is off a step issues exactly the launches, copies and synchronisations it issues without
 * this feature.  dvo_tracker_set_information(tr, 1) switches it on for the steps that follow: each step then adds ONE launch of a
 * kernel of its own (dvo_tracker_info.hip, one workgroup per aligned stream) after the alignment, one more after the re-run alignment
 * on a step in which streams switched key frame (for those streams: at the re-run's pose, against their new reference), and one
 * asynchronous copy of the records in front of each synchronisation the step makes anyway -- no host synchronisation is added, the
 * alignment launches are the same launches.  The kernel reads the stream's reference points and now level in the forms the context
 * keeps resident (compact list, compact now form), with the stream's own camera model: mixed rigs included -- the case
 * DVO_FLAG_NORMAL_MATRIX refuses.  Refused with DVO_ERR_INVALID, nothing changed: on = 1 on a tracker created with
 * dvo_params.interpolate_dt or engine_variant = 1 (those contexts keep other resident forms), or with debug_alias_mod.
 *
 * dvo_tracker_get_information: the record of `stream` for the pose its last step returned, on the finest level that ran
 * (`level`): H36 = H = sum_i w_i J_i J_i^T, the symmetric 6x6 matrix (row-major = column-major), g6 = J^T W eps, sum_eps2 = the
 * correctly rounded exact sum of eps_i^2 and n_visible = the number of visible points -- the quantities dvo_accumulate gives for that
 * pair, level and pose (double sums; only their order of addition differs, sum_eps2 and n_visible are equal).  The six components
 * are in the order of J in dvo_eval_points and of psi: [translation x, y, z, rotation x, y, z].  A stream on its first frame (event 1:
 * no alignment happened) has the all-zero record with n_visible = 0 and level = -1.  Any output pointer may be NULL.  Host memory, no
 * device access.  DVO_ERR_STATE: information is off, or the stream has not been stepped since it was switched on or since
 * dvo_tracker_reset_stream; DVO_ERR_INVALID: a stream outside [0, max_streams).
 * Covariance: dvo_amd::poseCovariance (include/dvo_amd.hpp) / DvoTracker.covariance. */
int  dvo_tracker_set_information(dvo_tracker *tr, int on);
int  dvo_tracker_get_information(dvo_tracker *tr, int stream, double *H36, double *g6, double *sum_eps2, int *n_visible, int *level);
/* The views SolveDVO::loop shows after every frame, rendered in HBM for every listed stream: where the reference edge points landed in
 * the now frame, over the distance transform (sOverlay, SolveDVO.cpp:1186-1226, :2294); the same points coloured by their residual,
 * over the now grey image (visualizeDistanceResidueHeatMap, :1528-1583); and the residue histogram (processResidueHistogram,
 * :1398-1410).  Off by default; while they are off a step issues exactly the launches, copies and synchronisations it issues without
 * this feature.  dvo_tracker_set_views(tr, 1) switches them on for the steps that follow: each step then adds one RENDERING =
 * DVO_TRACKER_VIEW_LAUNCHES launches of kernels of their own (dvo_tracker_views.hip: pixel tiles x listed streams for the backgrounds,
 * point chunks x listed streams for the marks and the histogram) where the information kernel runs, a second rendering after the
 * re-run alignment on a step in which streams switched key frame (for those streams), and one asynchronous copy of the histogram
 * records in front of each synchronisation the step makes anyway -- no host synchronisation is added, and images are never copied by
 * a step: they stay resident (2 x max_streams x rows x cols x 3 bytes) and are fetched on request.  Refused with DVO_ERR_INVALID,
 * nothing changed: on = 1 on a tracker created with dvo_params.interpolate_dt, engine_variant = 1 or debug_alias_mod (the rule of
 * dvo_tracker_set_information; views and information are independent and may both be on).
 *
 * Everything is evaluated at the pose and level of dvo_tracker_get_information: the pose the step returned for the stream (the re-run's
 * for a stream that switched key frame), against the reference it now has, on the finest level that ran (dvo_tracker_view_size).  A
 * reference point i is projected with the engine's per-point code, the stream's own intrinsics and the engine's half-open visibility
 * rule; for a visible point (px, py) = ((int)u, (int)v) and d_i = DT(py, px), the float the alignment looks up.
 *   histogram: hist260[(int)eps_i + 1]++ for every point of the list, eps_i = d_i for a visible point and 0 for an invisible one
 *       (getReprojectedEpsilons): the counts sum to n_points, bin 0 is empty; they stay integers (the reference's division by N is the
 *       caller's).
 *   DVO_VIEW_REPROJ_ON_DT: BGR8, row-major rows x cols x 3; every pixel (g, g, g), g = DT(y, x) rounded half to even and saturated
 *       (convertTo(CV_8UC1)); every pixel hit by a visible point (0, 255, 0).
 *   DVO_VIEW_RESIDUE_HEAT: every pixel (g, g, g), g = the grey level of the frame the step was given, at that level; every pixel hit by
 *       a visible point jet[d > 60 ? 63 : (int)d], d = DT at that pixel, jet = the 64-entry jet map of FColorMap in B, G, R order
 *       (dvo_amd::jetColour in include/dvo_amd.hpp).
 * One deviation from the reference: its cordList_2_mask (:472) accepts u == cols and v == rows and then writes outside the mask; here
 * a point marks a pixel exactly when the engine counts it visible.  A stream on its first frame (event 1: no alignment happened) has
 * the all-zero histogram with n_points = 0 and level = -1, and both views are their plain backgrounds.
 *
 * dvo_tracker_get_residue_histogram: host memory, no device access; any output pointer may be NULL.  dvo_tracker_view_size: geometry
 * and level of the views (always available).  dvo_tracker_get_view: one copy of rows * cols * 3 bytes to host memory and one
 * synchronisation.  dvo_tracker_view_device: the resident image itself, valid until the stream's next step (ordered on the context's
 * stream).  DVO_ERR_STATE: views are off, or the stream has not been stepped since they were switched on or since
 * dvo_tracker_reset_stream; DVO_ERR_INVALID: a stream outside [0, max_streams) or an unknown view. */
#define DVO_VIEW_REPROJ_ON_DT 0
#define DVO_VIEW_RESIDUE_HEAT 1
#define DVO_TRACKER_VIEW_LAUNCHES 2
#define DVO_VIEW_HISTOGRAM_BINS 260
int  dvo_tracker_set_views(dvo_tracker *tr, int on);
int  dvo_tracker_get_residue_histogram(dvo_tracker *tr, int stream, unsigned *hist260, int *n_points, int *level);
int  dvo_tracker_view_size(dvo_tracker *tr, int *rows, int *cols, int *level);
int  dvo_tracker_get_view(dvo_tracker *tr, int stream, int view, unsigned char *bgr8);
int  dvo_tracker_view_device(dvo_tracker *tr, int stream, int view, const unsigned char **d_bgr8);
/* ---- key-frame archive and loop-closure alignment ------------------------------------------------------------------------------
 * A pose-graph back end needs, beside the poses and their information, edges between a frame and key frames OTHER than its stream's
 * current one: revisits, relocalisation after a reset, one camera of a fleet seeing what another saw.  The archive keeps the key
 * frames the tracker makes, in HBM, and two calls evaluate kept key frames against a stream's CURRENT now frame without an upload, a
 * frame stage or a second handle.  Off by default; while it is off a step issues exactly the launches, copies and synchronisations it
 * issues without this feature, and nothing below the archive's own calls ever touches the alignment kernels or the tracker's context.
 *
 * dvo_tracker_set_archive(tr, capacity, max_matches, points_capacity): a ring of `capacity` slots and a private match context of
 *   `max_matches` pairs.  points_capacity[l] (DVO_MAX_LEVELS entries, or NULL) = the longest list of level l a slot holds; 0 = rows_l *
 *   cols_l / 8 (edge images of 5-6 % edge pixels, the usual density, fill less than half of that).  capacity = 0 switches the archive
 *   off and frees it.  A second call re-configures: the ring starts empty, ids go on counting.  Refused with DVO_ERR_INVALID, nothing
 *   changed: a tracker created with dvo_params.interpolate_dt, engine_variant = 1 or debug_alias_mod (the rule of
 *   dvo_tracker_set_information), capacity < 0, max_matches < 1, a negative points_capacity.
 *   While it is on, every stream that gets a new key frame in a step (events 1 and 2..5) has it stored in the next slot: per level the
 *   reference list in the resident forms the index-list alignment reads (compact 8-byte points, their 4-byte twins) and its count, the
 *   stream's camera model (fx, fy, cx, cy), the stream and the frame number (0 for event 1, the previous frame's number for a switch).
 *   The store is a device-side copy on the context's stream (dvo_tracker_archive.hip): DVO_TRACKER_ARCHIVE_LAUNCHES launch for all the
 *   first frames of a step and one for all its key-frame switches, after the respective reference extraction -- one launch on an
 *   ordinary tick with new key frames, two on a tick that has both; no host synchronisation is added.
 *   Ids are 64-bit and increase by one per archived key frame: id n lives in slot n % capacity and is evicted by id n + capacity.
 *   (More new key frames in ONE step than the ring has slots: the earliest of them are evicted at once.)  A key frame with a list longer
 *   than points_capacity[l] at some level is not archived: its id is -1 and the `refused` counter goes up.
 * dvo_tracker_key_frame_id: id of the stream's current key frame; -1 = not archived (refused, evicted since, or made while the archive
 *   was off).  DVO_ERR_STATE: archive off, stream never stepped.
 * dvo_tracker_archive_info: stream, frame number and per-level point counts (tracker's n_levels entries) of an archived key frame; any
 *   output pointer may be NULL.  dvo_tracker_archive_get_points: the contract of dvo_get_ref_level -- the list of `level` as 3 x N floats
 *   decoded from the slot, bit-equal to what dvo_get_ref_level(dvo_tracker_context(tr), stream, level) gave right after the step that
 *   made the key frame (*N_out = N, min(N, capacity) points are copied; one launch, one copy, one synchronisation).  An id that was
 *   never given, was refused or has been evicted gives DVO_ERR_STATE in every call that takes one.
 * dvo_tracker_archive_stats: key frames archived, refused and evicted so far, and the kernel launches and host synchronisations of the
 *   last dvo_tracker_score / dvo_tracker_match / dvo_tracker_query_places / dvo_tracker_place_shifts / dvo_tracker_verify /
 *   dvo_tracker_archive_export / dvo_tracker_archive_import (counted as for dvo_tracker_get_stats).  Any pointer may be NULL.
 *
 * dvo_tracker_score(tr, n, stream, key_id, level, R, t, records): for candidate i the archived key frame key_id[i] against the current
 *   now frame of stream[i], on the points of `level`, at the pose (R + 9 i, t + 3 i) in the convention of dvo_tracker_step's outputs.
 *   records[i]: n_points = the list's length, and H36, g6, sum_eps2, n_visible with the meanings of dvo_tracker_get_information.  ONE
 *   launch for all candidates (one workgroup per candidate, the information kernel's walk: a record depends on its own candidate alone,
 *   not on n nor on the candidates' order), the candidates' upload, one copy of the records and ONE synchronisation.
 * dvo_tracker_match(tr, n, stream, key_id, R0, t0, R, t, records): the tracker's whole level schedule (dvo_tracker_params.iters) for
 *   every candidate from the guess (R0 + 9 i, t0 + 3 i), then the records at the resulting poses on the finest level that ran.
 *   DVO_TRACKER_MATCH_LAUNCHES launches -- one device-to-device load of the slots' lists and the streams' resident now levels into the
 *   match context, ONE alignment launch through an index list, one scoring launch -- and ONE synchronisation.  (Once, at the first
 *   match after a stream got intrinsics of its own, one more synchronisation makes the match context's table.)  The tracker's context
 *   is only read: which texels travel with a now level is decided from the host state it already has and, where that is not known yet,
 *   on the device.  The pose of candidate i
 *   is what a tracker of its own, fed the key frame's image and then the now image, returns for its second step from that guess: the
 *   same kernel, the same launch shape, the same data.  It does not disturb tracking: poses, warm starts, references, signals,
 *   information records and views of every stream are what they were.
 *   Both calls are refused, nothing changed, with DVO_ERR_INVALID: n outside [1, max_matches], a stream outside [0, max_streams), a level
 *   outside the tracker's, a NULL argument, a key frame whose camera model (fx, fy, cx, cy) is not bit-equal to that of stream[i] (a
 *   pair is decoded and projected under one model; key frames of ANOTHER stream with the same model are welcome); with DVO_ERR_STATE:
 *   archive off, a stream that has never been stepped, an unknown or evicted id. */
#define DVO_TRACKER_ARCHIVE_LAUNCHES 1
#define DVO_TRACKER_MATCH_LAUNCHES 3
typedef struct dvo_tracker_score_record {
    double H36[36];           /* H = sum w J J^T, symmetric */
    double g6[6];             /* J^T W eps */
    double sum_eps2;          /* the correctly rounded exact sum */
    int n_points, n_visible;
} dvo_tracker_score_record;
int  dvo_tracker_set_archive(dvo_tracker *tr, int capacity, int max_matches, const int *points_capacity);
int  dvo_tracker_key_frame_id(dvo_tracker *tr, int stream, long long *id);
int  dvo_tracker_archive_info(dvo_tracker *tr, long long id, int *stream, long long *frame, int *n_points);
int  dvo_tracker_archive_get_points(dvo_tracker *tr, long long id, int level, float *xyz_out, int capacity, int *N_out);
int  dvo_tracker_archive_stats(dvo_tracker *tr, long long *archived, long long *refused, long long *evicted, int *last_launches,
                               int *last_syncs);
int  dvo_tracker_score(dvo_tracker *tr, int n, const int *stream, const long long *key_id, int level, const double *R, const double *t,
                       dvo_tracker_score_record *records);
int  dvo_tracker_match(dvo_tracker *tr, int n, const int *stream, const long long *key_id, const double *R0, const double *t0, double *R,
                       double *t, dvo_tracker_score_record *records);
/* ---- place descriptors and top-k key-frame retrieval ---------------------------------------------------------------------------
 * dvo_tracker_match takes (stream, key_id) pairs; this is what chooses them.  The tracker returns key-frame-relative poses only, so
 * pose proximity is not available inside the library -- and it is useless for relocalisation after a reset or for one camera of a
 * fleet seeing what another saw.  Retrieval is therefore by appearance: one small descriptor per archived key frame and one batched
 * query that returns, per listed stream, the k archived key frames whose descriptors are nearest to the stream's CURRENT frame.  Off
 * by default; while it is off every step, store, score and match issues exactly the launches, copies and synchronisations it issues
 * without this feature.
 *
 * The descriptor is the brightness-normalised tiny image (the classic SAD place descriptor), taken from the grey image of one pyramid
 * level that the frame store already holds in HBM (u8, column-major).  For level L: D = rows_L * cols_L, a_i the grey bytes in the
 * store's order, S = sum a_i;  m = (2 S + D) / (2 D) in integers (the mean, rounded half up);  b_i = clamp(a_i - m + 128, 0, 255).
 * distance(b, b') = sum |b_i - b'_i| as unsigned 32-bit.  Integer arithmetic throughout: a descriptor and a distance have one value.
 * (On the device a row is padded to a multiple of 16 bytes with 128, which adds 0 to every distance.)
 *
 * dvo_tracker_set_places(tr, level): level >= 0 switches descriptors on at that level of the tracker's pyramid (the coarsest,
 *   n_levels - 1, is the usual choice), -1 switches them off and frees them.  Needs the archive: DVO_ERR_STATE while it is off.
 *   DVO_ERR_INVALID, nothing changed: a level outside the tracker's, or one with D > 19 200 (120 x 160; it keeps a distance below 2^23
 *   and the query tile in LDS).  Allocates capacity x stride bytes beside the ring.  Every successful call starts without descriptors;
 *   re-configuring the archive (dvo_tracker_set_archive again) switches places off.
 *   While places are on, every key frame the archive stores also gets its descriptor, computed on the device from the frame-store slot
 *   that has just become the stream's reference (event 1: the slot of the frame just fed; events 2..5: the previous frame's slot in the
 *   other bank) and written beside the key frame's ring slot: DVO_TRACKER_PLACE_STORE_LAUNCHES more launch wherever the archive's store
 *   is launched (one for all first frames of a step, one for all its switches), ordered on the context's stream, no host
 *   synchronisation.  A key frame archived while places were off has no descriptor and is never returned; one the archive refuses
 *   gets none either.
 * dvo_tracker_archive_get_descriptor: the D unpadded bytes of an archived key frame's descriptor (*D_out = D, min(D, capacity) bytes are
 *   copied; one copy, one synchronisation).  DVO_ERR_STATE: places off, or an id that is unknown, evicted, refused or has no descriptor.
 * dvo_tracker_query_places(tr, n, streams, k, min_frame_gap, out, n_found): for each listed stream the descriptor of its current frame
 *   is computed from the frame store (no upload, no frame stage) and compared with every live slot that has a descriptor, EXCEPT
 *   (a) key frames whose camera model (fx, fy, cx, cy) is not bit-equal to the stream's (dvo_tracker_match would refuse them), (b) the
 *   stream's own current key frame (it is being tracked against already), (c) key frames made by the same stream with current frame
 *   number - key frame's frame number < min_frame_gap (the numbers of dvo_tracker_archive_info; 0 disables the rule).
 *   out[i * k .. i * k + n_found[i]) holds the nearest key frames ordered by (distance, key_id) ascending -- ties go to the smaller id,
 *   a total order, so the result is unique -- and the remaining entries of the row are {-1, -1, -1, 0xFFFFFFFF}.  A row depends on its
 *   own stream alone: not on n, not on the order of `streams`, and on k only as the k-prefix of the longer list.  n_found may be NULL.
 *   Cost: DVO_TRACKER_PLACE_QUERY_LAUNCHES launches (distances with the queries' descriptors made in LDS; selection), the upload of the
 *   query list, one copy of the result and ONE synchronisation, reported by dvo_tracker_archive_stats (last_launches, last_syncs) as
 *   for score and match.  The tracker's context and the archive are only read.
 *   DVO_ERR_INVALID, nothing changed: n outside [1, max_streams], k outside [1, DVO_TRACKER_PLACES_MAX_K], a stream outside range or
 *   listed twice, a negative min_frame_gap, NULL streams or out.  DVO_ERR_STATE: places off, a stream that has never been stepped. */
typedef struct dvo_tracker_place {
    long long key_id;         /* -1: no entry */
    long long frame;          /* the key frame's frame number (dvo_tracker_archive_info) */
    int stream;               /* the stream that made it */
    unsigned distance;        /* 0xFFFFFFFF: no entry */
} dvo_tracker_place;
#define DVO_TRACKER_PLACE_STORE_LAUNCHES 1
#define DVO_TRACKER_PLACE_QUERY_LAUNCHES 2
#define DVO_TRACKER_PLACES_MAX_K 32
int  dvo_tracker_set_places(dvo_tracker *tr, int level);
int  dvo_tracker_archive_get_descriptor(dvo_tracker *tr, long long id, unsigned char *out, int capacity, int *D_out);
int  dvo_tracker_query_places(dvo_tracker *tr, int n, const int *streams, int k, long long min_frame_gap, dvo_tracker_place *out,
                              int *n_found);
/* ---- shift search on place descriptors, and a pose guess from the shift ---------------------------------------------------------
 * The whole-descriptor SAD of dvo_tracker_query_places has no tolerance to image shift, and a revisit is never pixel-aligned: a frame
 * shifted by a few pixels of the descriptor level is as far from its key frame as a different scene is.  Between the query and
 * dvo_tracker_match stands therefore a registration of the two descriptors: for explicit (stream, key frame) candidates, the integer
 * shift that best lays the key frame's descriptor onto the stream's current frame, with the evidence to rank or reject on -- and, from
 * the shift, a rotation guess for dvo_tracker_match, whose callers otherwise pass the identity.
 *
 * Definition.  L = the places level, rows_L x cols_L its geometry, D = rows_L * cols_L.  b(y, x) = byte x * rows_L + y of an unpadded
 * descriptor (the store is column-major).  k = the stored descriptor of key_id[i]; q = the descriptor of the current frame of
 * stream[i], computed from the frame store exactly as dvo_tracker_query_places computes it (the mean over all D bytes; no upload, no
 * frame stage).  For radius r the window is W = { r <= y < rows_L - r, r <= x < cols_L - r }, area = (rows_L - 2 r)(cols_L - 2 r), and
 *   SAD(dy, dx) = sum over W of |k(y, x) - q(y + dy, x + dx)|   for |dy|, |dx| <= r, as unsigned 32-bit.
 * Sign convention: what the key frame shows at (y, x), the current frame shows at (y + dy, x + dx).  The best shift is the minimum under
 * the total order (SAD, |dy| + |dx|, dy, dx): the result is unique.  Integer arithmetic throughout: every field has one value.
 *
 * dvo_tracker_place_shifts(tr, n, stream, key_id, radius, records): records[i] for candidate (stream[i], key_id[i]): the best shift
 *   (dy, dx); sad = SAD there; sad_zero = SAD(0, 0) over the same window; sad_second = the smallest SAD among the shifts with
 *   max(|dy - dy*|, |dx - dx*|) >= 2 of the best (dy*, dx*) -- how far the minimum stands out of its surroundings -- or 0xFFFFFFFF where
 *   there is no such shift; area.  Radius 0 is allowed: then sad == sad_zero == the distance dvo_tracker_query_places reports for the
 *   pair, and sad_second is 0xFFFFFFFF.  A record depends on its own candidate alone: not on n, not on the order of the candidates, not
 *   on duplicates in the list; a stream may be listed with many key frames.
 *   Cost: the candidates' upload, DVO_TRACKER_PLACE_SHIFT_LAUNCHES launch (one workgroup per candidate: both descriptors and the table
 *   of the (2 r + 1)^2 SADs in LDS), one copy of the records and ONE synchronisation, reported by dvo_tracker_archive_stats
 *   (last_launches, last_syncs).  The tracker's context, the frame store, the archive and the descriptors are only read; the buffers
 *   of candidates and records are allocated by dvo_tracker_set_places, never in a step; while nobody calls it every step, store, score,
 *   match, query and verify issues exactly what it issues without this feature.
 *   DVO_ERR_INVALID, nothing changed: n outside [1, max_streams * DVO_TRACKER_PLACES_MAX_K], a NULL argument, a stream outside range,
 *   radius outside [0, DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS] or with rows_L - 2 r < 1 or cols_L - 2 r < 1, a key frame whose camera model
 *   is not bit-equal to the stream's (the rule of match and verify).  DVO_ERR_STATE: places off, a stream that has never been stepped,
 *   an id that is unknown, refused or evicted, or has no descriptor because it was archived while places were off.
 * dvo_tracker_place_guess(tr, stream, dy, dx, R0, t0): a shift as a guess for dvo_tracker_match.  Host memory only, no device access.
 *   fx_L = fx * 2^-(first_shift + L), fy_L likewise, in double from the stream's own float intrinsics;  a = (dx / fx_L, dy / fy_L, 1);
 *   d = a / |a|;  v = d x e3 = (d_y, -d_x, 0);  R0 = I + [v]x + [v]x^2 / (1 + d_z), the smallest rotation with R0 d = e3;  t0 = 0.
 *   In the convention of dvo_tracker_step's outputs the now-camera point is R^T (X - t), so the key frame's optical axis, R0^T e3 = d,
 *   is seen in the current camera at (cx_L + dx, cy_L + dy).  R0 is column-major like every R of this header.  This is a first-order,
 *   pure-rotation GUESS, not an estimate: a shift of the image is explained by rotation alone, translation and parallax are ignored.
 *   DVO_ERR_STATE: places off (or intrinsics never set).  DVO_ERR_INVALID: a stream outside range, a NULL pointer, |dy| or |dx| above
 *   DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS. */
#define DVO_TRACKER_PLACE_SHIFT_LAUNCHES 1
#define DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS 8
typedef struct dvo_tracker_place_shift {
    int dy, dx;               /* best shift, |dy|, |dx| <= radius */
    unsigned sad;             /* SAD at the best shift */
    unsigned sad_zero;        /* SAD at (0, 0) over the same window */
    unsigned sad_second;      /* smallest SAD among shifts with max(|dy-dy*|, |dx-dx*|) >= 2; 0xFFFFFFFF if there is none */
    int area;                 /* pixels in the window */
} dvo_tracker_place_shift;
int  dvo_tracker_place_shifts(dvo_tracker *tr, int n, const int *stream, const long long *key_id, int radius,
                              dvo_tracker_place_shift *records);
int  dvo_tracker_place_guess(dvo_tracker *tr, int stream, int dy, int dx, double *R0, double *t0);
/* ---- depth verification of loop-closure candidates -----------------------------------------------------------------------------
 * Everything dvo_tracker_score and dvo_tracker_match return is measured on the edge distance transform, the signal the alignment
 * minimised: a wrong candidate in an edge-rich scene still lands its points near SOME edge.  The independent evidence is the depth of
 * the stream's current frame, which the frame store holds in HBM (float millimetres, every level) and the alignment never reads.  A
 * key-frame point warped into the current camera has a predicted depth; the current frame has a measured one at the pixel the point
 * lands on.  Points that agree support the candidate, points far IN FRONT of the measured surface (free-space violations) count
 * against it, points BEHIND it (occlusions) are neutral.
 *
 * dvo_tracker_verify(tr, n, stream, key_id, level, R, t, vp, records): for candidate i the archived key frame key_id[i] against the
 *   depth plane of `level` of the current frame of stream[i], at the pose (R + 9 i, t + 3 i) in the convention of dvo_tracker_step's
 *   outputs.  vp = NULL: the defaults.  Per point of the slot's list of `level`, all in float32 and in this order: X, Y, Z from the
 *   compact point; vis, u, v by the engine's projection (half-open bounds, false for NaN); px = (int)u, py = (int)v; d = the depth at
 *   (py, px) in mm; has = vis && d > min_depth_mm && d <= max_depth_mm (false for NaN; the store writes 1.0 for "no measurement" and 0
 *   outside an undistortion map: the default min_depth_mm = 1 excludes both); z_mm = p2 * 1000 with p2 the third coordinate of
 *   R^T (X - t); r = z_mm - d; tol = tol_mm + tol_rel * d.  agree: has && |r| <= tol; front: has && r < -tol; behind: has && r > tol.
 *   records[i]: n_points = the list's length, n_visible, n_depth (`has`), n_agree, n_front, n_behind, and sum_abs_q4 = the sum over
 *   agreeing points of (unsigned)(min(|r|, 65535) * 16), i.e. |r| in 1/16 mm, truncated.  Integers only: every field has one value,
 *   whatever the order of the reduction; a record depends on its own candidate alone, not on n nor on the candidates' order.
 *   Cost: the candidates' upload, DVO_TRACKER_VERIFY_LAUNCHES launch (one workgroup per candidate, one 4-byte gather per point), one
 *   copy of the records and ONE synchronisation, reported by dvo_tracker_archive_stats (last_launches, last_syncs).  The tracker's
 *   context, the frame store and the archive are only read: tracking, records, views and places are undisturbed, and while nobody
 *   calls it every step, store, score, match and query issues exactly what it issues without this feature.
 *   DVO_ERR_INVALID, nothing changed: n outside [1, max_matches], a stream outside range, a level outside the tracker's, a NULL stream,
 *   key_id, R, t or records, a key frame whose camera model is not bit-equal to the stream's, tol_mm < 0, tol_rel < 0, min_depth_mm >=
 *   max_depth_mm or a NaN in vp.  DVO_ERR_STATE: archive off, a stream that has never been stepped, an unknown, refused or evicted id,
 *   a current frame that was stored without a depth plane.
 * dvo_tracker_verify_params_default: tol_mm = 25, tol_rel = 0.02, min_depth_mm = 1, max_depth_mm = 65535.  These are PARAMETERS sized
 *   for a structured-light sensor (whose depth noise grows with range), not measured values: set them from the sensor's data sheet. */
typedef struct dvo_tracker_verify_params {
    float tol_mm, tol_rel, min_depth_mm, max_depth_mm;
} dvo_tracker_verify_params;
typedef struct dvo_tracker_verify_record {
    int n_points, n_visible, n_depth, n_agree, n_front, n_behind;
    unsigned long long sum_abs_q4;
} dvo_tracker_verify_record;
#define DVO_TRACKER_VERIFY_LAUNCHES 1
int  dvo_tracker_verify_params_default(dvo_tracker_verify_params *vp);
int  dvo_tracker_verify(dvo_tracker *tr, int n, const int *stream, const long long *key_id, int level, const double *R, const double *t,
                        const dvo_tracker_verify_params *vp, dvo_tracker_verify_record *records);
/* ---- export and import of the key-frame archive ("save map / load map") ---------------------------------------------------------
 * The archive lives in one process's HBM: dvo_tracker_destroy or a restart loses every key frame.  These calls move key frames out of
 * a tracker and into another one -- another run, another process, another machine -- in the form score, match, verify, the query and
 * the shift search read: the slots as they are.  A slot is self-contained (compact lists, 4-byte twins, chunk headers, camera model,
 * descriptor), so this is transport and validation only.  While nobody calls them, every step, store, score, match, query, shift
 * search and verify issues exactly the launches, copies and synchronisations it issues without this feature.
 *
 * The blob, format version 1.  Little-endian.  Every offset counts from the start of the blob and is a multiple of 16.  The bytes are
 * fully determined by the key frames: two exports of the same key frames are byte-identical.
 *   Header, 80 bytes:  char magic[8] = "DVOKFAR1";  u32 version = 1;  u32 0;  u64 header_bytes = 80;  u64 record_bytes = 144;
 *     u64 total_bytes;  i32 n_key_frames;  i32 rows, cols, n_levels, first_shift (the exporting tracker's);  i32 places_level (-1: no
 *     descriptors);  i32 D (bytes of a descriptor, 0: none);  i32 0;  u64 table_checksum.
 *   Table at offset 80: n_key_frames records of 144 bytes, one per key frame in the order exported:  i64 origin id;  i32 origin stream;
 *     i32 0;  i64 origin frame number;  f32 K[4] = fx, fy, cx, cy (the bits the slot holds);  i32 N[DVO_MAX_LEVELS];
 *     i32 pt4_ok[DVO_MAX_LEVELS] (0 or 1; both zero beyond n_levels);  i32 has_desc;  i32 0;  u64 payload_offset;  u64 payload_bytes;
 *     u64 payload_checksum;  u64 0.
 *   Payload of one key frame: for l = 0 .. n_levels - 1 the slot's cpts[N_l] (8-byte words), cidx[N_l], cpt4[N_l] and
 *     chdr[ceil(N_l / 64)] (4-byte words), verbatim, then the D unpadded descriptor bytes where has_desc; every section zero-padded to a
 *     multiple of 16 bytes.  Where pt4_ok[l] == 0 the cpt4 and chdr sections are zeros (their slot content is not defined).
 *   Checksum of a byte range taken as u32 words w_0 .. w_{m-1}:  sum_i mix(w_i | (u64)(i + 1) << 32) mod 2^64,  mix = the splitmix64
 *     finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31).  It depends on position
 *     and not on the order of addition: one value whatever the shape of the reduction.  payload_checksum covers the key frame's
 *     payload, table_checksum the table.  It guards against truncation and bit rot; it is NOT a security boundary -- whoever can
 *     write a blob can write its checksums, so take blobs only from where you would take code.
 *
 * dvo_archive_blob_info(blob, bytes, info): host only, no tracker, no device.  Validates header and table -- magic, version, sizes
 *   (bytes must equal total_bytes), offsets in range and multiples of 16, payload sizes equal to what N, has_desc and D imply, no
 *   overlapping payloads, N >= 0, pt4_ok and has_desc in {0, 1}, zero padding, the table checksum -- and returns the geometry, the places
 *   level, D and the count.  (The struct shares its name with the function, like stat: write `struct dvo_archive_blob_info`.)
 *   DVO_ERR_INVALID with the defect named by dvo_last_error(NULL).
 * dvo_tracker_archive_export_size(tr, n, key_id, bytes): the size of the blob dvo_tracker_archive_export would write.  Host only.
 * dvo_tracker_archive_export(tr, n, key_id, blob, capacity, bytes): key_id == NULL exports every live key frame in ascending id,
 *   otherwise the n listed ones in the listed order (duplicates allowed, n = 0 gives a valid empty blob).  *bytes = the blob's size;
 *   capacity smaller than that: DVO_ERR_INVALID, nothing written.  Cost: the entry list's upload, DVO_TRACKER_EXPORT_LAUNCHES launch
 *   (dvo_tracker_archive_blob.hip: the ragged slots are gathered into a dense device staging buffer; while copying, the kernel forms
 *   each key frame's checksum and writes the records of the table), one copy of the blob to the caller's memory and ONE
 *   synchronisation.  The staging buffer is allocated or grown inside this call (not counted), never in a step;
 *   dvo_tracker_set_archive frees it.  A key frame made while places were off, or before a dvo_tracker_set_places, is exported with
 *   has_desc = 0.  The archive is only read.
 * dvo_tracker_archive_import(tr, blob, bytes, ids_out, ids_capacity, n_in_blob): the validation of dvo_archive_blob_info, and rows,
 *   cols, n_levels, first_shift equal to the tracker's; one upload of the blob; launch 1 recomputes the payload checksums on the
 *   device, a short record is read back (the ONE synchronisation) and compared on the host; launch 2 scatters the payloads into the
 *   next slots of the ring (lists, header, descriptor row and mark): DVO_TRACKER_IMPORT_LAUNCHES launches.  Nothing of the tracker
 *   changes unless every check passed.  Each key frame gets the next id and the next slot under the ring rule above, eviction counters
 *   included; a blob with more key frames than the ring has slots evicts its own earliest ones (they get ids, which are gone at
 *   once).  A key frame with N[l] above the archive's points_capacity[l] is refused like a native one: id -1, `refused` + 1, the others
 *   still go in.  Descriptors are taken only when places are on at the blob's places_level with the same D; otherwise the key frame
 *   comes without one and is never returned by a query.  An imported key frame is foreign: dvo_tracker_archive_info and
 *   dvo_tracker_place.stream report stream -1 (so rules (b) and (c) of dvo_tracker_query_places never apply to it) and the frame number
 *   of its origin.  It keeps its origin, which a re-export writes again: export from tracker A, import into B, re-export from B gives
 *   the bytes A gave.  ids_out receives min(n, ids_capacity) ids, *n_in_blob (may be NULL) receives n.
 * dvo_tracker_archive_origin(tr, id, origin_id, origin_stream, origin_frame): who made the key frame; a native one is its own origin.
 *   Any output pointer may be NULL.
 * dvo_tracker_archive_stats reports last_launches and last_syncs of export (1, 1) and import (2, 1) as for score and match.
 * DVO_ERR_STATE: the archive is off, or an id is unknown, refused or evicted.  DVO_ERR_INVALID: a NULL argument, n < 0, or any defect
 *   of the blob; dvo_tracker_last_error names it. */
#define DVO_TRACKER_EXPORT_LAUNCHES 1
#define DVO_TRACKER_IMPORT_LAUNCHES 2
struct dvo_archive_blob_info {
    int version;
    int rows, cols, n_levels, first_shift;
    int places_level;         /* -1: no descriptors */
    int D;                    /* 0: none */
    int n_key_frames;
    unsigned long long total_bytes;
};
int  dvo_archive_blob_info(const void *blob, size_t bytes, struct dvo_archive_blob_info *info);
int  dvo_tracker_archive_export_size(dvo_tracker *tr, int n, const long long *key_id, size_t *bytes);
int  dvo_tracker_archive_export(dvo_tracker *tr, int n, const long long *key_id, void *blob, size_t capacity, size_t *bytes);
int  dvo_tracker_archive_import(dvo_tracker *tr, const void *blob, size_t bytes, long long *ids_out, int ids_capacity, int *n_in_blob);
int  dvo_tracker_archive_origin(dvo_tracker *tr, long long id, long long *origin_id, int *origin_stream, long long *origin_frame);
/* What the last step issued (any pointer may be NULL): kernel launches (every launch of the library goes through one counting macro,
 * dvo_launch.h; per host thread), host synchronisations (blocking waits for the context stream; not counted: the upload paths'
 * waits for the copy of a pinned staging buffer that an earlier call submitted, which has finished by then since every step ends with
 * a synchronisation), stage calls (frame uploads per run + reference extractions + alignments), streams that switched key frame, and
 * reallocations of the reference-point slabs. */
int  dvo_tracker_get_stats(dvo_tracker *tr, int *kernel_launches, int *host_syncs, int *runs, int *key_frames, int *slab_growths);
/* the underlying context (pair = stream): dvo_get_level_report, dvo_get_ref_level, dvo_set_keep_warm2 ... */
dvo_ctx *dvo_tracker_context(dvo_tracker *tr);

/* ---- pose graphs: batched pose-graph optimisation on the device, with a host definition --------------------------------------
 * The back end for what the tracker produces: key-frame-relative poses (dvo_tracker_step*), their information
 * (dvo_tracker_get_information) and verified loop-closure edges (dvo_tracker_match, dvo_tracker_verify).  A dvo_graph_batch is a
 * stand-alone handle: it touches no dvo_ctx and no tracker, and the caller builds the graphs.  K graphs -- one per stream of a fleet or a
 * replay -- are solved in ONE launch, one workgroup per graph.
 * Conventions.  A pose is 12 doubles {R column-major, t}; node pose T_n = (R_n, t_n) maps node-frame points to the world:
 * X_w = R_n X_n + t_n.  An edge (i, j, Z, Omega, flags) measures Z ~ T_i^-1 T_j: exactly what dvo_tracker_step or dvo_tracker_match
 * returns when i is the key frame and j the current frame.  Tangent order [translation x, y, z, rotation x, y, z], right perturbation
 * T <- T Exp(d) with the full SE(3) exponential -- the engine's own update, so the tracker's H is an information matrix in this
 * convention up to the residual variance: dvo_graph_information.
 *   residual r = Log(Z^-1 T_i^-1 T_j), s^2 = r^T Omega r, cost = sum rho(s^2); rho = s^2, and on edges flagged DVO_GRAPH_EDGE_ROBUST
 *   Huber: s^2 if s <= huber_delta, else 2 huber_delta s - huber_delta^2 (weight w = min(1, huber_delta / s); 1 when s = 0 or
 *   huber_delta <= 0).  J_j = Jr^-1(r), J_i = -Jr^-1(r) Ad(T_j^-1 T_i), Jr^-1(r) = I + ad/2 + ad^2/12 - ad^4/720 (the truncation is part
 *   of the definition).
 * Algorithm (dvo_pose_graph.h is the definition; host and device run the same loop).  Per outer iteration, at most max_iterations:
 * every edge is linearised; per free node the diagonal block and b are summed over its incidence list in edge order; (H + lambda
 * diag H) x = -b is solved by block-Jacobi preconditioned CG (6 x 6 Cholesky per node, matrix-free operator; stops at sqrt(r^T z) <=
 * cg_tol sqrt(r0^T z0) or after cg_max_iterations, 0 = 12 n_nodes); the trial poses are T_n Exp(x_n), re-orthogonalised by the polar
 * factor; a trial whose robust cost does not increase is accepted (lambda <- max(lambda lambda_down, lambda_min)), any other -- a
 * non-finite cost or step included -- is rejected (lambda <- min(lambda lambda_up, lambda_max)).  The loop stops after an accepted step
 * with max|x| < step_tol or a cost decrease <= cost_tol cost (DVO_GRAPH_CONVERGED; a tolerance of 0 never stops the loop, not even at a
 * trial of exactly equal cost, so that with both at 0 only the two ends that follow remain), after max_iterations (DVO_GRAPH_MAX_ITERATIONS), or
 * at a rejection with lambda already lambda_max: DVO_GRAPH_CONVERGED if the trial was finite -- a step damped that far that still does
 * not lower the cost means the cost sits at its rounding floor, where a trial changes it by less than the error of the sum -- else
 * DVO_GRAPH_NUMERIC, as for a start cost that is not finite.  The two meanings of DVO_GRAPH_CONVERGED are told apart by the report:
 * lambda == lambda_max only after the second (an accepted step always lowers lambda below it).  Fixed nodes never change.
 * Log covers residual rotations up to and including pi: near a half turn the axis is taken from the symmetric part of the rotation and
 * only its sign from the antisymmetric part; at exactly pi either sign is the same rotation.
 * CONTRACT of the device: a graph's poses and report are bit-identical run to run, and identical whatever the batch size, the graph's
 * position in the batch and the other graphs (sums run over lanes, then waves in wave order; no atomics).  Against the host solver,
 * whose sums run in index order, they agree to rounding: poses to 1e-7, the cost to 1e-9 relative, on the cases of
 * tests/pose_graph_reference.py.
 * MARGINAL COVARIANCES.  How certain the poses are: the joint covariance of m listed nodes is the matching block of H^-1, H the undamped
 * Gauss-Newton matrix over the free nodes at the graph's poses, in the convention above (tangent order, right perturbation, the truncated
 * Jr^-1, Huber weights at the current residuals).  Every edge is linearised and every free node assembled as in an outer iteration, at
 * lambda = 0; per listed node c and k in 0..5 the column H x = e(c, k) is solved by the solver's CG loop (x = 0, r = e, z = Minv r, p = z;
 * the same stop rules, cg_tol and cg_max_iterations; fixed nodes stay zero; a listed fixed node has x = 0 and no iterations);
 * M[6a + q][6b + k] = x(nodes[b], k) at node nodes[a], component q, and cov = (M + M^T) / 2.  cov is exactly symmetric; its block (a, b)
 * depends on the graph, nodes[a] and nodes[b] alone, not on m, the other listed nodes or their order.  Status: DVO_GRAPH_NUMERIC (cov all
 * zero) when a free node's block has no Cholesky factor, and for a residual or a solution that is not finite; DVO_GRAPH_MAX_ITERATIONS
 * when a column stopped at the cap or at p^T A p <= 0 (cov is what the columns held); else DVO_GRAPH_CONVERGED.  Of the parameters only
 * huber_delta, cg_tol and cg_max_iterations are used.  UNIT: the covariance inherits the scale of the edges' information -- with edges
 * from dvo_graph_information that is the distance-transform residual's, relative and uncalibrated: compare covariances and chi-squares of
 * one graph with each other, or calibrate the scale of all edges alike first.
 * CONTRACT of the device (dvo_graph_marginals): a block (graph, nodes[a], nodes[b]) is bit-identical run to run and whatever the batch,
 * the graph's position in it, m, the other listed nodes and their order.  The call changes nothing a solve can see: the graph's poses
 * and last report are what they were, and a solve after it returns byte for byte what it returns without it.  Against the host
 * definition, whose sums run in index order, the device agrees to 100 times the host definition's own distance from the dense inverse
 * on the cases of tests/pose_graph_reference.py (profiles/pose_graph_marginals/README.md), relative to the largest entry of the block.
 * OUT OF SCOPE: more than one workgroup per graph; stronger preconditioners and sparse direct solves; the full covariance of all nodes,
 * a Takahashi / sparse-direct inverse, covariances in another gauge than the fixed nodes', a different m per graph of one call; robust
 * kernels other than Huber and switchable constraints; landmarks and calibration variables; graph construction inside the tracker;
 * incremental updates; graphs beyond DVO_GRAPH_MAX_NODES / DVO_GRAPH_MAX_EDGES. */
#ifndef DVO_GRAPH_TYPES_DEFINED_
#define DVO_GRAPH_TYPES_DEFINED_
#define DVO_GRAPH_EDGE_ROBUST 1          /* edge flag: Huber instead of the plain square */
#define DVO_GRAPH_MAX_NODES 4096         /* per graph */
#define DVO_GRAPH_MAX_EDGES 32768        /* per graph */
#define DVO_GRAPH_CONVERGED 0            /* report status: an accepted step met step_tol or cost_tol, or no damping improves the cost */
#define DVO_GRAPH_MAX_ITERATIONS 1       /* max_iterations outer iterations ran */
#define DVO_GRAPH_NUMERIC 2              /* a cost or step that is not finite, at the start or still at lambda_max */
typedef struct dvo_graph_edge {
    int    i, j;                         /* nodes: Z measures T_i^-1 T_j */
    double R[9];                         /* Z's rotation, column-major like every R of this header */
    double t[3];                         /* Z's translation */
    double info[36];                     /* Omega, symmetric positive definite, tangent order [translation, rotation] */
    int    flags;                        /* 0 or DVO_GRAPH_EDGE_ROBUST */
} dvo_graph_edge;
typedef struct dvo_graph_params {
    int    max_iterations;               /* outer (Levenberg-Marquardt) iterations */
    int    cg_max_iterations;            /* 0: 12 * n_nodes */
    double lambda0, lambda_up, lambda_down, lambda_min, lambda_max;
    double cg_tol, step_tol, cost_tol;
    double huber_delta;                  /* <= 0: robust edges are plain */
} dvo_graph_params;
typedef struct dvo_graph_report {
    double cost0, cost, lambda, max_step;
    int    iterations, accepted, cg_iterations, status;
} dvo_graph_report;
#endif
#ifndef DVO_GRAPH_MARGINAL_TYPES_DEFINED_
#define DVO_GRAPH_MARGINAL_TYPES_DEFINED_
#define DVO_GRAPH_MARGINAL_MAX_NODES 16  /* nodes of one query */
typedef struct dvo_graph_marginal_report {
    double worst_residual;               /* max over the columns of sqrt(r^T z) / sqrt(r0^T z0) at the stop */
    int    cg_iterations;                /* sum over the columns */
    int    cg_iterations_max;            /* the longest column */
    int    status;                       /* DVO_GRAPH_CONVERGED / _MAX_ITERATIONS / _NUMERIC */
} dvo_graph_marginal_report;
#endif
#define DVO_GRAPH_LAUNCHES 1             /* per dvo_graph_solve, whatever count is; a constant of the build */
#define DVO_GRAPH_MARGINAL_LAUNCHES 2    /* per dvo_graph_marginals, whatever count and m are; a constant of the build */
typedef struct dvo_graph_batch dvo_graph_batch;
/* max_iterations 50, cg_max_iterations 0, lambda0 1e-4, lambda_up 10, lambda_down 0.1, lambda_min 1e-12, lambda_max 1e12, cg_tol 1e-6,
 * step_tol 1e-10, cost_tol 1e-14, huber_delta 1.0 */
int  dvo_graph_params_default(dvo_graph_params *p);
/* The definition on the host, no device and no handle needed; every sum in index order.  p NULL = defaults.  poses12 (12 n_nodes
 * doubles) is updated in place; fixed[n] != 0 holds node n.  report receives cost0, the final cost and lambda, max|x| of the last accepted
 * step, the outer iterations run and accepted, the CG iterations in total and the status; cost_trace (may be NULL with capacity 0)
 * receives cost0 and the cost after every outer iteration, iterations + 1 entries, as far as it has room.
 * DVO_ERR_INVALID, nothing written: a NULL poses12, fixed or report, NULL edges with n_edges > 0, a trace buffer that does not match its
 * capacity; n_nodes < 1, n_nodes above DVO_GRAPH_MAX_NODES or n_edges above DVO_GRAPH_MAX_EDGES; an edge index out of range or i == j; a
 * number anywhere that is not finite; an info that is not symmetric to 1e-9 relative or has no Cholesky factor; unknown flags; a
 * connected component without a fixed node (its gauge is free); parameters out of range: a count < 0, lambda_up <= 1, lambda_down outside
 * (0, 1), a negative lambda or tolerance, lambda_max < lambda_min.  n_edges = 0 with every node fixed is valid and returns the input. */
int  dvo_graph_solve_host(const dvo_graph_params *p, int n_nodes, double *poses12, const unsigned char *fixed, int n_edges,
                          const dvo_graph_edge *edges, dvo_graph_report *report, double *cost_trace, int trace_capacity);
/* A handle for up to max_graphs graphs that together hold at most max_nodes_total nodes and max_edges_total edges; the resident arrays
 * and the workspace (960 bytes per edge, 720 per node) are allocated here.  DVO_ERR_NO_DEVICE without a HIP device (no CPU fallback),
 * DVO_ERR_NOMEM when they do not fit, DVO_ERR_INVALID for capacities below 1 (edges: below 0) and for max_graphs above max_nodes_total
 * (a graph has at least one node).  The block the results come back in (report, trace and poses of every listed graph) is allocated
 * by the first solve and again by a solve that needs a larger one (a larger max_iterations, more listed nodes). */
int  dvo_graph_create(int max_graphs, int max_nodes_total, int max_edges_total, dvo_graph_batch **out);
int  dvo_graph_destroy(dvo_graph_batch *b);
const char *dvo_graph_last_error(const dvo_graph_batch *b);               /* b may be NULL: last creation error */
/* Graph `graph` becomes the given one: validated and staged on the host, no device work; it goes up with the next solve that lists it.
 * Refused with DVO_ERR_INVALID, the graph in place unchanged: a graph outside [0, max_graphs), what dvo_graph_solve_host refuses in a
 * graph, and a total over the set graphs above the handle's capacities. */
int  dvo_graph_set(dvo_graph_batch *b, int graph, int n_nodes, const double *poses12, const unsigned char *fixed, int n_edges,
                   const dvo_graph_edge *edges);
/* Solve graphs[0 .. count) (p NULL = defaults): one upload of the list and of the listed graphs set since they last went up,
 * DVO_GRAPH_LAUNCHES launch, one copy back, one synchronisation.  Solving again continues from the solved poses.  Refused, nothing
 * changed: DVO_ERR_INVALID count outside [1, max_graphs], a NULL list, a graph outside range or listed twice, parameters out of range;
 * DVO_ERR_STATE a listed graph that was never set. */
int  dvo_graph_solve(dvo_graph_batch *b, const dvo_graph_params *p, int count, const int *graphs);
/* the graph's current poses (as set, or as last solved); no device access.  DVO_ERR_STATE: never set */
int  dvo_graph_get_poses(dvo_graph_batch *b, int graph, double *poses12);
/* the report and trace of the graph's last solve, as dvo_graph_solve_host gives them; no device access.  DVO_ERR_STATE: not solved since
 * it was set */
int  dvo_graph_get_report(dvo_graph_batch *b, int graph, dvo_graph_report *report, double *cost_trace, int trace_capacity);
/* what the last solve or marginals call issued (either pointer may be NULL): kernel launches (counted as for dvo_tracker_get_stats) and
 * host synchronisations */
int  dvo_graph_stats(dvo_graph_batch *b, int *last_launches, int *last_syncs);
/* The definition of the marginal covariances on the host ("MARGINAL COVARIANCES" above), no device and no handle needed; every sum in
 * index order.  p NULL = defaults.  The joint covariance of nodes[0 .. m) at the given poses -> cov, (6 m)^2 doubles row-major, node
 * nodes[a]'s tangent components at rows and columns 6 a .. 6 a + 5; the rows and columns of a fixed node are zero.
 * DVO_ERR_INVALID, nothing written: everything dvo_graph_solve_host refuses in parameters and graph; m outside
 * [1, DVO_GRAPH_MARGINAL_MAX_NODES]; a NULL nodes, cov or report; a node out of range or listed twice.  A graph with no free node is
 * valid and gives zeros. */
int  dvo_graph_marginals_host(const dvo_graph_params *p, int n_nodes, const double *poses12, const unsigned char *fixed, int n_edges,
                              const dvo_graph_edge *edges, int m, const int *nodes, double *cov, dvo_graph_marginal_report *report);
/* The same on the device for graphs[0 .. count), each at its CURRENT poses (as set, or as last solved; a graph set and never solved goes
 * up as it would with a solve): nodes holds m nodes per listed graph, cov count * (6 m)^2 doubles, reports count records.  One upload,
 * DVO_GRAPH_MARGINAL_LAUNCHES launches (prepare: one workgroup per graph; columns: one per graph, node and k), one copy back, one
 * synchronisation, counted in dvo_graph_stats; the symmetrisation runs on the host.  A graph above 681 nodes keeps its columns' CG
 * vectors in a workspace of 240 bytes per node and column, allocated by the first call that needs it and grown on demand.  Refused,
 * nothing changed: DVO_ERR_INVALID what dvo_graph_solve and dvo_graph_marginals_host refuse in their arguments; DVO_ERR_STATE a listed
 * graph that was never set; DVO_ERR_NOMEM a workspace that does not fit. */
int  dvo_graph_marginals(dvo_graph_batch *b, const dvo_graph_params *p, int count, const int *graphs, int m, const int *nodes, double *cov,
                         dvo_graph_marginal_report *reports);
/* The gate for a loop-closure candidate: is `edge`, a measurement of T_i^-1 T_j, compatible with what the graph believes about nodes i
 * and j?  r = Log(Z^-1 T_i^-1 T_j) with its Jacobians J_i, J_j as in the definition; S = [J_i J_j] cov [J_i J_j]^T + Omega^-1, cov144 the
 * joint covariance of (i, j) from a marginals call on the nodes {i, j} in this order (NULL = zero: the poses are taken as certain);
 * chi2 = r^T S^-1 r, to be compared with a chi-square quantile of 6 degrees of freedom of the caller's choice -- in the unit of the
 * edges' information (see UNIT above).  The robust flag plays no part.  r6, S36 (row-major), chi2: any may be NULL.  Host only.
 * DVO_ERR_INVALID, nothing written: a NULL pose or edge, a number that is not finite, an Omega or an S without a Cholesky factor. */
int  dvo_graph_edge_chi2(const double *pose_i12, const double *pose_j12, const double *cov144, const dvo_graph_edge *edge, double *r6,
                         double *S36, double *chi2);
/* An edge's Omega from a tracker information record or a score record: info36 = H36 (n_visible - 6) / sum_eps2, the inverse of
 * dvo_amd::poseCovariance, in the units of the distance-transform residual (a relative, uncalibrated scale; rescale all edges alike or
 * not at all).  DVO_ERR_INVALID, nothing written, under poseCovariance's conditions -- n_visible <= 6, an H that is not finite or has no
 * Cholesky factor -- and for a NULL argument or a sum_eps2 that is not positive and finite. */
int  dvo_graph_information(const double *H36, double sum_eps2, int n_visible, double *info36);

/* ---- depth fusion: depth frames at given poses into truncated-signed-distance volumes, and their surface as points ---------------
 * The map side of what the tracker and the pose graphs produce: depth images plus (optimised) poses in, a model of the scene out.  A
 * dvo_tsdf_batch is a stand-alone handle: it touches no dvo_ctx and no tracker.  It owns a pool of voxels for several volumes -- one
 * per stream of a fleet, or one per region -- and fuses any list of frames into them in ONE launch.
 * Conventions.  A volume is nx * ny * nz voxels; voxel (ix, iy, iz) is stored at index ix + nx * (iy + ny * iz) and its centre lies at
 * origin + voxel_size * (ix, iy, iz) in the world.  One voxel is one 32-bit word: low 16 bits q (int16: the truncated distance in units
 * of trunc / 32767), high 16 bits w (uint16: the observation count).  Word 0 = never seen, so clearing is a fill with zero.  A frame is a
 * depth image (rows x cols, row-major, DVO_DEPTH_U16 millimetres or DVO_DEPTH_F32 metres; a pinhole camera K4 = fx, fy, cx, cy, the image
 * taken as undistorted and registered) and a pose of 12 doubles {R column-major, t}, camera to world: what dvo_graph_get_poses returns.
 * Definition (rgbd_odometry_amd/csrc/dvo_tsdf_map.h; IEEE double in the order written, nothing fused, no transcendental function, no
 * float).  One frame into one volume, per voxel:
 *   wx = origin[0] + voxel_size * ix (wy, wz alike: always the direct formula); dx = wx - t[0] (dy, dz alike);
 *   X = R[0] dx + R[1] dy + R[2] dz, Y = R[3] dx + R[4] dy + R[5] dz, Z = R[6] dx + R[7] dy + R[8] dz; skip unless Z > z_near;
 *   iz = 1 / Z, u = fx (X iz) + cx, v = fy (Y iz) + cy, ui = floor(u + 0.5), vi = floor(v + 0.5); skip unless 0 <= ui < cols and
 *   0 <= vi < rows (compared in double: NaN falls out here); D = metres of depth[vi][ui] (U16: 0 is a hole, else r / 1000; F32: not
 *   finite or <= 0 is a hole); skip a hole and D > z_far; sdf = D - Z; skip if sdf < -trunc; f = min(sdf (1 / trunc), 1), F = 32767 f;
 *   q' = (int)rint((q w + F) / (w + 1)) (round half to even), w' = min(w + 1, max_weight).
 * A skipped voxel keeps its word.  A frame list is applied in list order: the result is that of integrating the frames one at a time.
 * Surface points (min_weight >= 1): visit the voxels a in index order and for each the axes x, y, z in this order, b the next voxel
 * along the axis; skip when b is out of bounds or either weight is below min_weight; a crossing is (qa < 0) != (qb < 0); then
 * lambda = qa / (qa - qb) and the point is the centre of a moved by lambda voxel_size along the axis, output as three floats.  The order
 * of the output is part of the definition.
 * CONTRACT of the device: every result -- the words after dvo_tsdf_integrate, the points and their count -- is byte-equal to the host
 * definition, whatever the batch: one call of many frames, one call per frame, and the listed volumes in any order (each volume's own
 * frames in theirs) give the same bytes.  Every voxel is one thread's: no atomics, no communication between workgroups.
 * OUT OF SCOPE: hashed or unbounded volumes, de-integration, a distorted or unregistered depth image, float arithmetic. */
#ifndef DVO_TSDF_TYPES_DEFINED_
#define DVO_TSDF_TYPES_DEFINED_
#define DVO_TSDF_MAX_DIM 1024            /* voxels along one axis */
typedef struct dvo_tsdf_volume {
    int    nx, ny, nz;                   /* each in [1, DVO_TSDF_MAX_DIM]; voxel (ix, iy, iz) at index ix + nx * (iy + ny * iz) */
    double voxel_size;                   /* metres, > 0 */
    double origin[3];                    /* world position of the centre of voxel (0, 0, 0) */
    double trunc;                        /* truncation distance, metres, > 0 */
} dvo_tsdf_volume;
typedef struct dvo_tsdf_params {
    double z_near, z_far;                /* metres: a voxel at camera depth <= z_near, a measurement beyond z_far are skipped */
    int    max_weight;                   /* the observation count saturates here: [1, 65535] */
} dvo_tsdf_params;
#endif
#define DVO_TSDF_INTEGRATE_LAUNCHES 1    /* per dvo_tsdf_integrate, whatever count is; a constant of the build */
#define DVO_TSDF_EXTRACT_LAUNCHES 3      /* per dvo_tsdf_extract_points: count, scan, write; a constant of the build */
typedef struct dvo_tsdf_batch dvo_tsdf_batch;
/* z_near 0.1, z_far 8.0, max_weight 128 */
int  dvo_tsdf_params_default(dvo_tsdf_params *p);
/* The definition on the host, no device and no handle needed: frames 0 .. count - 1, in this order, into the nx * ny * nz words of one
 * volume.  depth[i]: rows x cols of depth_format; K4: 4 doubles per frame; poses12: 12 per frame.
 * DVO_ERR_INVALID, nothing written: a NULL argument (a depth[i] included); a dimension outside [1, DVO_TSDF_MAX_DIM], a voxel_size or
 * trunc that is not positive and finite, an origin that is not finite; parameters out of range (0 < z_near < z_far, both finite,
 * max_weight in [1, 65535]); count, rows or cols < 1; an unknown format; a K4 or pose that is not finite, fx or fy not positive.  R is
 * taken as given (not checked for orthogonality). */
int  dvo_tsdf_integrate_host(const dvo_tsdf_volume *vol, unsigned *voxels, const dvo_tsdf_params *p, int count, const void *const *depth,
                             int depth_format, int rows, int cols, const double *K4, const double *poses12);
/* The surface points of a volume on the host: *n_points = how many there are, the first `capacity` of them -> xyz (3 floats each; xyz may
 * be NULL with capacity 0).  DVO_ERR_INVALID, nothing written: a NULL vol, voxels or n_points, a bad volume, min_weight < 1, capacity < 0,
 * a NULL xyz with capacity > 0. */
int  dvo_tsdf_extract_host(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long capacity,
                           long long *n_points);
/* A handle for up to max_volumes volumes that together hold at most max_voxels_total voxels: the pool (4 bytes per voxel) is allocated
 * here.  DVO_ERR_NO_DEVICE without a HIP device (no CPU fallback), DVO_ERR_NOMEM when the pool cannot be allocated (always above 2^38
 * voxels), DVO_ERR_INVALID for a capacity below 1 and for max_volumes above max_voxels_total (a volume has at least one voxel).  The blocks a call stages its
 * descriptors and images in, and an extraction's points come back in, are allocated by the first call that needs them and again by a
 * call that needs larger ones. */
int  dvo_tsdf_create(int max_volumes, long long max_voxels_total, dvo_tsdf_batch **out);
int  dvo_tsdf_destroy(dvo_tsdf_batch *b);
const char *dvo_tsdf_last_error(const dvo_tsdf_batch *b);                 /* b may be NULL: last creation error */
/* Volume `volume` gets this geometry and is cleared.  Volumes are placed in the pool back to back in the order they are set; a volume
 * set again keeps its place when its voxel count is unchanged, and the volume placed last may also change its count.  Refused with
 * DVO_ERR_INVALID, everything as it was: a volume outside [0, max_volumes), what dvo_tsdf_integrate_host refuses in a volume, another
 * count for a volume that is not the last placed, a total above max_voxels_total. */
int  dvo_tsdf_set_volume(dvo_tsdf_batch *b, int volume, const dvo_tsdf_volume *vol);
/* every word of the volume becomes 0 (never seen); the geometry stays.  DVO_ERR_STATE: never set */
int  dvo_tsdf_clear(dvo_tsdf_batch *b, int volume);
/* Fuse frames 0 .. count - 1: frame i -- depth[i], K4 + 4 i, poses12 + 12 i -- into volume volumes[i].  A volume may be listed several
 * times: its frames are applied in list order.  flags 0: the images are host memory and are staged by the call; DVO_UPLOAD_DEVICE: they
 * are device pointers of the handle's GPU, read in place.  Either way: one upload (descriptors, and the images when staged),
 * DVO_TSDF_INTEGRATE_LAUNCHES launch -- the thread that owns a voxel applies all its volume's frames in registers, so the volume crosses
 * HBM once per call, not once per frame -- and one synchronisation: the buffers are borrowed only until the call returns.  Re-fusing
 * after a pose-graph solve is dvo_tsdf_clear plus one call with the whole key-frame list.  Refused, nothing changed: DVO_ERR_INVALID a
 * NULL argument (a depth[i] included), parameters out of range, count, rows or cols < 1, an unknown format or flag, a listed volume
 * outside [0, max_volumes), a K4 or pose that is not finite, fx or fy not positive; DVO_ERR_STATE a listed volume that was never set. */
int  dvo_tsdf_integrate(dvo_tsdf_batch *b, const dvo_tsdf_params *p, int count, const int *volumes, const void *const *depth, int depth_format,
                        int rows, int cols, const double *K4, const double *poses12, int flags);
/* The volume's surface points in the definition's order: *n_points = the full count, the first `capacity` points -> xyz (may be NULL with
 * capacity 0).  DVO_TSDF_EXTRACT_LAUNCHES launches (count per workgroup, scan of the counts by one workgroup, write), one copy back of the
 * count and min(capacity, 3 nx ny nz) points, one synchronisation.  The volume's words are not changed.  Refused: DVO_ERR_INVALID
 * min_weight < 1, capacity < 0, a NULL xyz with capacity > 0, a NULL n_points, a volume outside range; DVO_ERR_STATE never set. */
int  dvo_tsdf_extract_points(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, long long capacity, long long *n_points);
/* the volume's nx * ny * nz words out of and into the pool: persistence, and inspection.  DVO_ERR_INVALID a NULL buffer or a volume
 * outside range; DVO_ERR_STATE never set */
int  dvo_tsdf_get_voxels(dvo_tsdf_batch *b, int volume, unsigned *out);
int  dvo_tsdf_set_voxels(dvo_tsdf_batch *b, int volume, const unsigned *in);
/* what the last dvo_tsdf_integrate, dvo_tsdf_extract_points, dvo_raycast_views or dvo_mesh_extract, or the colour variant of one of them,
 * issued (either pointer may be NULL): kernel launches (counted as for dvo_tracker_get_stats) and host synchronisations --
 * DVO_MESH_LAUNCHES and 1 after a mesh call.  Also after dvo_esdf_update (DVO_ESDF_UPDATE_LAUNCHES and 1), dvo_esdf_get_distances and
 * dvo_esdf_query (1 and 1 each) of the distance-field section */
int  dvo_tsdf_stats(dvo_tsdf_batch *b, int *last_launches, int *last_syncs);

/* ---- from the map back to depth: fused volumes ray-cast into depth and normal maps -------------------------------------------------
 * The predicted view of the model from any pose, in the formats the rest of the engine consumes: a rendered depth image goes into
 * dvo_tsdf_integrate, dvo_tracker_step or dvo_tracker_verify as a camera's would.  A view is a volume, K4 = fx, fy, cx, cy and a pose of
 * 12 doubles {R column-major, t}, camera to world; rows x cols and the depth format are shared by a call.
 * Definition (rgbd_odometry_amd/csrc/dvo_tsdf_raycast.h; IEEE double in the order written, nothing fused, no transcendental function;
 * sqrt and division in double, both correctly rounded).  Pixel (u, v):
 *   xn = ((double)u - cx) / fx, yn = ((double)v - cy) / fy; the point at camera depth Z is Pc = (xn Z, yn Z, Z), Pw = R Pc + t,
 *   g = (Pw - origin) inv_vs with inv_vs = 1.0 / voxel_size;
 *   sample S(g): i = floor(g), f = g - i per axis; valid iff 0 <= i and i + 1 <= n - 1 on every axis (a NaN fails) and all eight corner
 *   words have w >= min_weight; its value is the trilinear interpolation of the eight q as doubles, along x, then y, then z, each step
 *   a + f (b - a).  A volume with a dimension of 1 has no valid sample;
 *   march: step = step_trunc * trunc; sample k at Z_k = z_near + step (double)k, k = 0, 1, ... while Z_k <= z_far; the ray ends at the
 *   first valid sample with S <= 0: a hit iff sample k - 1 exists and was valid with S_prev > 0, else a hole (the ray started inside or
 *   behind a surface); on a hit Z* = Z_{k-1} + step (S_prev / (S_prev - S_cur)); a ray that passes z_far without ending is a hole;
 *   depth: DVO_DEPTH_F32 (float)Z*, a hole 0.0f; DVO_DEPTH_U16 m = rint(Z* 1000.0), a hole 0, m outside [1, 65535] a hole;
 *   normal (three floats, world axes): with g* the voxel coordinates of the point at Z*, G = (S(g* + ex) - S(g* - ex), S(g* + ey) -
 *   S(g* - ey), S(g* + ez) - S(g* - ez)) and the normal is (float)(G_k / sqrt(G.G)); (0, 0, 0) for a hole, when one of the six samples is
 *   invalid or when G.G is not > 0.  q is positive in front of a surface: the normal points to the viewer's side.
 * step_trunc <= 0.5 keeps both samples that bracket the surface inside the unsaturated band for ordinary fields of view; at 1.0 the
 * bracket reaches clamped values and Z* is biased (on a fused plane the worst error grew from 6e-7 m to 1.9e-4 m).
 * CONTRACT of the device: every image is byte-equal to the host definition, whatever the batch: all views in one call, one call per
 * view and any order of the list give the same bytes.  Every pixel is one thread's; the pool is only read. */
#ifndef DVO_RAYCAST_TYPES_DEFINED_
#define DVO_RAYCAST_TYPES_DEFINED_
#define DVO_RAYCAST_MAX_STEPS 65536      /* samples of one view's march */
typedef struct dvo_raycast_params {
    double z_near, z_far;                /* metres: the first sample's camera depth, and the depth no sample lies beyond */
    double step_trunc;                   /* the march's step in units of the volume's trunc: (0, 1] */
    int    min_weight;                   /* a sample needs this many observations in all eight corners: [1, 65535] */
} dvo_raycast_params;
#endif
#define DVO_RAYCAST_LAUNCHES 1           /* per dvo_raycast_views, whatever count is; a constant of the build */
/* z_near 0.1, z_far 8.0, step_trunc 0.5, min_weight 1 */
int  dvo_raycast_params_default(dvo_raycast_params *p);
/* The definition on the host, no device and no handle needed: views 0 .. count - 1 of ONE volume (its nx * ny * nz words).  K4: 4
 * doubles per view; poses12: 12 per view; depth_out[i]: rows x cols of depth_format; normals_out: NULL, or normals_out[i] 3 rows x cols
 * floats.  DVO_ERR_INVALID, nothing written: a NULL argument (a depth_out[i], and a normals_out[i] of a non-NULL list, included); what
 * dvo_tsdf_integrate_host refuses in a volume, a K4 or a pose; a parameter that is not finite, anything other than 0 < z_near < z_far,
 * step_trunc outside (0, 1], min_weight outside [1, 65535]; a march of more than DVO_RAYCAST_MAX_STEPS samples; count, rows or cols < 1;
 * an unknown format. */
int  dvo_raycast_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const dvo_raycast_params *p, int count, int depth_format, int rows,
                      int cols, const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out /* may be NULL */);
/* Views 0 .. count - 1 on the device: view i looks at volume volumes[i] of the handle.  One upload of the view records,
 * DVO_RAYCAST_LAUNCHES launch for the whole list (one thread per pixel) and one synchronisation.  flags 0: the outputs are host memory,
 * filled by one copy back; DVO_UPLOAD_DEVICE: they are device pointers of the handle's GPU, written in place, and nothing is copied back
 * -- a rendered depth goes straight into dvo_tsdf_integrate(..., DVO_UPLOAD_DEVICE) or the tracker.  No voxel is changed.  Refused,
 * nothing written: DVO_ERR_INVALID as dvo_raycast_host, and for a listed volume outside [0, max_volumes) or an unknown flag;
 * DVO_ERR_STATE a listed volume that was never set. */
int  dvo_raycast_views(dvo_tsdf_batch *b, const dvo_raycast_params *p, int count, const int *volumes, int depth_format, int rows, int cols,
                       const double *K4, const double *poses12, void *const *depth_out, float *const *normals_out /* may be NULL */, int flags);

/* ---- the surface as a triangle mesh: fused volumes into vertices and triangles, extracted on the device -----------------------------
 * What a viewer, a planner's collision geometry or a comparison against a CAD model consumes.  Marching tetrahedra on the Kuhn split of
 * the voxel lattice: no case table to transcribe, no ambiguous case, consistent between neighbouring cells by construction.
 * Conventions.  Volumes, words and min_weight as in the fusion section.  A vertex is three floats in the world; a triangle is three
 * 32-bit vertex numbers, its normal (right-hand rule) pointing from the inside (q < 0) to the outside -- to the viewer's side, like the
 * ray caster's normals.  The order of vertices and of triangles is part of the definition.
 * Definition (rgbd_odometry_amd/csrc/dvo_tsdf_mesh.h; IEEE double in the order written, nothing fused).
 *   Vertices: voxel a = (ix, iy, iz) owns seven lattice edges, direction d = 0, 1, 2: the axes (1,0,0), (0,1,0), (0,0,1); d = 3, 4, 5: the
 *   face diagonals (1,1,0), (1,0,1), (0,1,1); d = 6: the body diagonal (1,1,1); b = a + dir(d).  The edge carries a vertex iff b is inside
 *   the volume, both weights are >= min_weight and (qa < 0) != (qb < 0) -- the crossing rule of the surface points; then
 *   lambda = qa / (qa - qb) and the vertex is the centre of a (the direct formula) with lambda voxel_size added to every component whose
 *   direction component is 1, output as three floats.  Vertices are numbered in voxel index order and, within a voxel, in the order of d:
 *   the vertices with d < 3, taken in order, are byte for byte the points of dvo_tsdf_extract_host with the same min_weight.
 *   Cells: cell a exists when ix + 1 < nx, iy + 1 < ny and iz + 1 < nz; its corners are c_k = a + (k & 1, (k >> 1) & 1, (k >> 2) & 1); it is
 *   valid iff all eight corners have w >= min_weight (the validity of a ray-cast sample).  A valid cell is split into six tetrahedra, one
 *   per permutation p of the axes (0, 1, 2) in lexicographic order: v0 = c_0, v1 = c_[1 << p0], v2 = c_[(1 << p0) | (1 << p1)], v3 = c_7.
 *   Every edge of every tetrahedron is an owned edge of a corner voxel of the cell; E(i, j) = the vertex on the edge between v_i and v_j.
 *   Triangles of one tetrahedron, the inside corners being those with q < 0: none or four inside, nothing; one corner i that differs from
 *   the other three j < k < l: (E(i,j), E(i,k), E(i,l)); two inside i < j and two outside k < l: (E(i,k), E(i,l), E(j,l)) then (E(i,k),
 *   E(j,l), E(j,k)).  The second and third index are swapped when the orientation above needs it; the sign is decided on the unit lattice
 *   with every vertex at its edge's midpoint, so it depends on (p, inside mask) alone: a table the header generates at compile time.
 *   Triangles are numbered in cell index order, then p, then as listed.
 * Properties, none of them a defect: a vertex whose surrounding cells are all invalid or outside the volume is referenced by no triangle
 * (only at the rim of the observed region); a voxel with q == 0 exactly is "outside" with lambda = 0, its vertices coincide with its
 * centre and the triangles between them have zero area, their indices still distinct; no vertex is shared across a sign-consistent pair,
 * and the mesh of a closed surface that lies wholly inside valid cells is a closed oriented 2-manifold.
 * CONTRACT of the device: vertices, triangles and both counts are byte-equal to the host definition, whatever the capacities and
 * whatever ran on the handle before.  No atomics, no communication between workgroups; the volume's words are only read.
 * OUT OF SCOPE: marching cubes, vertex normals, welding of coincident vertices, removal of unreferenced vertices or zero-area
 * triangles, several volumes per call, simplification. */
#define DVO_MESH_LAUNCHES 4              /* per dvo_mesh_extract: count, scan, vertices, triangles; a constant of the build whatever the volume */
/* The definition on the host, no device and no handle needed.  *n_vertices and *n_triangles are always the full counts; the first
 * vertex_capacity vertices -> xyz (3 floats each) and the first triangle_capacity triangles -> tri (3 ints each); either buffer may be
 * NULL with capacity 0: counting with two zero capacities and then calling again is the intended use.  A triangle may reference a vertex
 * beyond vertex_capacity: a complete mesh needs both capacities to be at least the counts.  DVO_ERR_INVALID, nothing written: a NULL
 * vol, voxels, n_vertices or n_triangles, a bad volume, min_weight < 1, a capacity < 0, a NULL buffer with its capacity > 0; and a mesh
 * of more than 2^31 - 1 vertices (32-bit indices), refused after the counts are set and before anything else is written -- that needs a
 * volume of gigabytes and is not tested.  DVO_ERR_NOMEM: no memory for the 6 bytes per voxel the call works in. */
int  dvo_mesh_host(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long vertex_capacity, int *tri,
                   long long triangle_capacity, long long *n_vertices, long long *n_triangles);
/* The mesh of one volume of the handle on the device, with dvo_mesh_host's meaning of buffers, capacities and counts.  DVO_MESH_LAUNCHES
 * launches and one synchronisation.  flags 0: xyz and tri are host memory, filled by one copy back of the counts and min(capacity, count
 * bound) entries each; DVO_UPLOAD_DEVICE: they are device pointers of the handle's GPU, written in place, and only the two counts come
 * back.  The call works in 5 bytes of device scratch per voxel of the volume, allocated by the first call that needs it and again by a
 * call on a larger volume, before anything is enqueued: DVO_ERR_NOMEM when that fails, everything as it was.  The volume's words are
 * never changed.  Refused, nothing written: DVO_ERR_INVALID min_weight < 1, a capacity < 0, a NULL buffer with its capacity > 0, a NULL
 * count, an unknown flag, a volume outside range, more than 2^31 - 1 vertices (counts set); DVO_ERR_STATE a volume that was never set. */
int  dvo_mesh_extract(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, long long vertex_capacity, int *tri, long long triangle_capacity,
                      long long *n_vertices, long long *n_triangles, int flags);

/* ---- colour in the map: colour images fused beside the depth, coloured ray-cast views and coloured meshes ---------------------------
 * The tracker takes colour cameras; with this section the map keeps what they saw.  A coloured ray-cast view is an image plus a depth:
 * what dvo_tracker_step takes from a camera, rendered from the model.  Nothing of the sections above changes: a handle on which
 * dvo_colour_enable was never called does what it did, and every uncoloured result of a colour call -- words, depth, normals,
 * vertices, triangles, counts -- is byte-equal to its uncoloured sibling's.
 * Definition (rgbd_odometry_amd/csrc/dvo_tsdf_colour.h).
 *   Colour word: one 64-bit word per voxel in a second pool laid out exactly like the voxel pool (same offsets, same index
 *   ix + nx (iy + ny iz)).  Bits 0-15 r, 16-31 g, 32-47 b: the running mean of the channel in units of 1/256 of an 8-bit level, 0 ..
 *   65280; bits 48-63 wc, the colour observation count.  Word 0 = no colour yet, so clearing is a fill with zero.  Sixteen-bit channels
 *   on purpose: with 8-bit storage and max_weight 128 a running mean stops moving for changes below 65 levels.
 *   Fusing a frame: the depth frame of the fusion section plus an image of the same rows x cols, registered to the depth, DVO_CAM_BGR8,
 *   DVO_CAM_RGB8 or DVO_CAM_MONO8 (a value g stands for (g, g, g)).  Per voxel the TSDF word is updated exactly as above; the colour word
 *   is updated iff the voxel was not skipped (every test up to and including sdf >= -trunc passed) and sdf <= trunc, compared in double
 *   (sdf == trunc is in): free space further than trunc in front of a surface takes no colour.  The pixel is the one at (vi, ui) the
 *   depth was read from, channels C = R, G, B as integers 0 .. 255.  Integer arithmetic only, per channel
 *   c' = (c wc + 256 C + ((wc + 1) >> 1)) / (wc + 1), the division truncating (the mean rounds half up; all of it fits in 32 unsigned
 *   bits), and wc' = min(wc + 1, max_weight).  A frame list is applied in list order.
 *   A ray-cast pixel's colour: on a hit (after the u16 rule that turns m outside [1, 65535] into a hole) g* = the voxel coordinates of
 *   the point at Z* (the point the normal uses); i = floor(g*), f = g* - i per axis with the bounds test of a sample; all eight corner
 *   colour words need wc >= 1 (TSDF weights are not consulted); each channel is the trilinear interpolation of the eight values as
 *   doubles, along x, then y, then z, each step a + f (b - a); the level is L = (int)floor(c / 256.0 + 0.5), clamped to [0, 255].  A
 *   hole, an out-of-bounds cell or a corner without colour gives (0, 0, 0).  DVO_CAM_RGB8 writes (R, G, B), DVO_CAM_BGR8 (B, G, R),
 *   DVO_CAM_MONO8 the engine's grey (1868 B + 9617 G + 4899 R + 8192) >> 14.
 *   A mesh vertex's colour: the vertex lies on the owned edge between voxels a and b with the lambda of the mesh section.  Both ends
 *   have wc >= 1: each channel is ca + lambda (cb - ca) in double; exactly one end has: that end's values; neither: (0, 0, 0).  The
 *   level comes from the ray caster's formula.  Three bytes per vertex, always R, G, B, in vertex order.
 * CONTRACT of the device: every result is byte-equal to the host definition, whatever the batch, the order of the listed volumes, the
 * capacities and what ran on the handle before.  Every voxel, pixel and vertex is one thread's: no atomics, no workgroup waits on
 * another.
 * OUT OF SCOPE: textures and UV atlases, colour from a camera that is not registered to the depth, exposure or white-balance
 * compensation between frames, view-dependent weighting of colour samples, vertex normals, de-integration, hashed volumes. */
/* The definitions on the host, no device and no handle needed.  Each takes what its uncoloured sibling takes, plus `colours` (the
 * volume's nx * ny * nz colour words) and its images: image[i] / image_out[i] rows x cols of image_format (three bytes per pixel, one
 * for DVO_CAM_MONO8), rgb three bytes per vertex for vertex_capacity vertices.  Each refuses what its sibling refuses, and returns
 * DVO_ERR_INVALID, nothing written, for a NULL colours, image, image[i], image_out or image_out[i], an unknown image format and a NULL
 * rgb with vertex_capacity > 0. */
int  dvo_colour_integrate_host(const dvo_tsdf_volume *vol, unsigned *voxels, unsigned long long *colours, const dvo_tsdf_params *p,
                                    int count, const void *const *depth, int depth_format, const void *const *image, int image_format,
                                    int rows, int cols, const double *K4, const double *poses12);
int  dvo_colour_raycast_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const unsigned long long *colours, const dvo_raycast_params *p,
                             int count, int depth_format, int rows, int cols, const double *K4, const double *poses12, void *const *depth_out,
                             float *const *normals_out /* may be NULL */, void *const *image_out, int image_format);
int  dvo_colour_mesh_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const unsigned long long *colours, int min_weight, float *xyz,
                          unsigned char *rgb, long long vertex_capacity, int *tri, long long triangle_capacity, long long *n_vertices,
                          long long *n_triangles);
/* The handle gets its colour pool: 8 bytes per voxel of max_voxels_total, allocated and zeroed here.  DVO_ERR_NOMEM with everything as it
 * was when that fails; a second call returns DVO_OK and changes nothing; there is no disable.  From then on dvo_tsdf_set_volume and
 * dvo_tsdf_clear also zero the volume's colour words; dvo_tsdf_set_voxels and dvo_tsdf_integrate never touch them (depth-only frames
 * keep going through dvo_tsdf_integrate).  Every colour call below on a handle without a colour pool returns DVO_ERR_STATE with nothing
 * changed. */
int  dvo_colour_enable(dvo_tsdf_batch *b);
/* dvo_tsdf_integrate with an image per frame: its contract, its refusals, and those of dvo_colour_integrate_host for the images.
 * One upload carries the descriptors, plus both image kinds when staged; with DVO_UPLOAD_DEVICE depth and image are both device
 * pointers, read in place.  DVO_TSDF_INTEGRATE_LAUNCHES launch and one synchronisation. */
int  dvo_colour_integrate(dvo_tsdf_batch *b, const dvo_tsdf_params *p, int count, const int *volumes, const void *const *depth,
                               int depth_format, const void *const *image, int image_format, int rows, int cols, const double *K4,
                               const double *poses12, int flags);
/* the volume's nx * ny * nz colour words out of and into the colour pool; refusals as dvo_tsdf_get_voxels */
int  dvo_colour_get_words(dvo_tsdf_batch *b, int volume, unsigned long long *out);
int  dvo_colour_set_words(dvo_tsdf_batch *b, int volume, const unsigned long long *in);
/* dvo_raycast_views with an image per view (host memory, or device pointers with DVO_UPLOAD_DEVICE, as depth_out): DVO_RAYCAST_LAUNCHES
 * launch and one synchronisation; depth and normals are byte-equal to dvo_raycast_views'. */
int  dvo_colour_raycast_views(dvo_tsdf_batch *b, const dvo_raycast_params *p, int count, const int *volumes, int depth_format, int rows,
                              int cols, const double *K4, const double *poses12, void *const *depth_out,
                              float *const *normals_out /* may be NULL */, void *const *image_out, int image_format, int flags);
/* dvo_mesh_extract with three bytes R, G, B per vertex (host memory, or a device pointer with DVO_UPLOAD_DEVICE, as xyz):
 * DVO_MESH_LAUNCHES launches -- the vertices kernel also writes the colours -- and one synchronisation. */
int  dvo_colour_mesh_extract(dvo_tsdf_batch *b, int volume, int min_weight, float *xyz, unsigned char *rgb, long long vertex_capacity, int *tri,
                             long long triangle_capacity, long long *n_vertices, long long *n_triangles, int flags);

/* ---- distance fields: the Euclidean signed distance from every voxel of a fused volume to the nearest obstacle ----------------------
 * What a planner asks of a map: collision checks, trajectory optimisation (cost and gradient per way-point), inflated cost maps.  A
 * TSDF stops at trunc and measures along the viewing ray; the ESDF of this section covers the whole volume and is Euclidean.  It is
 * opt-in like colour: a handle on which dvo_esdf_enable was never called does what it did, with the same bytes, launches and
 * synchronisations.
 * Conventions.  Volumes, words and min_weight as in the fusion section.  One ESDF word of 32 bits per voxel, at the voxel's index, in a
 * second pool laid out exactly like the voxel pool.
 * Definition (rgbd_odometry_amd/csrc/dvo_esdf.h; integers, plus IEEE double in the order written for metres and queries, nothing fused,
 * no transcendental function, sqrt and division in double, both correctly rounded).  Per voxel a with q, w from its TSDF word:
 *   observed(a) = w >= min_weight; inside(a) = observed(a) and q < 0 (the sign test of a crossing);
 *   a is a surface site when it is observed and one of its up to six axis neighbours b inside the volume is observed with
 *   (qa < 0) != (qb < 0): both sides of a crossing are sites.  With sites = DVO_ESDF_SITES_SURFACE_AND_UNKNOWN every voxel that is not
 *   observed is a site too: unknown space is an obstacle;
 *   d2(a) = the minimum over all sites s of (ax - sx)^2 + (ay - sy)^2 + (az - sz)^2 on the lattice: an integer of at most
 *   3 * 1023^2 = 3 139 587, DVO_ESDF_NO_SITE in a volume without a site;
 *   the word: bits 0..23 d2, bit 30 (DVO_ESDF_INSIDE) inside, bit 31 (DVO_ESDF_UNKNOWN) !observed, every other bit 0.
 *   Metres of a word: (float)(voxel_size * sqrt((double)d2)), negated when inside; d2 == DVO_ESDF_NO_SITE gives +INFINITY, -INFINITY
 *   when inside.  It is the distance to the CENTRE of the nearest site voxel: every surface site lies within one voxel_size of the
 *   surface, so within trunc of the surface the TSDF itself is the better value.
 *   Point query, world point P: per axis g = (P - origin) / voxel_size, i = floor(g), f = g - i; DVO_ESDF_OUTSIDE unless 0 <= i and
 *   i + 1 <= n - 1 on all three axes (compared in double: a NaN falls out); the eight corners are read as signed doubles
 *   +-voxel_size * sqrt((double)d2); `unknown` counts the corners with bit 31; DVO_ESDF_NO_DISTANCE when a corner has no distance;
 *   otherwise the distance is their trilinear interpolation along x, then y, then z, each step a + f (b - a), and the gradient is the
 *   analytic derivative of that same form divided by voxel_size (the header writes out the order of every operation).
 * CONTRACT of the device: the words, the metres and the query records are byte-equal to the host definition, whatever the batch: all
 * volumes in one update, one update per volume and any order of the list give the same bytes, and the words of a volume that is not
 * listed are untouched.  No atomics, no workgroup waits on another.
 * Staleness.  The handle keeps one "field is current" flag per volume: set by a successful dvo_esdf_update that lists it, cleared by
 * dvo_tsdf_set_volume, dvo_tsdf_clear, dvo_tsdf_set_voxels, dvo_tsdf_integrate and dvo_colour_integrate on it.  Every reader below
 * returns DVO_ERR_STATE for a volume whose field is not current and on a handle that was never enabled.
 * OUT OF SCOPE: incremental updates after a single frame, a clamp on the distance, sub-voxel refinement of the distance by the site's
 * own TSDF value, 2-D cost-map projection, hashed volumes. */
#ifndef DVO_ESDF_TYPES_DEFINED_
#define DVO_ESDF_TYPES_DEFINED_
#define DVO_ESDF_SITES_SURFACE 0                 /* sites: the voxels on either side of a sign change between observed neighbours */
#define DVO_ESDF_SITES_SURFACE_AND_UNKNOWN 1     /* and every voxel that is not observed */
#define DVO_ESDF_NO_SITE 0xFFFFFFu               /* d2 of every voxel of a volume without a site */
#define DVO_ESDF_INSIDE 0x40000000u              /* bit 30 of an ESDF word: observed with q < 0 */
#define DVO_ESDF_UNKNOWN 0x80000000u             /* bit 31: not observed (w < min_weight) */
#define DVO_ESDF_FOUND 0                         /* dvo_esdf_sample.status: distance and gradient are set */
#define DVO_ESDF_OUTSIDE 1                       /* the point's cell is not inside the lattice (or the point is not finite) */
#define DVO_ESDF_NO_DISTANCE 2                   /* a corner of the cell has d2 == DVO_ESDF_NO_SITE */
typedef struct dvo_esdf_params {
    int min_weight;                      /* a voxel is observed with this many observations: >= 1 */
    int sites;                           /* DVO_ESDF_SITES_SURFACE or DVO_ESDF_SITES_SURFACE_AND_UNKNOWN */
} dvo_esdf_params;
typedef struct dvo_esdf_sample {
    int    status;                       /* DVO_ESDF_FOUND, DVO_ESDF_OUTSIDE or DVO_ESDF_NO_DISTANCE */
    int    unknown;                      /* corners of the cell that are not observed (bit 31): 0 when OUTSIDE */
    double distance;                     /* metres, negative inside; 0 unless FOUND */
    double gradient[3];                  /* d distance / d P, world axes; 0 unless FOUND */
} dvo_esdf_sample;
#endif
#define DVO_ESDF_UPDATE_LAUNCHES 3       /* per dvo_esdf_update: pass x with the classification, pass y, pass z; whatever the list */
/* min_weight 1, sites DVO_ESDF_SITES_SURFACE */
int  dvo_esdf_params_default(dvo_esdf_params *p);
/* The definition on the host, no device and no handle needed: the nx * ny * nz ESDF words of one volume from its TSDF words.
 * DVO_ERR_INVALID, nothing written: a NULL argument, what dvo_tsdf_integrate_host refuses in a volume, min_weight < 1, an unknown
 * sites.  DVO_ERR_NOMEM: no memory for the 4 bytes per voxel the call works in. */
int  dvo_esdf_host(const dvo_tsdf_volume *vol, const unsigned *voxels, const dvo_esdf_params *p, unsigned *words_out);
/* metres of every word of a volume (out: nx * ny * nz floats).  DVO_ERR_INVALID, nothing written: a NULL argument, a bad volume */
int  dvo_esdf_distances_host(const dvo_tsdf_volume *vol, const unsigned *words, float *out);
/* the point query of `count` points (xyz: 3 doubles each) against the ESDF words of a volume.  DVO_ERR_INVALID, nothing written: a NULL
 * argument, a bad volume, count < 1, a point that is not finite */
int  dvo_esdf_query_host(const dvo_tsdf_volume *vol, const unsigned *words, int count, const double *xyz, dvo_esdf_sample *records);
/* The handle gets its distance-field pool: 4 bytes per voxel of max_voxels_total, allocated here and never freed before the handle.
 * DVO_ERR_NOMEM with everything as it was when that fails; a second call returns DVO_OK and changes nothing; there is no disable. */
int  dvo_esdf_enable(dvo_tsdf_batch *b);
/* Recompute the fields of the listed volumes from their words: one upload of the volume records, DVO_ESDF_UPDATE_LAUNCHES launches
 * whatever count and the sizes are, and one synchronisation.  The passes ping-pong between the pool and a scratch block of 4 bytes per
 * listed voxel, allocated by the first call that needs it and again by a call that lists more voxels, before anything is enqueued.
 * Each output scans its column outwards and stops at the exact radius, so the cost follows the distances present; a volume whose
 * voxels are observed but which has no site at all is the worst case, a full column per voxel.  Refused, nothing changed:
 * DVO_ERR_INVALID bad parameters, count outside [1, max_volumes], a NULL list, a volume outside range or listed twice; DVO_ERR_STATE a
 * handle that was never enabled, a listed volume that was never set. */
int  dvo_esdf_update(dvo_tsdf_batch *b, const dvo_esdf_params *p, int count, const int *volumes);
/* the volume's nx * ny * nz ESDF words; DVO_ERR_INVALID a NULL buffer or a volume outside range */
int  dvo_esdf_get_words(dvo_tsdf_batch *b, int volume, unsigned *out);
/* metres of the nz z-planes from iz0 (out: nx * ny * nz floats, in index order): converted on the device in ONE launch, one
 * synchronisation, so that a planner that needs one storey does not pay for the whole volume.  flags 0: out is host memory, filled by
 * one copy back; DVO_UPLOAD_DEVICE: a device pointer of the handle's GPU, written in place.  Refused, nothing written: DVO_ERR_INVALID
 * a NULL buffer, an unknown flag, a volume outside range, iz0 < 0, nz < 1, iz0 + nz above the volume's nz. */
int  dvo_esdf_get_distances(dvo_tsdf_batch *b, int volume, int iz0, int nz, float *out, int flags);
/* the batched point query: ONE launch and one synchronisation.  flags 0: xyz and out are host memory (one upload, one copy back);
 * DVO_UPLOAD_DEVICE: both are device pointers of the handle's GPU.  Refused, nothing written: DVO_ERR_INVALID count < 1, a NULL
 * argument, an unknown flag, a volume outside range and, in host memory, a point that is not finite (in device memory such a point is
 * not seen by the host: its record is DVO_ESDF_OUTSIDE). */
int  dvo_esdf_query(dvo_tsdf_batch *b, int volume, int count, const double *xyz, dvo_esdf_sample *out, int flags);

/* ---- frame-to-model alignment: projective point-to-plane ICP of depth frames against ray-cast model views ---------------------------
 * The estimator a TSDF pipeline pairs with its ray caster: a new depth frame is aligned to the model's predicted depth and normals --
 * what dvo_raycast_views writes, in HBM with DVO_UPLOAD_DEVICE.  It works from depth alone (in the dark, on textureless walls), refines
 * a loop-closure pose geometrically after dvo_tracker_verify, closes the loop render -> align -> fuse on the device, and returns the
 * 6 x 6 information matrix of the alignment for a pose-graph edge.  A dvo_icp_batch is a stand-alone handle: no dvo_ctx, no tracker,
 * no dvo_tsdf_batch.
 * A view is a now-depth image and a model depth image, both rows x cols (each DVO_DEPTH_U16 millimetres or DVO_DEPTH_F32 metres, the
 * hole rules of the fusion section), the model's normals (three floats per pixel, world axes, (0, 0, 0) = none), one K4 = fx, fy, cx,
 * cy for both images, the model view's pose Tm = {Rm, tm} and a start pose T = {R, t} of the now frame; poses are 12 doubles, R
 * column-major then t, camera to world.  A call aligns `count` views independently.
 * Definition (rgbd_odometry_amd/csrc/dvo_icp.h; IEEE double in the order written, nothing fused, no transcendental function; division
 * and sqrt in double, both correctly rounded).  Pixel term at the estimate (R, t), now pixel (u, v); a skipped pixel contributes +0.0
 * to every sum and 0 to the count:
 *   D = metres of now[v][u]; skip a hole, D <= z_near and D > z_far; pc = (((double)u - cx) / fx D, ((double)v - cy) / fy D, D);
 *   p = R pc + t; q = Rm^T (p - tm); skip unless q.z > z_near; um = floor((fx (q.x / q.z) + cx) + 0.5), vm alike; skip out of bounds
 *   (compared in double: a NaN falls out); Dm = metres of model[vm][um], skip a hole; n = the normal there as doubles, skip (0, 0, 0);
 *   m = Rm backproject(um, vm, Dm) + tm; d = p - m; skip if d.d > dist_max dist_max; r = n.d; wgt = 1 when huber <= 0 or |r| <= huber,
 *   else huber / |r|; J = (n, p x n), tangent order (v, w) of the world-frame left increment p <- p + v + w x p; the sums: the 21 upper
 *   entries of sum (wgt J_i) J_j, the 6 of sum (wgt J_i) r, sum r r (unweighted) and the count.  Every product of a matrix and a
 *   vector and every dot product is ((a0 b0 + a1 b1) + a2 b2).
 * Sum order (part of the definition).  The pixels a sweep visits form a list in raster order.  tree64(x[0 .. 64)): for s = 32, 16, 8,
 *   4, 2, 1: for l < s: x[l] = x[l] + x[l + s]; the result is x[0].  The sum of a list: pad it with +0.0 to a multiple of 64, replace
 *   each run of 64 consecutive entries by its tree64, and repeat on the list of results until one value is left (at least one round).
 * Levels.  Level l visits the now pixels with u % 2^l == 0 and v % 2^l == 0 in the raster order of that sub-grid; the model images are
 *   always read at full resolution, no pyramid is built.  Levels run from levels - 1 down to 0 with iterations[l] sweeps at level l.
 * After each sweep, per view: count < min_count stops the view with DVO_ICP_FEW; else A = L D L^T without a square root, in the order
 *   the header writes out, and a pivot that fails D_k > min_pivot_ratio A_kk stops it with DVO_ICP_DEGENERATE (a single plane ends
 *   here); else A x = -b, x = (v, w), and the Cayley update a = w / 2, C = I + (2 / (1 + a.a)) ([a]x + [a]x^2), R <- C R, t <- C t + v;
 *   x.x < stop_norm stop_norm skips the rest of this level's sweeps for this view.  A stopped view keeps the pose it had.
 * After level 0 one more level-0 sweep runs with no update, unless the view stopped with FEW or DEGENERATE (then the record comes from
 *   the sweep that stopped it): the record describes the returned pose.
 * info is in the tangent order (v, w) of a world-frame LEFT increment T <- exp(x) T; dvo_graph_information and the pose graph's edges
 *   take the order [translation, rotation] of a RIGHT (body-frame) increment: INTEGRATION.md 3g has the 6 x 6 adjoint between them.
 * CONTRACT of the device: poses and records are byte-equal to dvo_icp_align_host whatever the batch: all views in one call, one call
 * per view and any order of the list give the same bytes.  No atomics, no workgroup waits on another; the images are only read.
 * The front end of a sensor's depth frame -- bilateral filter, now-frame normals -- and the normal gate that uses them are the
 * sub-section "preparing a depth frame" below.
 * OUT OF SCOPE: a depth pyramid, separate intrinsics for the model and the now frame, damping, colour terms. */
#ifndef DVO_ICP_TYPES_DEFINED_
#define DVO_ICP_TYPES_DEFINED_
#define DVO_ICP_MAX_LEVELS 4
#define DVO_ICP_MAX_ITERATIONS 64        /* sweeps of one level */
#define DVO_ICP_MAX_PIXELS 16777216      /* rows * cols of a call: 2^24 */
#define DVO_ICP_OK 0                     /* dvo_icp_record.status: every sweep ran (or was skipped after stop_norm) */
#define DVO_ICP_FEW 1                    /* a sweep found fewer than min_count pixels: the view stopped there */
#define DVO_ICP_DEGENERATE 2             /* a pivot of the normal matrix failed min_pivot_ratio: the view stopped there */
typedef struct dvo_icp_params {
    int    levels;                       /* [1, DVO_ICP_MAX_LEVELS] */
    int    iterations[DVO_ICP_MAX_LEVELS];   /* sweeps at level l, each in [0, DVO_ICP_MAX_ITERATIONS]; those of levels >= `levels` play no part */
    double z_near, z_far;                /* metres: a now depth <= z_near or > z_far, a point at model-camera depth <= z_near are skipped */
    double dist_max;                     /* metres: a pair further apart is skipped; > 0 */
    double huber;                        /* metres: residuals beyond it are down-weighted; 0 = off */
    double stop_norm;                    /* an update shorter than this ends its level; 0 = never */
    double min_pivot_ratio;              /* (0, 1) */
    int    min_count;                    /* >= 1 */
} dvo_icp_params;
typedef struct dvo_icp_record {
    int    status;                       /* DVO_ICP_OK, DVO_ICP_FEW, DVO_ICP_DEGENERATE */
    int    iterations;                   /* updates applied */
    int    count;                        /* pixels of the record's sweep */
    int    reserved;                     /* 0 */
    double sum_r2, rms;                  /* of the record's sweep: sum r r (unweighted), sqrt(sum_r2 / count) */
    double info[36];                     /* sum (wgt J_i) J_j, row-major, tangent order (v, w) */
} dvo_icp_record;
#endif
#define DVO_ICP_LAUNCHES_PER_SWEEP 2     /* the sweep kernel and the solve kernel; a constant of the build whatever count is */
typedef struct dvo_icp_batch dvo_icp_batch;
/* levels 3, iterations {10, 5, 4, 0}, z_near 0.1, z_far 8.0, dist_max 0.1, huber 0 (off), stop_norm 0 (never), min_pivot_ratio 1e-9,
 * min_count 6 */
int  dvo_icp_params_default(dvo_icp_params *p);
/* The definition on the host, no device and no handle needed.  Per view i: now_depth[i] and model_depth[i] rows x cols of their
 * formats, model_normals[i] 3 rows x cols floats, K4 + 4 i, model_poses12 + 12 i, start_poses12 + 12 i; out: poses12_out + 12 i and
 * records[i].  DVO_ERR_INVALID, nothing written: a NULL argument (an image of a list included); a parameter that is not finite,
 * levels outside [1, DVO_ICP_MAX_LEVELS], an iterations[l] outside [0, DVO_ICP_MAX_ITERATIONS], anything other than 0 < z_near < z_far,
 * dist_max <= 0, a negative huber or stop_norm, min_pivot_ratio outside (0, 1), min_count < 1; count, rows or cols < 1;
 * rows * cols > DVO_ICP_MAX_PIXELS; an unknown format; a K4 or pose as dvo_tsdf_integrate_host refuses them. */
int  dvo_icp_align_host(const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                        const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                        const double *model_poses12, const double *start_poses12, double *poses12_out, dvo_icp_record *records);
/* A handle for calls of up to max_views views.  DVO_ERR_NO_DEVICE without a HIP device (no CPU fallback), DVO_ERR_INVALID for
 * max_views < 1.  The blocks a call stages its views and images in, sums its partials in and brings its results back in are allocated
 * by the first call that needs them and again by a call that needs larger ones, before anything is enqueued. */
int  dvo_icp_create(int max_views, dvo_icp_batch **out);
int  dvo_icp_destroy(dvo_icp_batch *b);
const char *dvo_icp_last_error(const dvo_icp_batch *b);                   /* b may be NULL: last creation error */
/* dvo_icp_align_host on the device (p NULL: the defaults).  flags 0: the images are host memory and are staged by the call;
 * DVO_UPLOAD_DEVICE: they are device pointers of the handle's GPU, read in place -- what dvo_raycast_views(..., DVO_UPLOAD_DEVICE) has
 * just written and what the tracker's device upload holds.  Either way: one upload (the views and their start poses, and the images
 * when staged), DVO_ICP_LAUNCHES_PER_SWEEP launches for each of the sum of iterations[0 .. levels) + 1 sweeps, one copy back of poses
 * and records, ONE synchronisation: the host looks at nothing between sweeps, and views that have stopped or converged are skipped on
 * the device through a per-view state word.  Refused, nothing written: DVO_ERR_INVALID as dvo_icp_align_host, and for count above
 * max_views or an unknown flag. */
int  dvo_icp_align(dvo_icp_batch *b, const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols,
                   const double *K4, const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                   const double *model_poses12, const double *start_poses12, double *poses12_out, dvo_icp_record *records, int flags);
/* what the last dvo_icp_align, dvo_icp_align_gated or dvo_icp_prepare issued (either pointer may be NULL): kernel launches and host
 * synchronisations */
int  dvo_icp_stats(dvo_icp_batch *b, int *last_launches, int *last_syncs);

/* ---- preparing a depth frame: bilateral filter, now-frame normals, normal gate (KinectFusion's front end) -----------------------------
 * A sensor's depth is quantised and noisy; normals taken from it raw are useless, and without normals of the now frame projective
 * association cannot reject a pixel on one wall that lands on a pixel of the adjoining wall.  dvo_icp_prepare filters a depth image
 * into float metres and takes its normals; dvo_icp_align_gated is dvo_icp_align with a test of those normals against the model's.
 * Definition (rgbd_odometry_amd/csrc/dvo_icp_prepare.h and the gate in dvo_icp.h; the rules of the section above).  The weights of the
 * filter are DATA, two tables in dvo_icp_prepare_params: host and device agree in bytes given the tables, whatever anyone's exp().
 * Filter: the input is rows x cols, DVO_DEPTH_U16 or DVO_DEPTH_F32 under the hole rules of the fusion section; the output is float
 *   metres, 0.0f = a hole.  Per pixel: Dc = metres of the centre, a hole stays a hole; num = 0.0, den = 0u (32 unsigned bits); taps dy
 *   from -radius to radius and inside that dx from -radius to radius, the centre an ordinary tap; a tap outside the image or on a hole is
 *   skipped; D = its metres, k = fabs(D - Dc) * range_scale, skipped unless k < 256.0; w = (unsigned)spatial[(dy + radius) * (2 radius +
 *   1) + (dx + radius)] * (unsigned)range[(int)k]; num = num + (double)w * D; den = den + w; the output is (float)(num / (double)den).
 * Normals: from the filtered image F, in the axes of the NOW CAMERA, three floats per pixel, (0, 0, 0) = none.  None unless 1 <= u <=
 *   cols - 2, 1 <= v <= rows - 2, F is no hole at the pixel and its four neighbours and every neighbour has fabs(D_nb - D_c) <=
 *   edge_max; else V(u, v) = (((double)u - cx) / fx * D, ((double)v - cy) / fy * D, D), a = V(u + 1, v) - V(u - 1, v), b = V(u, v + 1) -
 *   V(u, v - 1), G = b x a, gg = (G0 G0 + G1 G1) + G2 G2, none unless gg > 0, n_k = (float)(G_k / sqrt(gg)).  On a fronto-parallel plane
 *   G points along -z: to the viewer's side, as the ray caster's normals do.
 * Gate, in the pixel term of the alignment after the model normal n is read, only when the call has now normals: nn = the now normal at
 *   the now pixel as doubles, skip (0, 0, 0); nw_k = (R[k] nn0 + R[3 + k] nn1) + R[6 + k] nn2; c = (n0 nw0 + n1 nw1) + n2 nw2; skip
 *   unless c >= normal_cos_min (a NaN falls out).  Unit length of either normal is the caller's business. */
#ifndef DVO_ICP_PREPARE_TYPES_DEFINED_
#define DVO_ICP_PREPARE_TYPES_DEFINED_
#define DVO_ICP_PREPARE_MAX_RADIUS 6
#define DVO_ICP_PREPARE_RANGE_BINS 256
typedef struct dvo_icp_prepare_params {
    int            radius;              /* [0, 6]: the window is (2 radius + 1)^2 */
    int            reserved;            /* 0 */
    double         range_scale;         /* bins per metre of depth difference: finite, > 0 */
    double         edge_max;            /* metres, finite, > 0: no normal across a larger depth step */
    unsigned short range[256];          /* range weight of bin k; range[0] >= 1 */
    unsigned char  spatial[13 * 13];    /* weight of tap (dy, dx) at (dy + radius) * (2 radius + 1) + (dx + radius);
                                           the centre's >= 1; entries past (2 radius + 1)^2 play no part */
} dvo_icp_prepare_params;
#endif
#define DVO_ICP_PREPARE_LAUNCHES 2       /* the filter kernel and the normals kernel, whatever count is; 1 without normals_out */
/* The tables of a Gaussian pair, a host-only convenience: spatial = rint(255 exp(-(dx^2 + dy^2) / (2 sigma_s_px^2))), range_scale =
 * 256 / (3 sigma_r_m) -- the table ends at three sigmas --, range[k] = rint(65535 exp(-((k + 0.5) / range_scale)^2 / (2 sigma_r_m^2))).
 * DVO_ERR_INVALID, nothing written: fp NULL, a radius outside [0, DVO_ICP_PREPARE_MAX_RADIUS], a sigma or edge_max that is not finite
 * or not positive.  The default is gaussian(3, 2.0, 0.03, 0.05): a 7 x 7 window, 2 pixels, 30 mm, no normal across a 50 mm step -- a
 * design choice for a metre-range sensor with millimetre noise, not a property of the engine. */
int  dvo_icp_prepare_params_default(dvo_icp_prepare_params *fp);
int  dvo_icp_prepare_params_gaussian(int radius, double sigma_s_px, double sigma_r_m, double edge_max, dvo_icp_prepare_params *fp);
/* The definition on the host.  Per image i: depth[i] rows x cols of depth_format, K4 + 4 i; out: depth_out[i] rows x cols floats and,
 * unless the list normals_out is NULL, normals_out[i] 3 rows x cols floats.  DVO_ERR_INVALID, nothing written: a NULL argument or list
 * entry (a normals_out[i] of a non-NULL list included); a radius out of range, reserved != 0, range_scale or edge_max not finite or
 * not positive, range[0] or the centre's spatial weight 0; count, rows or cols < 1; rows * cols > DVO_ICP_MAX_PIXELS; an unknown format;
 * a K4 as dvo_tsdf_integrate_host refuses it.  An output must not overlap an input. */
int  dvo_icp_prepare_host(const dvo_icp_prepare_params *fp, int count, int depth_format, int rows, int cols, const double *K4,
                          const void *const *depth, float *const *depth_out, float *const *normals_out /* may be NULL */);
/* dvo_icp_prepare_host on the device (fp NULL: the default): byte-equal to it whatever the batch.  DVO_ICP_PREPARE_LAUNCHES launches
 * per call whatever count is -- the filter, then the normals, a kernel boundary between them --, one without normals_out; one upload,
 * ONE synchronisation.  flags 0: host memory, staged by the call, one copy back.  DVO_UPLOAD_DEVICE: device pointers of the handle's
 * GPU, read and written in place, nothing copied back: the tracker's device upload or a ray-cast depth goes in, and the outputs go
 * straight into dvo_icp_align_gated(..., DVO_UPLOAD_DEVICE) and dvo_tsdf_integrate(..., DVO_DEPTH_F32, ..., DVO_UPLOAD_DEVICE).
 * Buffers grow before anything is enqueued; dvo_icp_stats reports the call.  Refused, nothing written: DVO_ERR_INVALID as
 * dvo_icp_prepare_host, for count above max_views, an unknown flag and, with DVO_UPLOAD_DEVICE, a depth_out[i] equal to its depth[i]
 * (the filter reads a halo: it cannot run in place).  A partial overlap of an output with an input is the caller's to avoid. */
int  dvo_icp_prepare(dvo_icp_batch *b, const dvo_icp_prepare_params *fp, int count, int depth_format, int rows, int cols, const double *K4,
                     const void *const *depth, float *const *depth_out, float *const *normals_out /* may be NULL */, int flags);
/* dvo_icp_align_host and dvo_icp_align with the normal gate: their whole contract, and now_normals[i] 3 rows x cols floats in the axes
 * of the now camera (what dvo_icp_prepare writes).  now_normals NULL: the ungated call, the same bytes, normal_cos_min ignored --
 * dvo_icp_align_host and dvo_icp_align are these calls with NULL.  With a list: a NULL entry, or a normal_cos_min that is not finite or
 * outside [-1, 1], is refused.  A staged call copies the now normals with the other images in its one upload; launches and the one
 * synchronisation are those of dvo_icp_align. */
int  dvo_icp_align_gated_host(const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                              const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                              const double *model_poses12, const double *start_poses12, const float *const *now_normals /* may be NULL */,
                              double normal_cos_min, double *poses12_out, dvo_icp_record *records);
int  dvo_icp_align_gated(dvo_icp_batch *b, const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols,
                         const double *K4, const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                         const double *model_poses12, const double *start_poses12, const float *const *now_normals /* may be NULL */,
                         double normal_cos_min, double *poses12_out, dvo_icp_record *records, int flags);

/* ---- the legacy photometric Gauss-Newton odometry: the engine behind RGBDOdometry -----------
 * RGBDOdometry (include/RGBDOdometry.h:41-43, src/RGBDOdometry.cpp) aligns intensities instead of edge distances: per
 * reference frame a semi-dense Jacobian J (pixels with x-gradient >= 5) and A = J^T J per pyramid level (:363-508); per new
 * frame and level up to three iterations of eps_i = I_ref(i) - I_now(warp(i, T)), b = -J^T eps, A psi = b by
 * colPivHouseholderQr, T = T exp(psi)^-1 (:514-700), levels 3 then 2 (:162-163).  All in double, like the reference.
 *
 * The reference code has defects.  `fixed` = 0 (default) REPRODUCES its arithmetic as written, so that a user
 * of the rgbdSubsc node gets that node's numbers; `fixed` = 1 corrects: D1 tJ(0) = fx*fx/Z -> fx*gx/Z (:485); D2 tJ(5)'s
 * second term fx*gy*Y/Z -> fx*gx*Y/Z (:490); D4 level-0 intrinsics at every level -> scaled by 2^-level (:475-476);
 * D7 exponentialMap dropping the translation when |w| < 1e-12 (:727-731).  Kept in both modes: D3 the transposed image
 * convention (X from the row index with cx, fx, :475/:661/:683 -- self-consistent), D5 depth and translation in sensor units
 * (mm), D6 the selection rule gx >= 5, D8 the absolute stop threshold |eps| < 200 (:556).
 * Frames live in the frame store: upload them with dvo_frames_upload_cameras(..., n_levels = 4, first_shift = 0,
 * flags | DVO_UPLOAD_DEPTH_RAW) -- the node's own INTER_NEAREST pyramid of the full-resolution frame (:316-318, :347-350). */
typedef struct dvo_photo_params {
    double fx, fy, cx, cy;        /* cameraMatrix of params.xml, level 0                       RGBDOdometry.cpp:59-62 */
    int    gradient_threshold;    /* const_gradientThreshold = 5                               :32 */
    int    max_jacobian_size;     /* const_maxJacobianSize = 50000.  The reference asserts xc < const_maxJacobianSize before EVERY
                                     scanned pixel (:464), so a level with n selected pixels is refused when n > max_jacobian_size,
                                     and when n == max_jacobian_size unless its last selected pixel is the last pixel scanned,
                                     (rows-1, cols-1) */
    int    min_required_pts;      /* const_minimumRequiredPts = 100 (fewer: error, :500)        :34 */
    int    iterations;            /* 3                                                          :545 */
    double eps_norm_stop;         /* 200.0                                                      :556 */
    int    fixed;                 /* 0 = the reference's arithmetic, 1 = defects D1 D2 D4 D7 corrected */
    int    reserved;
} dvo_photo_params;
int  dvo_photo_params_default(dvo_photo_params *p);
int  dvo_photo_configure(dvo_ctx *ctx, const dvo_photo_params *p);
/* setRefFrame + computeJacobianAllLevels (:296-327, :363-398) for levels first_level .. n_levels-1 of stored frame `slot`
 * (the reference: first_level = 1).  n_selected[n_levels] (may be NULL) receives the rows of J per level, also when the frame is
 * refused.  Every level is counted and checked (max_jacobian_size, min_required_pts) before anything is written: a refused frame
 * changes nothing, and the previous reference stays in force for dvo_photo_align and dvo_photo_get_jacobian.
 * Depth 0 (a hole in a DVO_UPLOAD_DEPTH_RAW frame) at a selected pixel is used as the reference uses it: that row of J holds inf
 * and NaN (1/Z, 0 * inf), so A is not finite, and so is T after the first update on that level.  The point itself projects to
 * 0/0 under T = I (eps 0) and to the image of the translation otherwise.  Fill or mask holes before the upload to avoid this. */
int  dvo_photo_set_ref(dvo_ctx *ctx, int slot, int first_level, int *n_selected);
/* gaussNewtonIterations(level, T) (:514-597) for levels[0], levels[1], ... in that order (the reference: {3, 2}, :162-163) on
 * stored frame `now_slot`.  T16: TransformRep::matrix(), 4x4 row-major, in/out.  eps_norms[n_run * iterations]: |eps| of every
 * iteration (-1 where not run); updates[n_run]: iterations that changed T.  Both may be NULL. */
int  dvo_photo_align(dvo_ctx *ctx, int now_slot, const int *levels, int n_run, double *T16, double *eps_norms, int *updates);
/* inspection: J (n x 6 row-major), selected pixels (row, column) and A = J^T J (6x6) of a reference level */
int  dvo_photo_get_jacobian(dvo_ctx *ctx, int level, double *J, int *sel_i, int *sel_j, int capacity, double *A36, int *n_out);

/* ---- many camera streams on the photometric engine: RGBDOdometry::processFrame for K streams at once ------------------------
 * A dvo_photo_streams handle owns K independent streams, each with its own reference (J, sel, zref, gref, A and n per level), warm-start
 * T and frame counter nFrame.  dvo_photo_streams_step advances any subset of them by one frame, and each listed stream does what
 * dvo_amd::RGBDOdometry::processFrame does (RGBDOdometry.cpp:146-163): when nFrame % ref_every == 0 the frame becomes its reference, T
 * is reset to I and the frame is then aligned to itself (event 1); otherwise the frame is aligned from the last T (event 0).  T, the
 * norms and the update counts are bit-identical to the dvo_photo_set_ref / dvo_photo_align sequence on a one-stream context: the
 * kernels are the single-pair kernels' bodies, with the same 1024-thread workgroups and reductions.  `base` (base = base * T at a
 * reference tick, :146-150) and the published pose are the caller's, as GOP is for the edge tracker: dvo_amd::RGBDOdometryStreams.
 *
 * Layout: one context whose frame store has K slots (stream s uses slot s; the frame store holds the latest frame only: the reference
 * lives in the stream's slabs), and per stream and level l >= first_level a slab of min(max_jacobian_size, rows_l * cols_l) rows of J
 * (6 doubles), zref (double), sel (int), gref (float), plus A (36 doubles) and n, all allocated at creation: about 4.7 MB per stream at
 * 640x480 with levels 1..3.  Creation fails with DVO_ERR_NOMEM when they do not fit.
 *
 * A step, in order: one batched frame upload per run of consecutive listed streams (dvo_frames_upload_cameras: 4 levels, first_shift
 * 0, DVO_UPLOAD_DEPTH_RAW plus the caller's DVO_UPLOAD_DEVICE / _MAPPED / _DIRECT); if any listed stream is on a reference tick: the
 * selection (count + scan, one launch per level and stage for all of them), ONE read of every count and last-pixel flag, the rules of
 * dvo_photo_set_ref per stream (max_jacobian_size, min_required_pts), and the fill (J + A, two launches per level) of the accepted ones;
 * then ONE Gauss-Newton launch (one workgroup per stream, every level of `levels` in order) for every stream that has a reference, and
 * ONE read of T, norms and updates.  An ordinary step is thus the upload launches + 1 launch and 1 host synchronisation at any K; a step
 * with reference ticks adds 4 launches per reference level and one synchronisation (the first step of a handle also allocates the frame
 * store).
 * A stream whose new reference breaks a rule gets event -1 and keeps everything as it was (reference, T, nFrame): the frame has the
 * effect of a frame that never arrived, and a stream without a reference yet retries on its next frame.  The other streams go on. */
typedef struct dvo_photo_streams dvo_photo_streams;
typedef struct dvo_photo_streams_params {
    dvo_photo_params photo;       /* camera matrix, gradient threshold, max_jacobian_size, min_required_pts, iterations, stop, fixed */
    int ref_every;                /* (nFrame % ref_every) == 0 renews the reference (RGBDOdometry.cpp:146): default 10000 */
    int first_level;              /* computeJacobianAllLevels from this level (:373): default 1 */
    int n_run, levels[DVO_MAX_LEVELS];   /* gaussNewtonIterations order (:162-163): default 2, {3, 2}; n_run * iterations <= 64 */
    int rows, cols;               /* camera frame; default 480 x 640.  Pyramid: 4 levels, first_shift 0, DVO_UPLOAD_DEPTH_RAW */
} dvo_photo_streams_params;
int  dvo_photo_streams_params_default(dvo_photo_streams_params *p);
/* Refused with DVO_ERR_INVALID: bad photometric parameters (as dvo_photo_configure), ref_every < 1, first_level outside [0, 4), a level of
 * `levels` below first_level or beyond the pyramid, n_run * iterations > 64, max_streams outside [1, 65535].  DVO_ERR_NO_DEVICE
 * without a HIP device (no CPU fallback), DVO_ERR_NOMEM when the slabs do not fit. */
int  dvo_photo_streams_create(const dvo_photo_streams_params *p, int max_streams, dvo_photo_streams **out);
int  dvo_photo_streams_destroy(dvo_photo_streams *h);
const char *dvo_photo_streams_last_error(const dvo_photo_streams *h);    /* h may be NULL: last creation error */
/* the stream starts over: nFrame = 0, no reference (its next frame is a reference tick); its camera matrix stays and may now be changed */
int  dvo_photo_streams_reset_stream(dvo_photo_streams *h, int stream);
/* The stream's own level-0 camera matrix (fx, fy, cx, cy as dvo_photo_params; `fixed` and the level scaling stay the handle's), in
 * place of p.photo.fx .. cy, for a rig whose cameras differ.  Only while the stream is at its start (never stepped since creation or
 * dvo_photo_streams_reset_stream), else DVO_ERR_STATE and nothing changes: its reference's Jacobians were computed with the old matrix.
 * Refused with DVO_ERR_INVALID, nothing changed: a stream outside [0, max_streams), fx or fy not positive.  Uploaded here, once. */
int  dvo_photo_streams_set_stream_intrinsics(dvo_photo_streams *h, int stream, double fx, double fy, double cx, double cy);
/* Advance streams[0..count) by one frame each: bgr8[i] (rows x cols x 3, row-major) and depth[i] (float, sensor units, row-major) of
 * stream streams[i]; flags: DVO_UPLOAD_DEVICE / DVO_UPLOAD_MAPPED / DVO_UPLOAD_DIRECT as for dvo_frames_upload_cameras (the buffers are
 * borrowed until the call returns).  Outputs per listed stream i: T16_out[16i..] the key-frame relative T (4x4 row-major), eps_norms
 * [(i * n_run + r) * iterations + it] the |eps| of every iteration (-1 where not run; may be NULL), updates[i * n_run + r] (may be
 * NULL), event[i] = 1 reference tick, 0 ordinary, -1 new reference refused (T16_out = the stream's unchanged T, norms -1, updates 0).
 * Refused with DVO_ERR_INVALID, state unchanged: count outside [1, max_streams], a stream outside [0, max_streams) or listed twice,
 * rows / cols other than the handle's, a NULL argument. */
int  dvo_photo_streams_step(dvo_photo_streams *h, int count, const int *streams, const unsigned char *const *bgr8,
                            const float *const *depth, int rows, int cols, int flags, double *T16_out, double *eps_norms, int *updates,
                            int *event);
/* dvo_photo_streams_step with the frames in sensor formats (dvo_frames_upload_cameras_fmt); DVO_UPLOAD_DEPTH_RAW stays forced, so a
 * DVO_DEPTH_U16 value v is the sensor value (float)v, holes stay 0 -- the mono16 image RGBDOdometry.cpp:231 receives.
 * dvo_photo_streams_step is this call with (DVO_CAM_BGR8, DVO_DEPTH_F32).  Also refused with DVO_ERR_INVALID: an unknown format. */
int  dvo_photo_streams_step_fmt(dvo_photo_streams *h, int count, const int *streams, const void *const *image, int image_format,
                                const void *const *depth, int depth_format, int rows, int cols, int flags, double *T16_out,
                                double *eps_norms, int *updates, int *event);
/* as dvo_photo_get_jacobian, for the current reference of `stream` (DVO_ERR_STATE if it has none) */
int  dvo_photo_streams_get_jacobian(dvo_photo_streams *h, int stream, int level, double *J, int *sel_i, int *sel_j, int capacity,
                                    double *A36, int *n_out);
/* What the last step issued (any pointer may be NULL): kernel launches and host synchronisations (counted as for dvo_tracker_get_stats),
 * frame-upload calls (one per run of consecutive listed streams), streams that took a new reference, streams whose reference was refused. */
int  dvo_photo_streams_get_stats(dvo_photo_streams *h, int *kernel_launches, int *host_syncs, int *runs, int *ref_events, int *refused);
/* the underlying context (frame store: slot = stream) */
dvo_ctx *dvo_photo_streams_context(dvo_photo_streams *h);

#ifdef __cplusplus
}
#endif
#endif /* DVO_AMD_H_ */
