/*
 * dvo_oracle.h -- CPU ORACLE for the SolveDVO edge-alignment hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, the smoke()
 * entry point and bench.py's cpu_baseline leg may load it.  The shipped engine
 * (rgbd_odometry_amd/csrc) never includes, links or calls anything in here.
 *
 * PARITY UNPINNED: the reference (mpkuse/rgbd_odometry) ships no tests, golden
 * vectors or fixtures for this path and cannot be compiled in this image (it
 * needs ROS, OpenCV 2.4, Eigen3, Sophus and libigl, none of which are present),
 * so this restatement is pinned only by (a) the algebraic properties the cited
 * lines imply and (b) its own committed golden vectors (tests/golden).
 *
 * What it restates (all paths relative to /root/reference):
 *   src/SolveDVO.cpp:224-264    enlistRefEdgePts      -> dvo_oracle_enlist_ref_points
 *   src/SolveDVO.cpp:1230-1264  selectedPts           -> (same function, mask rule)
 *   src/SolveDVO.cpp:306-414    computeJacobianOfNowFrame
 *   src/SolveDVO.cpp:425-462    getReprojectedEpsilons -> dvo_oracle_eval_points
 *   src/SolveDVO.cpp:1047-1053  getWeightOf           -> dvo_oracle_weight
 *   src/SolveDVO.cpp:1285-1308  interpolate           -> (flag interpolate_dt)
 *   src/SolveDVO.cpp:1310-1312  aggregateEpsilons
 *   src/SolveDVO.cpp:619-1017   runIterations         -> dvo_oracle_run_iterations
 *   src/SolveDVO.cpp:1269-1282  rotationize           -> dvo_oracle_rotationize
 *   src/SolveDVO.cpp:2097-2104  level schedule        -> dvo_oracle_align_pyramid
 *   src/SolveDVO.cpp:1768-1795, :1063-1098  DT / normalise / gradients of the now frame (after Canny)
 *                                                     -> dvo_oracle_now_level_from_edges
 * Third-party arithmetic on the path that is NOT in /root/reference and is
 * restated from its published algorithm (versions unpinned by the reference's
 * package.xml / CMakeLists.txt):
 *   Sophus (templated SE3Group/SO3Group, 2012-2015): SE3d::exp, SE3d::log,
 *     setRotationMatrix, rotationMatrix  (call sites SolveDVO.cpp:736-739,905-907)
 *   Eigen 3: JacobiSVD<Matrix3d,NoQRPreconditioner> (two-sided Jacobi),
 *     Quaternion(Matrix3) and Quaternion::toRotationMatrix
 *   libigl: igl::repmat (trivial)
 *
 * Layout conventions (Eigen defaults): images are COLUMN-major H x W floats,
 * element (yy,xx) at data[yy + xx*rows]; point lists are 3xN column-major
 * (xyz interleaved); R is 3x3 column-major double, R(i,j) = R[i+3*j].
 */
#ifndef DVO_ORACLE_H_
#define DVO_ORACLE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every literal of runIterations, with the reference value as default. */
typedef struct dvo_oracle_params {
    double beta;                /* heavy-ball BETA = 0.5                    SolveDVO.cpp:653 */
    double precond_rot;         /* PFactor = .5 -> P=diag(1,1,1,.5,.5,.5)   :724-730 */
    double reg_lambda;          /* regularizationLambda = 0.05              :742 */
    double step_a;              /* 9.0      (stepLength = 9.0*1.0E-2/...)   :773 */
    double step_b;              /* 1.0E-2                                   :773 */
    int    step_decay_after;    /* 5  : (itr>5)?(itr-4):1                   :773 */
    int    step_decay_offset;   /* 4                                        :773 */
    float  trust_radius;        /* trustRegionHyperSphereRadius = 0.003     :25  (float member) */
    float  psi_norm_stop;       /* psiNormTerminationThreshold = 1.0E-7     :24  (float member) */
    int    enable_rotationize;  /* __ENABLE_ROTATIONIZE__      SolveDVO.h:107 */
    int    enable_l2_reg;       /* __ENABLE_L2_REGULARIZATION  SolveDVO.h:112 */
    int    interpolate_dt;      /* __INTERPOLATE_DISTANCE_TRANSFORM, off  SolveDVO.h:97 */
} dvo_oracle_params;

void dvo_oracle_params_default(dvo_oracle_params *p);

/* Per-iteration trace record (for golden vectors and step-by-step parity). */
typedef struct dvo_oracle_iter_trace {
    double g[6];        /* J^T W eps before the regulariser (:777) */
    double H[21];       /* upper triangle of sum_i w_i J_i J_i^T (not used by the reference policy) */
    double sum_eps2;    /* sum eps_i^2 in double */
    double psi[6];      /* step actually applied (after clamp); zeros if the loop broke */
    double R[9];        /* pose AFTER the update (col-major) */
    double t[3];
    float  energy;
    int    n_visible;
    int    broke;       /* 1 if early termination happened in this iteration */
} dvo_oracle_iter_trace;

/* SolveDVO.cpp:1230-1264 + :224-264.  edge (int32) and depth_mm (f32) are
 * column-major rows x cols.  Returns N (number of selected points) or -1 if
 * capacity is too small.  xyz: 3xN, uv: 2xN (may be NULL). */
int dvo_oracle_enlist_ref_points(int level, const int *edge, const float *depth_mm,
                                 int rows, int cols,
                                 float fx, float fy, float cx, float cy,
                                 float *xyz, float *uv, int capacity);

/* One evaluation of :306-414 + :425-462 at a float pose.
 * Rf: 3x3 col-major float, tf: 3 float.  Outputs (any may be NULL):
 * reproj 3xN col-major; J Nx6 ROW-major (J[6*i+k]); eps[N]; w[N]; visible[N] (0/1). */
void dvo_oracle_eval_points(const dvo_oracle_params *prm, int level,
                            const float *xyz, int N,
                            const float *dt, const float *gx, const float *gy,
                            int rows, int cols,
                            float fx, float fy, float cx, float cy,
                            const float *Rf, const float *tf,
                            float *reproj, float *J, float *eps, float *w, int *visible);

/* :619-1017.  R,t in/out.  energy[max_iters] zero-filled first.
 * final_eps[N], final_reproj[3N] may be NULL.  trace[max_iters] may be NULL.
 * Returns the number of iterations whose energy was evaluated. */
int dvo_oracle_run_iterations(const dvo_oracle_params *prm, int level, int max_iters,
                              const float *xyz, int N,
                              const float *dt, const float *gx, const float *gy,
                              int rows, int cols,
                              float fx, float fy, float cx, float cy,
                              double *R, double *t,
                              float *energy, float *final_eps, float *final_reproj,
                              int *best_idx, float *visible_ratio,
                              dvo_oracle_iter_trace *trace);

/* The 29 sums of one evaluation over points [first, first+n): acc[0..20] = upper triangle of
 * sum w J J^T, acc[21..26] = g, acc[27] = sum eps^2, acc[28] = n_visible. */
void dvo_oracle_accumulate(const dvo_oracle_params *prm, int level, const float *xyz, int first, int n,
                           const float *dt, const float *gx, const float *gy, int rows, int cols,
                           float fx, float fy, float cx, float cy,
                           const float *Rf, const float *tf, double *acc29);

/* acc32[0..28] as above; acc32[29..31] = the three limbs of the range's EXACT sum of eps^2 (integers below 2^53 held in doubles, unit
 * 2^-68: limbs of several ranges add exactly in any order).  dvo_oracle_e2_from_limbs turns (summed) limbs into the correctly rounded
 * double of the exact sum -- what acc[27] holds for one range; `fallback` is returned when a term was outside [2^-11, 2^12). */
void dvo_oracle_accumulate32(const dvo_oracle_params *prm, int level, const float *xyz, int first, int n,
                             const float *dt, const float *gx, const float *gy, int rows, int cols,
                             float fx, float fy, float cx, float cy,
                             const float *Rf, const float *tf, double *acc32);
void dvo_oracle_e2_limbs(const float *eps, int n, double *limbs3);
double dvo_oracle_e2_from_limbs(const double *limbs3, double fallback);

/* runIterations as an explicit state machine (what run_iterations itself uses), so that a
 * host-driven loop -- e.g. the multi-GPU tiled mode with an all-reduce between the per-point
 * phase and the update -- can be checked step by step. */
typedef struct dvo_oracle_state {
    double R[9], t[3], d[6], bestR[9], bestT[3];
    float bestE, bestRatio;
    int bestItr, stop;
} dvo_oracle_state;
void dvo_oracle_state_begin(dvo_oracle_state *s, const double *R, const double *t);
int  dvo_oracle_state_update(const dvo_oracle_params *prm, dvo_oracle_state *s, int itr, int N,
                             const double *g6, double sum_eps2, int n_vis, float *energy_out,
                             double *psi_out /* may be NULL */);
void dvo_oracle_state_finish(const dvo_oracle_params *prm, dvo_oracle_state *s, double *R, double *t);

/* :2097-2104: for f = n_levels-1 .. 0: if iters[f] > 0: runIterations(f, ...).
 * Per-level inputs are arrays of pointers / sizes indexed by level.
 * energy_out: concatenated per level in LEVEL order (level 0 first), each block
 * iters[l] floats.  best_idx_out[n_levels], ratio_out[n_levels] (entries of
 * skipped levels are -1 / 0).  final_* refer to the last level run (level of
 * the smallest index with iters>0). */
int dvo_oracle_align_pyramid(const dvo_oracle_params *prm, int n_levels, const int *iters,
                             const float *const *xyz, const int *N,
                             const float *const *dt, const float *const *gx, const float *const *gy,
                             const int *rows, const int *cols,
                             float fx, float fy, float cx, float cy,
                             double *R, double *t,
                             float *energy_out, int *best_idx_out, float *ratio_out,
                             float *final_eps, float *final_reproj);

/* n_pairs independent alignments from the identity, OpenMP over pairs (dvo_oracle_batch.cpp); pair i
 * aligns scene i % n_scenes, per-level inputs of scene s at index s * n_levels + l.  Returns the threads used. */
int dvo_oracle_align_batch_omp(const dvo_oracle_params *prm, int n_pairs, int n_scenes, int n_levels, const int *iters,
                               const float *const *xyz, const int *N, const float *const *dt, const float *const *gx,
                               const float *const *gy, const int *rows, const int *cols, float fx, float fy, float cx, float cy,
                               int n_threads, double *R_out, double *t_out, double *seconds_out, double *thread_seconds,
                               int *thread_pairs);

/* Now-frame preprocessing after Canny (computeDistTransfrmOfNow :1768-1795, imageGradient :1063-1098):
 * edge mask (uint8, >0 = edge, column-major) -> exact EDT -> min-max normalise to [0,255] -> central
 * differences with reflect-101 border.  OpenCV 2.4 semantics restated, unpinned (see the .cpp).
 * DECISION (round 2) on cv::normalize(src, dst, 0, 255, NORM_MINMAX) for a CV_32F image: OpenCV 2.4 computes
 * scale = 255*(1./(smax-smin)) and shift = 0 - smin*scale in double (cv::normalize, core/src/convert.cpp) and hands
 * them to Mat::convertTo, whose 32F -> 32F kernel (cvtScale32f = cvtScale_<float, float, float>) evaluates
 * dst = src*(float)scale + (float)shift in FLOAT.  The oracle, the GPU frame path and the synthetic scene generator
 * all use that form; the round-1 double evaluation (src-min)*(255/(max-min)) differed by one ulp on many pixels.
 * scipy.ndimage.distance_transform_edt cross-checks the EDT itself (tests/test_oracle_pins.py). */
void dvo_oracle_now_level_from_edges(const unsigned char *edge, int rows, int cols,
                                     float *dt, float *gx, float *gy);

/* ---- rows f1/f2: per-frame preprocessing outside the iteration loop (dvo_oracle_frames.cpp; OpenCV 2.4
 * semantics restated, PARITY UNPINNED).  Images here are ROW-major (OpenCV layout). ---- */
/* cv::Sobel(src, CV_16S, 1,0 / 0,1, 3, BORDER_REPLICATE) as cv::Canny calls it */
void dvo_oracle_sobel3(const unsigned char *src, int rows, int cols, short *dx, short *dy);
/* cv::Canny(src, dst, threshold1, threshold2, 3, true)  (SolveDVO.cpp:1704, :1764 with 150, 100); dst 0/255 */
void dvo_oracle_canny(const unsigned char *src, int rows, int cols, double threshold1, double threshold2,
                      unsigned char *dst);
/* same with the intermediate stages: squared magnitude, candidate map (0 / 1 weak / 2 strong); any may be NULL */
void dvo_oracle_canny_stages(const unsigned char *src, int rows, int cols, double threshold1, double threshold2,
                             int *mag_out, unsigned char *cand_out, unsigned char *dst);
/* cv::cvtColor(CV_BGR2GRAY), 8-bit  (camTopic2PublisherPyD.cpp:347) */
void dvo_oracle_bgr2gray(const unsigned char *bgr, size_t npx, unsigned char *grey);
/* cv::resize(src, dst, Size(), scale, scale, INTER_NEAREST)  (camTopic2PublisherPyD.cpp:344-345) */
void dvo_oracle_resize_nn_size(int rows, int cols, double scale, int *drows, int *dcols);
void dvo_oracle_resize_nn(const void *src, int rows, int cols, int elem_bytes, double scale, void *dst);
/* depthRcvd (camTopic2PublisherPyD.cpp:73-77): 1000.0*depth -> CV_16U -> 0 becomes 1 */
void dvo_oracle_depth_m_to_mm16(const float *depth_m, size_t npx, unsigned short *out);
/* cv::undistort (camTopic2PublisherPyD.cpp:88-107): bgr8 (rows x cols x 3) and mono16 images, row-major; K4 = fx fy cx cy,
 * D5 = k1 k2 p1 p2 k3 (sensor_msgs/CameraInfo K and D, :52-61) */
void dvo_oracle_undistort_bgr8(const unsigned char *src, int rows, int cols, const double *K4, const double *D5, unsigned char *dst);
void dvo_oracle_undistort_u16(const unsigned short *src, int rows, int cols, const double *K4, const double *D5, unsigned short *dst);
/* ... of a sensor-unit depth image given as floats (DVO_UPLOAD_DEPTH_RAW): the output is still saturate_cast<ushort>(cvRound(sum)),
 * so a sum that is NaN, infinite or >= 2^31 in magnitude gives 0 (dvo_oracle_frames.cpp) */
void dvo_oracle_undistort_u16_from_f32(const float *src, int rows, int cols, const double *K4, const double *D5, unsigned short *dst);
/* the CV_16SC2 map cv::undistort remaps with: integer source pixel (sx, sy) and fraction index fy*32 + fx per pixel, row-major */
void dvo_oracle_undistort_map(int rows, int cols, const double *K4, const double *D5, short *sx, short *sy, unsigned short *frac);

/* ---- row f4 / A14: the legacy photometric Gauss-Newton odometry, RGBDOdometry (src/RGBDOdometry.cpp:363-746), restated in
 * dvo_oracle_photo.cpp (PARITY UNPINNED; `fixed` = 0 reproduces the reference's defects, 1 corrects them -- see the .cpp).
 * Images row-major like cv::Mat; depth in sensor units; T 4x4 row-major (Eigen::Transform<double,3,Affine>::matrix()). */
int dvo_oracle_photo_jacobian(const unsigned char *grey, const unsigned short *depth, int rows, int cols, int level,
                              double fx, double fy, double cx, double cy, int fixed, double grad_threshold, int capacity,
                              double *J, int *sel_i, int *sel_j, double *A36);
double dvo_oracle_photo_epsilon(const unsigned char *grey_ref, const unsigned short *depth_ref, const unsigned char *grey_now,
                                int rows, int cols, int level, double fx, double fy, double cx, double cy, int fixed,
                                const int *sel_i, const int *sel_j, int n, const double *T16, double *eps);
int dvo_oracle_photo_gauss_newton(const unsigned char *grey_ref, const unsigned short *depth_ref, const unsigned char *grey_now,
                                  int rows, int cols, int level, double fx, double fy, double cx, double cy, int fixed,
                                  const double *J, const int *sel_i, const int *sel_j, int n, const double *A36,
                                  int max_iters, double eps_stop, double *T16, double *eps_norms);
void dvo_oracle_photo_exponential_map(const double *psi6, int fixed, double *out16);
void dvo_oracle_photo_solve6(const double *A36, const double *b6, double *x6);

/* Helpers exported for property tests. */
float dvo_oracle_weight(float r);                                   /* :1047-1053 */
float dvo_oracle_interpolate(const float *F, int rows, int cols, float ry, float rx); /* :1285-1308 */
void  dvo_oracle_se3_exp(const double *psi, double *R, double *t);  /* Sophus SE3d::exp */
void  dvo_oracle_se3_log(const double *R, const double *t, double *psi); /* Sophus SE3d::log */
void  dvo_oracle_rotationize(double *R);                            /* :1269-1282 */
void  dvo_oracle_svd3(const double *A, double *U, double *S, double *V); /* JacobiSVD */

#ifdef __cplusplus
}
#endif
#endif
