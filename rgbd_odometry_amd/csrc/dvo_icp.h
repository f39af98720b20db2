/*
 * dvo_icp.h -- projective point-to-plane ICP of depth frames against ray-cast model views (include/dvo_amd.h, "frame-to-model
 * alignment"): the definition, in plain C++.  It follows the rules of dvo_tsdf_map.h, which it includes for the depth formats and the
 * refusals of a camera and a pose: no device, no context, IEEE double in the order written, nothing fused (-ffp-contract=off), no
 * transcendental function; division and sqrt in double only, both correctly rounded on the host and on the device.  dvo_icp_align_host
 * is align() below; the kernels (dvo_icp.hip) call term() and after_sweep() -- the whole per-pixel and per-sweep functions -- as they are.
 *
 * A view is a now-depth image and a model depth image, both rows x cols (each DVO_DEPTH_U16 millimetres or DVO_DEPTH_F32 metres, the
 * hole rules of the fusion section), the model's normals (three floats per pixel in world axes, (0, 0, 0) = none: what
 * dvo_raycast_views writes), one K4 = fx, fy, cx, cy for both images, the model view's pose Tm = {Rm, tm} and a start pose T = {R, t} of
 * the now frame.  Poses are 12 doubles, R column-major then t, camera to world.  A call aligns `count` views independently.
 *
 * Pixel term at the estimate (R, t), now pixel (u, v).  A skipped pixel contributes +0.0 to every sum and 0 to the count.
 *   D = metres of now[v][u]; skip a hole, D <= z_near and D > z_far;
 *   pc = (((double)u - cx) / fx * D, ((double)v - cy) / fy * D, D); p = R pc + t;
 *   q = Rm^T (p - tm); skip unless q.z > z_near;
 *   um = floor((fx (q.x / q.z) + cx) + 0.5), vm = floor((fy (q.y / q.z) + cy) + 0.5); skip unless 0 <= um < cols and 0 <= vm < rows
 *   (compared in double: a NaN falls out);
 *   Dm = metres of model[vm][um]; skip a hole;  n = the normal there, floats to doubles; skip when all three components are 0;
 *   mc = (((double)um - cx) / fx * Dm, ((double)vm - cy) / fy * Dm, Dm); m = Rm mc + tm; d = p - m; skip if d.d > dist_max dist_max;
 *   r = n.d;  wgt = 1 when huber <= 0 or |r| <= huber, else huber / |r|;
 *   J = (n, p x n): the six components in the tangent order (v, w) of a world-frame left increment p <- p + v + w x p;
 *   the sums: the 21 upper entries of sum (wgt J_i) J_j (row-major), the 6 of sum (wgt J_i) r, sum r r (unweighted), and the count.
 * Every product of a matrix and a vector, and every dot product, is ((a0 b0 + a1 b1) + a2 b2), a translation added last.
 *
 * Sum order (part of the definition: what makes a parallel device byte-equal).  The pixels a sweep visits form a list in raster order.
 *   tree64(x[0 .. 64)): for s = 32, 16, 8, 4, 2, 1: for l < s: x[l] = x[l] + x[l + s]; the result is x[0].
 *   The sum of a list: pad it with +0.0 to a multiple of 64, replace each run of 64 consecutive entries by its tree64, and repeat on the
 *   list of results until one value is left (a list always takes at least one round).
 * A wave's xor butterfly with the strides 32 .. 1 leaves the same bits in lane 0, IEEE addition being commutative.  The count is an
 * integer and has no order.
 *
 * Levels.  Level l visits the now pixels with u % 2^l == 0 and v % 2^l == 0 in the raster order of that sub-grid, ceil(cols / 2^l) per
 * row; the model images are always read at full resolution and no pyramid is built.  Levels run from levels - 1 down to 0 with
 * iterations[l] sweeps at level l.
 *
 * After each sweep, per view (after_sweep()):
 *   count < min_count: the view stops with DVO_ICP_FEW;
 *   A = L D L^T without a square root (ldlt6() below has the order); a pivot that fails D_k > min_pivot_ratio A_kk stops the view with
 *   DVO_ICP_DEGENERATE -- where a single plane ends, its first three columns of J being one vector;
 *   else solve A x = -b, x = (v, w), and update with the Cayley map (no sine, no cosine): a = w / 2, C = I + (2 / (1 + a.a)) ([a]x +
 *   [a]x^2), R <- C R, t <- C t + v;  x.x < stop_norm stop_norm: the rest of this level's sweeps are skipped for this view.
 * A stopped view keeps the pose it had and takes no further sweeps.
 * After level 0 one more level-0 sweep runs with no update, unless the view stopped with FEW or DEGENERATE -- then the record comes
 * from the sweep that stopped it -- so the record describes the returned pose: status, iterations (the updates applied), count,
 * sum_r2, rms = sqrt(sum_r2 / count) (0 for count 0) and info[36], the full symmetric sum (wgt J_i) J_j, row-major.
 *
 * The normal gate (align_gated(); taken only when a view has now normals: three floats per now pixel in the axes of the now camera,
 * (0, 0, 0) = none -- what dvo_icp_prepare.h defines).  In the pixel term, after the model normal n has been read:
 *   nn = the now normal at now pixel (v, u), floats to doubles; skip when all three components are 0;
 *   nw_k = (R[k] nn0 + R[3 + k] nn1) + R[6 + k] nn2 (no translation);  c = (n0 nw0 + n1 nw1) + n2 nw2;
 *   skip unless c >= normal_cos_min (a NaN falls out).
 * A skip contributes +0.0 everywhere, so its place among the other skips does not change a bit.  Unit length of either normal is the
 * caller's business.  Without now normals a view is aligned as before, bit for bit.
 *
 * OUT OF SCOPE: a depth pyramid, separate intrinsics for the model and the now frame, damping, colour terms.
 */
#ifndef DVO_ICP_H_
#define DVO_ICP_H_

#include "dvo_tsdf_map.h"

/* the public structs as include/dvo_amd.h declares them (the same text under the same guard) */
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

namespace dvo_icp {

using dvo_tsdf::finite;
using dvo_tsdf::format_ok;
using dvo_tsdf::frame_ok;
using dvo_tsdf::kFormatU16;

constexpr int kMaxLevels = DVO_ICP_MAX_LEVELS;
constexpr int kSums = 28;                          /* 21 of A, 6 of b, sum r r */
constexpr int kTreeRounds = 4;                     /* 64^4 = 2^24 = DVO_ICP_MAX_PIXELS */

inline void params_default(dvo_icp_params *p) {
    p->levels = 3;
    p->iterations[0] = 10; p->iterations[1] = 5; p->iterations[2] = 4; p->iterations[3] = 0;
    p->z_near = 0.1; p->z_far = 8.0; p->dist_max = 0.1; p->huber = 0.0; p->stop_norm = 0.0; p->min_pivot_ratio = 1e-9;
    p->min_count = 6;
}
inline bool params_ok(const dvo_icp_params *p) {
    if (!p || p->levels < 1 || p->levels > kMaxLevels || p->min_count < 1) return false;
    for (int l = 0; l < kMaxLevels; l++)
        if (p->iterations[l] < 0 || p->iterations[l] > DVO_ICP_MAX_ITERATIONS) return false;
    if (!finite(p->z_near) || !finite(p->z_far) || !finite(p->dist_max) || !finite(p->huber) || !finite(p->stop_norm) || !finite(p->min_pivot_ratio))
        return false;
    return p->z_near > 0.0 && p->z_near < p->z_far && p->dist_max > 0.0 && p->huber >= 0.0 && p->stop_norm >= 0.0 && p->min_pivot_ratio > 0.0 &&
           p->min_pivot_ratio < 1.0;
}
inline bool shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && (long long)rows * (long long)cols <= (long long)DVO_ICP_MAX_PIXELS; }
/* the sweeps of a call: the updates of the levels in use, and the record's */
inline int sweeps_of(const dvo_icp_params &p) {
    int n = 1;
    for (int l = 0; l < p.levels; l++) n += p.iterations[l];
    return n;
}

/* ---- the per-pixel and per-sweep functions, shared with the device ---- */

/* one view: the model's pose and the camera, and where the three images are */
struct View {
    double Rm[9], tm[3], K[4];
    const void *now, *model;
    const float *normals;
    const float *now_normals;                      /* NULL: ungated */
};
struct SweepConst { int now_format, model_format, rows, cols; double z_near, z_far, dist_max2, huber, normal_cos_min; };
/* a view's estimate and where it stands: stopped with `status`, or converged at conv_level (-1: at none) */
struct State {
    double R[9], t[3];
    int status, stopped, conv_level, iterations;
};
DVO_TSDF_HD void state_start(State &s, const double *pose12) {
    for (int k = 0; k < 9; k++) s.R[k] = pose12[k];
    for (int k = 0; k < 3; k++) s.t[k] = pose12[9 + k];
    s.status = DVO_ICP_OK; s.stopped = 0; s.conv_level = -1; s.iterations = 0;
}
/* does the view take the sweeps of this level? */
DVO_TSDF_HD bool takes_part(const State &s, int level) { return !s.stopped && s.conv_level != level; }

/* the list of a level: its width, its length, and the pixel of entry e */
DVO_TSDF_HD int level_cols(int cols, int level) { return (cols + (1 << level) - 1) >> level; }
DVO_TSDF_HD int level_entries(int rows, int cols, int level) { return level_cols(cols, level) * level_cols(rows, level); }

DVO_TSDF_HD bool metres(const void *image, int format, size_t px, double *D) {
    return format == kFormatU16 ? dvo_tsdf::metres_u16(static_cast<const unsigned short *>(image)[px], D)
                                : dvo_tsdf::metres_f32(static_cast<const float *>(image)[px], D);
}
/* R x + t, R column-major */
DVO_TSDF_HD void transform(const double *R, const double *t, const double *x, double *y) {
    y[0] = ((R[0] * x[0] + R[3] * x[1]) + R[6] * x[2]) + t[0];
    y[1] = ((R[1] * x[0] + R[4] * x[1]) + R[7] * x[2]) + t[1];
    y[2] = ((R[2] * x[0] + R[5] * x[1]) + R[8] * x[2]) + t[2];
}

/* the term of now pixel (u, v) at the estimate (R, t): the kSums sums' entries into s; false: skipped, every entry +0.0.  GATED: the
 * view has now normals (a compile-time flag, so that the ungated code is what it was) */
template <bool GATED>
DVO_TSDF_HD bool term_of(const View &V, const SweepConst &c, const double *R, const double *t, int u, int v, double *s) {
    for (int k = 0; k < kSums; k++) s[k] = 0.0;
    const double fx = V.K[0], fy = V.K[1], cx = V.K[2], cy = V.K[3];
    double D;
    if (!metres(V.now, c.now_format, (size_t)v * (size_t)c.cols + (size_t)u, &D)) return false;
    if (D <= c.z_near || D > c.z_far) return false;
    const double pc[3] = {((double)u - cx) / fx * D, ((double)v - cy) / fy * D, D};
    double p[3];
    transform(R, t, pc, p);
    const double e[3] = {p[0] - V.tm[0], p[1] - V.tm[1], p[2] - V.tm[2]};
    const double qx = (V.Rm[0] * e[0] + V.Rm[1] * e[1]) + V.Rm[2] * e[2];
    const double qy = (V.Rm[3] * e[0] + V.Rm[4] * e[1]) + V.Rm[5] * e[2];
    const double qz = (V.Rm[6] * e[0] + V.Rm[7] * e[1]) + V.Rm[8] * e[2];
    if (!(qz > c.z_near)) return false;
    const double um = floor((fx * (qx / qz) + cx) + 0.5), vm = floor((fy * (qy / qz) + cy) + 0.5);
    if (!(um >= 0.0 && um < (double)c.cols && vm >= 0.0 && vm < (double)c.rows)) return false;       /* NaN falls out here */
    const size_t px = (size_t)(int)vm * (size_t)c.cols + (size_t)(int)um;
    double Dm;
    if (!metres(V.model, c.model_format, px, &Dm)) return false;
    const double n[3] = {(double)V.normals[3 * px], (double)V.normals[3 * px + 1], (double)V.normals[3 * px + 2]};
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return false;
    if (GATED) {
        const float *q = V.now_normals + 3 * ((size_t)v * (size_t)c.cols + (size_t)u);
        const double nn[3] = {(double)q[0], (double)q[1], (double)q[2]};
        if (nn[0] == 0.0 && nn[1] == 0.0 && nn[2] == 0.0) return false;
        const double nw[3] = {(R[0] * nn[0] + R[3] * nn[1]) + R[6] * nn[2], (R[1] * nn[0] + R[4] * nn[1]) + R[7] * nn[2],
                              (R[2] * nn[0] + R[5] * nn[1]) + R[8] * nn[2]};
        if (!((n[0] * nw[0] + n[1] * nw[1]) + n[2] * nw[2] >= c.normal_cos_min)) return false;       /* NaN falls out here */
    }
    const double mc[3] = {(um - cx) / fx * Dm, (vm - cy) / fy * Dm, Dm};
    double m[3];
    transform(V.Rm, V.tm, mc, m);
    const double d[3] = {p[0] - m[0], p[1] - m[1], p[2] - m[2]};
    if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > c.dist_max2) return false;
    const double r = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const double ar = fabs(r);
    const double wgt = (c.huber <= 0.0 || ar <= c.huber) ? 1.0 : c.huber / ar;
    const double J[6] = {n[0], n[1], n[2], p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0]};
    int at = 0;
    for (int i = 0; i < 6; i++) {
        const double wJ = wgt * J[i];
        for (int j = i; j < 6; j++) s[at++] = wJ * J[j];
        s[21 + i] = wJ * r;
    }
    s[27] = r * r;
    return true;
}
DVO_TSDF_HD bool term(const View &V, const SweepConst &c, const double *R, const double *t, int u, int v, double *s) {
    return V.now_normals ? term_of<true>(V, c, R, t, u, v, s) : term_of<false>(V, c, R, t, u, v, s);
}

/* entry (i, j) of the upper triangle, row-major, i <= j */
DVO_TSDF_HD int upper(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

/* A = L D L^T, column by column, every inner sum subtracted term by term in ascending k:
 *   D_j = A_jj - sum_{k<j} (L_jk L_jk) D_k;  refused unless D_j > min_pivot_ratio A_jj;  L_ij = (A_ij - sum_{k<j} (L_ik L_jk) D_k) / D_j, i > j;
 * then L y = -b downwards (y_i = -b_i - sum_{k<i} L_ik y_k), z_i = y_i / D_i, and L^T x = z upwards (x_i = z_i - sum_{k>i} L_ki x_k,
 * ascending k).  sums: the 21 of A and the 6 of b.  false: a pivot failed */
DVO_TSDF_HD bool ldlt6(const double *sums, double min_pivot_ratio, double *x) {
    double L[6][6], D[6];
    for (int j = 0; j < 6; j++) {
        const double ajj = sums[upper(j, j)];
        double dj = ajj;
        for (int k = 0; k < j; k++) dj = dj - (L[j][k] * L[j][k]) * D[k];
        if (!(dj > min_pivot_ratio * ajj)) return false;                                             /* NaN falls out here */
        D[j] = dj;
        for (int i = j + 1; i < 6; i++) {
            double a = sums[upper(j, i)];
            for (int k = 0; k < j; k++) a = a - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = a / dj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double a = -sums[21 + i];
        for (int k = 0; k < i; k++) a = a - L[i][k] * y[k];
        y[i] = a;
    }
    for (int i = 5; i >= 0; i--) {
        double a = y[i] / D[i];
        for (int k = i + 1; k < 6; k++) a = a - L[k][i] * x[k];
        x[i] = a;
    }
    return true;
}

/* the Cayley update of (R, t) by x = (v, w) */
DVO_TSDF_HD void cayley_update(double *R, double *t, const double *x) {
    const double a0 = x[3] * 0.5, a1 = x[4] * 0.5, a2 = x[5] * 0.5;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2, s = 2.0 / (1.0 + aa);
    const double C[9] = {1.0 + s * (a0 * a0 - aa), s * (a0 * a1 - a2),       s * (a0 * a2 + a1),            /* row-major */
                         s * (a1 * a0 + a2),       1.0 + s * (a1 * a1 - aa), s * (a1 * a2 - a0),
                         s * (a2 * a0 - a1),       s * (a2 * a1 + a0),       1.0 + s * (a2 * a2 - aa)};
    double Rn[9], tn[3];
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) Rn[i + 3 * j] = (C[3 * i] * R[3 * j] + C[3 * i + 1] * R[3 * j + 1]) + C[3 * i + 2] * R[3 * j + 2];
    for (int i = 0; i < 3; i++) tn[i] = ((C[3 * i] * t[0] + C[3 * i + 1] * t[1]) + C[3 * i + 2] * t[2]) + x[i];
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
    for (int k = 0; k < 3; k++) t[k] = tn[k];
}

DVO_TSDF_HD void fill_record(const State &st, const double *sums, int count, dvo_icp_record *rec) {
    rec->status = st.status; rec->iterations = st.iterations; rec->count = count; rec->reserved = 0;
    rec->sum_r2 = sums[27];
    rec->rms = count > 0 ? sqrt(sums[27] / (double)count) : 0.0;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) rec->info[6 * i + j] = sums[i <= j ? upper(i, j) : upper(j, i)];
}

/* what follows a sweep of `level` that the view took part in; record_sweep: the one after level 0, with no update.  true: the view's
 * pose and *rec are its result */
DVO_TSDF_HD bool after_sweep(State &st, const double *sums, int count, const dvo_icp_params &p, int level, bool record_sweep, dvo_icp_record *rec) {
    if (!record_sweep) {
        double x[6];
        if (count < p.min_count) st.status = DVO_ICP_FEW;
        else if (!ldlt6(sums, p.min_pivot_ratio, x)) st.status = DVO_ICP_DEGENERATE;
        if (st.status == DVO_ICP_OK) {
            cayley_update(st.R, st.t, x);
            st.iterations++;
            const double xx = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
            if (xx < p.stop_norm * p.stop_norm) st.conv_level = level;
            return false;
        }
        st.stopped = 1;
    }
    fill_record(st, sums, count, rec);
    return true;
}

/* tree64 in place */
DVO_TSDF_HD double tree64(double *x) {
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; l++) x[l] = x[l] + x[l + s];
    return x[0];
}

/* ---- the host: the sum of a list taken as its entries arrive ---- */

/* round k's pending run of up to 64 values per sum; a full run goes up one round as its tree64 */
struct TreeSum {
    double x[kTreeRounds + 1][kSums][64];
    int fill[kTreeRounds + 1];
    long long pushed[kTreeRounds + 1];
    TreeSum() { reset(); }
    void reset() { for (int k = 0; k <= kTreeRounds; k++) { fill[k] = 0; pushed[k] = 0; } }
    void push(int round, const double *s) {
        for (int k = 0; k < kSums; k++) x[round][k][fill[round]] = s[k];
        fill[round]++; pushed[round]++;
        if (fill[round] == 64) close(round);
    }
    void close(int round) {                        /* the pending run, padded with +0.0 */
        double up[kSums];
        for (int k = 0; k < kSums; k++) {
            for (int l = fill[round]; l < 64; l++) x[round][k][l] = 0.0;
            up[k] = tree64(x[round][k]);
        }
        fill[round] = 0;
        push(round + 1, up);
    }
    void finish(double *sums) {                    /* at least one entry was pushed */
        for (int round = 0; round < kTreeRounds; round++) {
            if (fill[round] > 0) close(round);
            if (pushed[round + 1] == 1) {
                for (int k = 0; k < kSums; k++) sums[k] = x[round + 1][k][0];
                return;
            }
        }
    }
};

/* one sweep of a view at `level`: the sums and the count */
inline void sweep(const View &V, const SweepConst &c, const State &st, int level, TreeSum &ts, double *sums, int *count) {
    ts.reset();
    int n = 0;
    double s[kSums];
    for (int v = 0; v < c.rows; v += 1 << level)
        for (int u = 0; u < c.cols; u += 1 << level) {
            if (term(V, c, st.R, st.t, u, v, s)) n++;
            ts.push(0, s);
        }
    ts.finish(sums);
    *count = n;
}

/* ---- the entry point ---- */

/* what every public call refuses in its lists */
inline bool views_ok(int count, const double *K4, const void *const *now_depth, const void *const *model_depth, const float *const *model_normals,
                     const double *model_poses12, const double *start_poses12) {
    if (count < 1 || !K4 || !now_depth || !model_depth || !model_normals || !model_poses12 || !start_poses12) return false;
    for (int i = 0; i < count; i++)
        if (!now_depth[i] || !model_depth[i] || !model_normals[i] || !frame_ok(K4 + 4 * (size_t)i, model_poses12 + 12 * (size_t)i) ||
            !frame_ok(K4 + 4 * (size_t)i, start_poses12 + 12 * (size_t)i))
            return false;
    return true;
}
inline SweepConst sweep_const(const dvo_icp_params &p, int now_format, int model_format, int rows, int cols, double normal_cos_min = 0.0) {
    SweepConst c;
    c.now_format = now_format; c.model_format = model_format; c.rows = rows; c.cols = cols;
    c.z_near = p.z_near; c.z_far = p.z_far; c.dist_max2 = p.dist_max * p.dist_max; c.huber = p.huber; c.normal_cos_min = normal_cos_min;
    return c;
}
/* what the gated calls refuse on top: a NULL entry of a non-NULL list, a normal_cos_min that is not finite or outside [-1, 1] */
inline bool gate_ok(int count, const float *const *now_normals, double normal_cos_min) {
    if (!now_normals) return true;
    if (!finite(normal_cos_min) || normal_cos_min < -1.0 || normal_cos_min > 1.0) return false;
    for (int i = 0; i < count; i++)
        if (!now_normals[i]) return false;
    return true;
}
inline View make_view(const double *K4, const double *model_pose12, const void *now, const void *model, const float *normals,
                      const float *now_normals = nullptr) {
    View V;
    for (int k = 0; k < 9; k++) V.Rm[k] = model_pose12[k];
    for (int k = 0; k < 3; k++) V.tm[k] = model_pose12[9 + k];
    for (int k = 0; k < 4; k++) V.K[k] = K4[k];
    V.now = now; V.model = model; V.normals = normals; V.now_normals = now_normals;
    return V;
}

/* views 0 .. count - 1, independently: K4 4 doubles per view, the poses 12 per view; poses12_out 12 doubles and one record per view.
 * now_normals: NULL (ungated: normal_cos_min is ignored) or one image of now normals per view.  False: refused, nothing written */
inline bool align_gated(const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                        const void *const *now_depth, const void *const *model_depth, const float *const *model_normals, const double *model_poses12,
                        const double *start_poses12, const float *const *now_normals, double normal_cos_min, double *poses12_out,
                        dvo_icp_record *records) {
    if (!params_ok(p) || !format_ok(now_format) || !format_ok(model_format) || !shape_ok(rows, cols) || !poses12_out || !records ||
        !views_ok(count, K4, now_depth, model_depth, model_normals, model_poses12, start_poses12) || !gate_ok(count, now_normals, normal_cos_min))
        return false;
    const SweepConst c = sweep_const(*p, now_format, model_format, rows, cols, now_normals ? normal_cos_min : 0.0);
    TreeSum ts;                                    /* 70 KiB */
    for (int i = 0; i < count; i++) {
        const View V = make_view(K4 + 4 * (size_t)i, model_poses12 + 12 * (size_t)i, now_depth[i], model_depth[i], model_normals[i],
                                 now_normals ? now_normals[i] : nullptr);
        State st;
        state_start(st, start_poses12 + 12 * (size_t)i);
        double sums[kSums];
        int n = 0;
        for (int level = p->levels - 1; level >= 0; level--)
            for (int it = 0; it < p->iterations[level]; it++) {
                if (!takes_part(st, level)) continue;
                sweep(V, c, st, level, ts, sums, &n);
                (void)after_sweep(st, sums, n, *p, level, false, records + i);
            }
        if (!st.stopped) {
            sweep(V, c, st, 0, ts, sums, &n);
            (void)after_sweep(st, sums, n, *p, 0, true, records + i);
        }
        for (int k = 0; k < 9; k++) poses12_out[12 * (size_t)i + k] = st.R[k];
        for (int k = 0; k < 3; k++) poses12_out[12 * (size_t)i + 9 + k] = st.t[k];
    }
    return true;
}
inline bool align(const dvo_icp_params *p, int count, int now_format, int model_format, int rows, int cols, const double *K4,
                  const void *const *now_depth, const void *const *model_depth, const float *const *model_normals, const double *model_poses12,
                  const double *start_poses12, double *poses12_out, dvo_icp_record *records) {
    return align_gated(p, count, now_format, model_format, rows, cols, K4, now_depth, model_depth, model_normals, model_poses12, start_poses12, nullptr,
                       0.0, poses12_out, records);
}

}  // namespace dvo_icp
#endif
