/*
 * dvo_pose_graph.h -- pose-graph optimisation (include/dvo_amd.h, "pose graphs"): the definition, in plain C++.  No device, no context,
 * no other header of the library: dvo_graph_solve_host is solve_host() below, the device kernel (dvo_pose_graph.hip) shares every
 * per-edge and per-node function with it, and a stand-alone program can include the file as it is.
 *
 * A pose is 12 doubles {R column-major, t}; node pose T_n maps node-frame points to the world.  An edge (i, j, Z, Omega, flags)
 * measures Z ~ T_i^-1 T_j.  Tangent order [translation, rotation], right perturbation T <- T Exp(d), full SE(3) exponential.
 *   r = Log(Z^-1 T_i^-1 T_j),  s^2 = r^T Omega r,  cost = sum rho(s^2)  (rho = s^2, or Huber on edges flagged DVO_GRAPH_EDGE_ROBUST)
 *   J_j = Jr^-1(r),  J_i = -Jr^-1(r) Ad(T_j^-1 T_i),  Jr^-1(r) = I + ad/2 + ad^2/12 - ad^4/720  (the truncation is the definition)
 * Levenberg-Marquardt: (H + lambda diag H) x = -b by block-Jacobi preconditioned CG, matrix-free over the per-node incidence lists
 * (a CSR in edge order, built by build_csr), trial poses T_n Exp(x_n) re-orthogonalised by the polar factor, accepted when the
 * robust cost does not increase.  Every loop is capped.
 *
 * All arithmetic is IEEE double in the order written, nothing fused (-ffp-contract=off); every sum of the host solver runs in index
 * order.  The logarithm covers the closed ball theta <= pi: near a half turn the axis is taken from the symmetric part of R (se3_log).
 */
#ifndef DVO_POSE_GRAPH_H_
#define DVO_POSE_GRAPH_H_

#include <math.h>
#include <stddef.h>

#include <vector>

#if defined(__HIPCC__)
#define DVO_PG_HD __host__ __device__ inline
#define DVO_PG_UNROLL _Pragma("unroll")
#else
#define DVO_PG_HD inline
#define DVO_PG_UNROLL
#endif

/* the types as include/dvo_amd.h declares them (the same text under the same guard: whichever header comes first defines them) */
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
/* the types of the marginal covariances, likewise */
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

namespace dvo_pg {

constexpr int kOk = 0, kInvalid = 1;               /* == DVO_OK, DVO_ERR_INVALID */
/* per-edge blocks of one linearisation: H_ii, H_ij, H_jj (6 x 6 row-major each), b_i, b_j */
constexpr int kBlk = 120, kHii = 0, kHij = 36, kHjj = 72, kBi = 108, kBj = 114;
/* per-node record of one outer iteration: diag of the assembled block, the inverse of the damped block (by Cholesky), b */
constexpr int kNode = 48, kDg = 0, kMinv = 6, kB = 42;
constexpr double kSmall2 = 1e-4;                   /* theta^2 below it: series */
constexpr double kNearPi = 0.1;                    /* sin(theta) below it with cos(theta) < 0: Log takes the axis from the symmetric part */

/* finite: neither NaN nor an infinity (x - x is NaN for both) */
DVO_PG_HD bool is_finite(double x) { return x - x == 0.0; }

/* C = A B, 6 x 6 row-major, every sum in index order from 0 */
DVO_PG_HD void mul6(const double *A, const double *B, double *C) {
    DVO_PG_UNROLL
    for (int r = 0; r < 6; r++) {
        DVO_PG_UNROLL
        for (int c = 0; c < 6; c++) {
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 6; k++) s += A[r * 6 + k] * B[k * 6 + c];
            C[r * 6 + c] = s;
        }
    }
}
/* y = A x */
DVO_PG_HD void mulv6(const double *A, const double *x, double *y) {
    DVO_PG_UNROLL
    for (int r = 0; r < 6; r++) {
        double s = 0.0;
        DVO_PG_UNROLL
        for (int k = 0; k < 6; k++) s += A[r * 6 + k] * x[k];
        y[r] = s;
    }
}

/* A = L L^T (lower, row-major); false unless every pivot is positive */
DVO_PG_HD bool chol6(const double *A, double *L) {
    DVO_PG_UNROLL
    for (int k = 0; k < 36; k++) L[k] = 0.0;
    DVO_PG_UNROLL
    for (int j = 0; j < 6; j++) {
        double d = A[j * 6 + j];
        DVO_PG_UNROLL
        for (int k = 0; k < j; k++) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0.0) || !is_finite(d)) return false;
        L[j * 6 + j] = sqrt(d);
        DVO_PG_UNROLL
        for (int i = j + 1; i < 6; i++) {
            double v = A[i * 6 + j];
            DVO_PG_UNROLL
            for (int k = 0; k < j; k++) v -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = v / L[j * 6 + j];
        }
    }
    return true;
}
/* Ainv = L^-T L^-1 for A = L L^T; false as chol6 */
DVO_PG_HD bool inv6_spd(const double *A, double *Ainv) {
    double L[36], Li[36];
    if (!chol6(A, L)) return false;
    DVO_PG_UNROLL
    for (int k = 0; k < 36; k++) Li[k] = 0.0;
    DVO_PG_UNROLL
    for (int k = 0; k < 6; k++) {
        DVO_PG_UNROLL
        for (int i = k; i < 6; i++) {
            double v = (i == k) ? 1.0 : 0.0;
            DVO_PG_UNROLL
            for (int m = k; m < i; m++) v -= L[i * 6 + m] * Li[m * 6 + k];
            Li[i * 6 + k] = v / L[i * 6 + i];
        }
    }
    DVO_PG_UNROLL
    for (int i = 0; i < 6; i++) {
        DVO_PG_UNROLL
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
            DVO_PG_UNROLL
            for (int m = 0; m < 6; m++) v += Li[m * 6 + i] * Li[m * 6 + j];
            Ainv[i * 6 + j] = v;
        }
    }
    return true;
}

DVO_PG_HD void cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

/* Exp of d = [v, w]: R = I + A W + B W^2 (column-major), t = v + B (w x v) + C (w x (w x v)) */
DVO_PG_HD void se3_exp(const double *d, double *R, double *t) {
    const double *v = d, *w = d + 3;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B, C;
    if (th2 < kSmall2) {
        A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
        B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
        C = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
    } else {
        const double th = sqrt(th2), s = sin(th), h = sin(0.5 * th);
        A = s / th;
        B = 2.0 * h * h / th2;
        C = (th - s) / (th2 * th);
    }
    R[0] = 1.0 + B * (w[0] * w[0] - th2);
    R[4] = 1.0 + B * (w[1] * w[1] - th2);
    R[8] = 1.0 + B * (w[2] * w[2] - th2);
    R[1] = B * (w[0] * w[1]) + A * w[2];      /* R(1,0) */
    R[3] = B * (w[0] * w[1]) - A * w[2];      /* R(0,1) */
    R[2] = B * (w[0] * w[2]) - A * w[1];      /* R(2,0) */
    R[6] = B * (w[0] * w[2]) + A * w[1];      /* R(0,2) */
    R[5] = B * (w[1] * w[2]) + A * w[0];      /* R(2,1) */
    R[7] = B * (w[1] * w[2]) - A * w[0];      /* R(1,2) */
    double c1[3], c2[3];
    cross3(w, v, c1);
    cross3(w, c1, c2);
    DVO_PG_UNROLL
    for (int k = 0; k < 3; k++) t[k] = v[k] + B * c1[k] + C * c2[k];
}

/* Log of (R, t): r = [v, w], theta = atan2(s, c) with s a = the antisymmetric part (s = sin theta, a the axis) and c = cos theta from
 * the trace; v = t - (w x t)/2 + D (w x (w x t)).  w = (theta / s) s a, except near a half turn (c < 0, s < kNearPi), where s a loses its
 * direction to rounding (by eps / s) and vanishes at pi: there the axis comes from the symmetric part, (R + R^T)/2 = c I + (1 - c) a a^T
 * -- the column of the largest a_k^2, normalised -- and only its sign from s a (at exactly pi both signs are the same rotation) */
DVO_PG_HD void se3_log(const double *R, const double *t, double *r) {
    const double sx = 0.5 * (R[5] - R[7]), sy = 0.5 * (R[6] - R[2]), sz = 0.5 * (R[1] - R[3]);
    const double s = sqrt(sx * sx + sy * sy + sz * sz), c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double th = atan2(s, c), th2 = th * th;
    double *w = r + 3;
    if (c < 0.0 && s < kNearPi) {
        const double ic = 1.0 / (1.0 - c);
        const double xx = (R[0] - c) * ic, yy = (R[4] - c) * ic, zz = (R[8] - c) * ic;                              /* a_k^2 */
        const double xy = 0.5 * (R[1] + R[3]) * ic, xz = 0.5 * (R[2] + R[6]) * ic, yz = 0.5 * (R[5] + R[7]) * ic;   /* a_j a_k */
        double ax, ay, az;
        if (xx >= yy && xx >= zz) { ax = sqrt(xx); ay = xy / ax; az = xz / ax; }
        else if (yy >= zz) { ay = sqrt(yy); ax = xy / ay; az = yz / ay; }
        else { az = sqrt(zz); ax = xz / az; ay = yz / az; }
        double f = th / sqrt(ax * ax + ay * ay + az * az);
        if (ax * sx + ay * sy + az * sz < 0.0) f = -f;
        w[0] = f * ax; w[1] = f * ay; w[2] = f * az;
    } else {
        const double f = (s > 1e-9) ? th / s : 1.0;
        w[0] = f * sx; w[1] = f * sy; w[2] = f * sz;
    }
    double D;
    if (th2 < kSmall2) {
        D = 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0;
    } else {
        const double hh = 0.5 * th;
        D = (1.0 - hh * cos(hh) / sin(hh)) / th2;
    }
    double c1[3], c2[3];
    cross3(w, t, c1);
    cross3(w, c1, c2);
    DVO_PG_UNROLL
    for (int k = 0; k < 3; k++) r[k] = t[k] - 0.5 * c1[k] + D * c2[k];
}

/* T_a^-1 T_b of two poses */
DVO_PG_HD void rel_pose(const double *Pa, const double *Pb, double *R, double *t) {
    DVO_PG_UNROLL
    for (int a = 0; a < 3; a++) {
        DVO_PG_UNROLL
        for (int b = 0; b < 3; b++) {
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 3; k++) s += Pa[k + 3 * a] * Pb[k + 3 * b];
            R[a + 3 * b] = s;
        }
    }
    double d[3];
    DVO_PG_UNROLL
    for (int k = 0; k < 3; k++) d[k] = Pb[9 + k] - Pa[9 + k];
    DVO_PG_UNROLL
    for (int a = 0; a < 3; a++) {
        double s = 0.0;
        DVO_PG_UNROLL
        for (int k = 0; k < 3; k++) s += Pa[k + 3 * a] * d[k];
        t[a] = s;
    }
}

/* r = Log(Z^-1 T_i^-1 T_j); Rij, tij (may be NULL) receive T_i^-1 T_j */
DVO_PG_HD void edge_residual(const double *Pi, const double *Pj, const dvo_graph_edge *E, double *r, double *Rij_out, double *tij_out) {
    double Rij[9], tij[3], Z[12], X[12];
    rel_pose(Pi, Pj, Rij, tij);
    DVO_PG_UNROLL
    for (int k = 0; k < 9; k++) { Z[k] = E->R[k]; X[k] = Rij[k]; }
    DVO_PG_UNROLL
    for (int k = 0; k < 3; k++) { Z[9 + k] = E->t[k]; X[9 + k] = tij[k]; }
    double RE[9], tE[3];
    rel_pose(Z, X, RE, tE);
    se3_log(RE, tE, r);
    if (Rij_out) {
        DVO_PG_UNROLL
        for (int k = 0; k < 9; k++) Rij_out[k] = Rij[k];
        DVO_PG_UNROLL
        for (int k = 0; k < 3; k++) tij_out[k] = tij[k];
    }
}

/* s^2 = r^T Omega r */
DVO_PG_HD double edge_s2(const double *info, const double *r) {
    double q[6];
    mulv6(info, r, q);
    double s2 = 0.0;
    DVO_PG_UNROLL
    for (int k = 0; k < 6; k++) s2 += r[k] * q[k];
    return s2;
}
DVO_PG_HD bool edge_is_robust(int flags, double delta) { return (flags & DVO_GRAPH_EDGE_ROBUST) != 0 && delta > 0.0; }
DVO_PG_HD double edge_rho(double s2, int flags, double delta) {
    if (!edge_is_robust(flags, delta)) return s2;
    const double s = sqrt(s2);
    if (s <= delta) return s2;
    return 2.0 * delta * s - delta * delta;
}
DVO_PG_HD double edge_weight(double s2, int flags, double delta) {
    if (!edge_is_robust(flags, delta)) return 1.0;
    const double s = sqrt(s2);
    if (!(s > delta)) return 1.0;                  /* s = 0 included */
    return delta / s;
}
/* rho of one edge at the poses P (12 doubles per node) */
DVO_PG_HD double edge_cost(const double *P, const dvo_graph_edge *E, double delta) {
    double r[6];
    edge_residual(P + 12 * (size_t)E->i, P + 12 * (size_t)E->j, E, r, nullptr, nullptr);
    return edge_rho(edge_s2(E->info, r), E->flags, delta);
}

/* Jr^-1(r) = I + ad/2 + ad^2/12 - ad^4/720, ad(r) = [[w^, v^], [0, w^]] */
DVO_PG_HD void jr_inv(const double *r, double *J) {
    double M[36], M2[36];
    DVO_PG_UNROLL
    for (int k = 0; k < 36; k++) M[k] = 0.0;
    const double *v = r, *w = r + 3;
    DVO_PG_UNROLL
    for (int b = 0; b < 2; b++) {                  /* w^ on both diagonal blocks */
        const int o = b * 21;
        M[o + 1] = -w[2]; M[o + 2] = w[1];
        M[o + 6] = w[2];  M[o + 8] = -w[0];
        M[o + 12] = -w[1]; M[o + 13] = w[0];
    }
    M[4] = -v[2]; M[5] = v[1];
    M[9] = v[2];  M[11] = -v[0];
    M[15] = -v[1]; M[16] = v[0];
    mul6(M, M, M2);
    DVO_PG_UNROLL
    for (int k = 0; k < 36; k++) J[k] = ((k % 7 == 0) ? 1.0 : 0.0) + 0.5 * M[k] + M2[k] / 12.0;
    mul6(M2, M2, M);                               /* ad^4 */
    DVO_PG_UNROLL
    for (int k = 0; k < 36; k++) J[k] = J[k] - M[k] / 720.0;
}

/* One edge linearised at the poses P: the blocks J_a^T (w Omega) J_c and J_a^T (w Omega) r into blk[kBlk] */
DVO_PG_HD void edge_linearise(const double *P, const dvo_graph_edge *E, double delta, double *blk) {
    double r[6], Rij[9], tij[3], Jj[36], Ji[36];
    edge_residual(P + 12 * (size_t)E->i, P + 12 * (size_t)E->j, E, r, Rij, tij);
    const double w = edge_weight(edge_s2(E->info, r), E->flags, delta);
    jr_inv(r, Jj);
    {   /* Ad(T_j^-1 T_i) = [[R, t^ R], [0, R]] with R = Rij^T, t = -Rij^T tij */
        double Ad[36], R[9], t[3];
        DVO_PG_UNROLL
        for (int a = 0; a < 3; a++) {
            DVO_PG_UNROLL
            for (int b = 0; b < 3; b++) R[a * 3 + b] = Rij[b + 3 * a];          /* R row-major here: R(a,b) = Rij(b,a) */
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 3; k++) s += Rij[k + 3 * a] * tij[k];
            t[a] = -s;
        }
        DVO_PG_UNROLL
        for (int b = 0; b < 3; b++) {
            Ad[0 * 6 + b] = R[0 * 3 + b]; Ad[1 * 6 + b] = R[1 * 3 + b]; Ad[2 * 6 + b] = R[2 * 3 + b];
            Ad[3 * 6 + 3 + b] = R[0 * 3 + b]; Ad[4 * 6 + 3 + b] = R[1 * 3 + b]; Ad[5 * 6 + 3 + b] = R[2 * 3 + b];
            Ad[3 * 6 + b] = 0.0; Ad[4 * 6 + b] = 0.0; Ad[5 * 6 + b] = 0.0;
            Ad[0 * 6 + 3 + b] = t[1] * R[2 * 3 + b] - t[2] * R[1 * 3 + b];
            Ad[1 * 6 + 3 + b] = t[2] * R[0 * 3 + b] - t[0] * R[2 * 3 + b];
            Ad[2 * 6 + 3 + b] = t[0] * R[1 * 3 + b] - t[1] * R[0 * 3 + b];
        }
        mul6(Jj, Ad, Ji);
        DVO_PG_UNROLL
        for (int k = 0; k < 36; k++) Ji[k] = -Ji[k];
    }
    DVO_PG_UNROLL
    for (int side = 0; side < 2; side++) {
        const double *Ja = side ? Jj : Ji;
        DVO_PG_UNROLL
        for (int a = 0; a < 6; a++) {
            double Arow[6];                        /* row a of J_a^T (w Omega) */
            DVO_PG_UNROLL
            for (int c = 0; c < 6; c++) {
                double s = 0.0;
                DVO_PG_UNROLL
                for (int k = 0; k < 6; k++) s += Ja[k * 6 + a] * (w * E->info[k * 6 + c]);
                Arow[c] = s;
            }
            DVO_PG_UNROLL
            for (int c = 0; c < 6; c++) {
                double s = 0.0;
                DVO_PG_UNROLL
                for (int k = 0; k < 6; k++) s += Arow[k] * Ja[k * 6 + c];
                blk[(side ? kHjj : kHii) + a * 6 + c] = s;
            }
            if (side == 0) {
                DVO_PG_UNROLL
                for (int c = 0; c < 6; c++) {
                    double s = 0.0;
                    DVO_PG_UNROLL
                    for (int k = 0; k < 6; k++) s += Arow[k] * Jj[k * 6 + c];
                    blk[kHij + a * 6 + c] = s;
                }
            }
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 6; k++) s += Arow[k] * r[k];
            blk[(side ? kBj : kBi) + a] = s;
        }
    }
}

/* Node n's record from its incidence list (entries 2 e + side, side 0: n is the edge's i; edge order): the diagonal block and b
 * summed in list order, then the inverse of block + lambda diag(block).  false: the damped block has no Cholesky factor */
DVO_PG_HD bool node_assemble(int n, const int *ptr, const int *inc, const double *blk, double lambda, double *node) {
    double D[36], b[6];
    DVO_PG_UNROLL
    for (int k = 0; k < 36; k++) D[k] = 0.0;
    DVO_PG_UNROLL
    for (int k = 0; k < 6; k++) b[k] = 0.0;
    for (int q = ptr[n]; q < ptr[n + 1]; q++) {
        const double *B = blk + (size_t)(inc[q] >> 1) * kBlk;
        const double *Hnn = B + ((inc[q] & 1) ? kHjj : kHii), *bn = B + ((inc[q] & 1) ? kBj : kBi);
        DVO_PG_UNROLL
        for (int k = 0; k < 36; k++) D[k] += Hnn[k];
        DVO_PG_UNROLL
        for (int k = 0; k < 6; k++) b[k] += bn[k];
    }
    DVO_PG_UNROLL
    for (int k = 0; k < 6; k++) {
        node[kDg + k] = D[k * 7];
        node[kB + k] = b[k];
        D[k * 7] = D[k * 7] + lambda * D[k * 7];
    }
    return inv6_spd(D, node + kMinv);
}

/* (H + lambda diag H) p at node n, matrix-free over its incidence list; node m's 6 doubles of p at p + pstride m, zero at fixed nodes */
DVO_PG_HD void node_apply(int n, const int *ptr, const int *inc, const dvo_graph_edge *E, const double *blk, const double *node, double lambda,
                          const double *p, size_t pstride, double *out) {
    double acc[6];
    DVO_PG_UNROLL
    for (int k = 0; k < 6; k++) acc[k] = 0.0;
    const double *pn = p + pstride * (size_t)n;
    for (int q = ptr[n]; q < ptr[n + 1]; q++) {
        const int e = inc[q] >> 1, side = inc[q] & 1;
        const double *B = blk + (size_t)e * kBlk;
        const double *pm = p + pstride * (size_t)(side ? E[e].i : E[e].j);
        const double *Hnn = B + (side ? kHjj : kHii), *Hx = B + kHij;
        DVO_PG_UNROLL
        for (int r = 0; r < 6; r++) {
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 6; k++) s += Hnn[r * 6 + k] * pn[k];
            DVO_PG_UNROLL
            for (int k = 0; k < 6; k++) s += (side ? Hx[k * 6 + r] : Hx[r * 6 + k]) * pm[k];      /* side 1: H_ij^T */
            acc[r] += s;
        }
    }
    DVO_PG_UNROLL
    for (int k = 0; k < 6; k++) out[k] = acc[k] + (lambda * node[kDg + k]) * pn[k];
}

/* T Exp(x) before the re-orthogonalisation: out = {R Rx, R tx + t} */
DVO_PG_HD void pose_step(const double *P, const double *x, double *out) {
    double Rx[9], tx[3];
    se3_exp(x, Rx, tx);
    DVO_PG_UNROLL
    for (int a = 0; a < 3; a++) {
        DVO_PG_UNROLL
        for (int b = 0; b < 3; b++) {
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 3; k++) s += P[a + 3 * k] * Rx[k + 3 * b];
            out[a + 3 * b] = s;
        }
        double s = 0.0;
        DVO_PG_UNROLL
        for (int k = 0; k < 3; k++) s += P[a + 3 * k] * tx[k];
        out[9 + a] = s + P[9 + a];
    }
}

/* the orthogonal polar factor of X (3 x 3), by the Newton iteration X <- (X + X^-T) / 2 -- what the engine's rotationize computes */
inline void polar3(double *X) {
    for (int it = 0; it < 32; it++) {
        double C[9];
        C[0] = X[4] * X[8] - X[7] * X[5];
        C[1] = X[6] * X[5] - X[3] * X[8];
        C[2] = X[3] * X[7] - X[6] * X[4];
        C[3] = X[7] * X[2] - X[1] * X[8];
        C[4] = X[0] * X[8] - X[6] * X[2];
        C[5] = X[6] * X[1] - X[0] * X[7];
        C[6] = X[1] * X[5] - X[4] * X[2];
        C[7] = X[3] * X[2] - X[0] * X[5];
        C[8] = X[0] * X[4] - X[3] * X[1];
        const double det = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
        if (det == 0.0 || !(det == det)) break;
        const double g = 0.5 / det;
        double nx = 0.0, diff = 0.0;
        for (int k = 0; k < 9; k++) nx += X[k] * X[k];
        for (int k = 0; k < 9; k++) {
            const double xn = 0.5 * X[k] + g * C[k];
            const double d = xn - X[k];
            diff += d * d;
            X[k] = xn;
        }
        if (diff <= 1e-30 * nx) break;
    }
}

inline void params_default(dvo_graph_params *p) {
    p->max_iterations = 50; p->cg_max_iterations = 0;
    p->lambda0 = 1e-4; p->lambda_up = 10.0; p->lambda_down = 0.1; p->lambda_min = 1e-12; p->lambda_max = 1e12;
    p->cg_tol = 1e-6; p->step_tol = 1e-10; p->cost_tol = 1e-14; p->huber_delta = 1.0;
}

inline bool params_ok(const dvo_graph_params *p) {
    if (!p || p->max_iterations < 0 || p->cg_max_iterations < 0) return false;
    const double v[9] = {p->lambda0, p->lambda_up, p->lambda_down, p->lambda_min, p->lambda_max, p->cg_tol, p->step_tol, p->cost_tol, p->huber_delta};
    for (double x : v) if (!is_finite(x)) return false;
    if (!(p->lambda_up > 1.0) || !(p->lambda_down > 0.0 && p->lambda_down < 1.0)) return false;
    return p->lambda0 >= 0.0 && p->lambda_min >= 0.0 && p->lambda_max >= p->lambda_min && p->cg_tol >= 0.0 && p->step_tol >= 0.0 &&
           p->cost_tol >= 0.0;
}

/* what every entry point refuses in a graph: a NULL array, n_nodes < 1, counts above the two maxima, an edge index out of range or
 * i == j, a number that is not finite, an Omega that is not symmetric to 1e-9 relative or has no Cholesky factor, unknown flags, a
 * connected component without a fixed node.  scratch: 2 n_nodes ints */
inline bool graph_ok(int n, const double *poses, const unsigned char *fixed, int ne, const dvo_graph_edge *E, int *scratch) {
    if (n < 1 || n > DVO_GRAPH_MAX_NODES || ne < 0 || ne > DVO_GRAPH_MAX_EDGES || !poses || !fixed || (ne > 0 && !E) || !scratch) return false;
    for (size_t k = 0; k < 12 * (size_t)n; k++) if (!is_finite(poses[k])) return false;
    for (int e = 0; e < ne; e++) {
        const dvo_graph_edge &g = E[e];
        if (g.i < 0 || g.i >= n || g.j < 0 || g.j >= n || g.i == g.j || (g.flags & ~DVO_GRAPH_EDGE_ROBUST)) return false;
        for (int k = 0; k < 9; k++) if (!is_finite(g.R[k])) return false;
        for (int k = 0; k < 3; k++) if (!is_finite(g.t[k])) return false;
        for (int k = 0; k < 36; k++) if (!is_finite(g.info[k])) return false;
        for (int a = 0; a < 6; a++)
            for (int b = a + 1; b < 6; b++) {
                const double x = g.info[a * 6 + b], y = g.info[b * 6 + a], m = fabs(x) > fabs(y) ? fabs(x) : fabs(y);
                if (fabs(x - y) > 1e-9 * m) return false;
            }
        double L[36];
        if (!chol6(g.info, L)) return false;
    }
    int *root = scratch, *has = scratch + n;       /* union-find; has: the component of this root holds a fixed node */
    for (int k = 0; k < n; k++) { root[k] = k; has[k] = 0; }
    for (int e = 0; e < ne; e++) {
        int a = E[e].i, b = E[e].j;
        while (root[a] != a) { root[a] = root[root[a]]; a = root[a]; }
        while (root[b] != b) { root[b] = root[root[b]]; b = root[b]; }
        if (a != b) root[a > b ? a : b] = a > b ? b : a;
    }
    for (int pass = 0; pass < 2; pass++)
        for (int k = 0; k < n; k++) {
            int a = k;
            while (root[a] != a) a = root[a];
            if (pass == 0) { if (fixed[k]) has[a] = 1; }
            else if (!has[a]) return false;
        }
    return true;
}

/* the incidence lists: ptr[n_nodes + 1], inc[2 n_edges]; node n's entries 2 e + side in edge order */
inline void build_csr(int n, int ne, const dvo_graph_edge *E, int *ptr, int *inc) {
    for (int k = 0; k <= n; k++) ptr[k] = 0;
    for (int e = 0; e < ne; e++) { ptr[E[e].i + 1]++; ptr[E[e].j + 1]++; }
    for (int k = 0; k < n; k++) ptr[k + 1] += ptr[k];
    for (int e = 0; e < ne; e++) { inc[ptr[E[e].i]++] = 2 * e; inc[ptr[E[e].j]++] = 2 * e + 1; }
    for (int k = n; k > 0; k--) ptr[k] = ptr[k - 1];
    ptr[0] = 0;
}

/* The whole solver for one graph, every sum in index order.  poses is updated in place (fixed nodes never change); cost_trace (may be
 * NULL with trace_capacity 0) receives cost0 and the cost after every outer iteration, iterations + 1 entries, as far as it has room.
 * kInvalid, nothing written: what params_ok and graph_ok refuse, a NULL report, a negative trace_capacity, a NULL trace with room */
inline int solve_host(const dvo_graph_params *prm, int n, double *poses, const unsigned char *fixed, int ne, const dvo_graph_edge *E,
                      dvo_graph_report *rep, double *trace, int trace_capacity) {
    dvo_graph_params P;
    if (prm) P = *prm; else params_default(&P);
    if (!params_ok(&P) || !rep || trace_capacity < 0 || (trace_capacity > 0 && !trace) || n < 1 || n > DVO_GRAPH_MAX_NODES) return kInvalid;
    std::vector<int> ptr(2 * (size_t)n + 2), inc;
    if (!graph_ok(n, poses, fixed, ne, E, ptr.data())) return kInvalid;
    inc.resize(2 * (size_t)ne);
    build_csr(n, ne, E, ptr.data(), inc.data());
    std::vector<double> blk((size_t)ne * kBlk), node((size_t)n * kNode), x(6 * (size_t)n), r(x.size()), z(x.size()), p(x.size()), Ap(x.size()),
        trial(12 * (size_t)n);
    auto total_cost = [&](const double *Q) {
        double c = 0.0;
        for (int e = 0; e < ne; e++) c += edge_cost(Q, E + e, P.huber_delta);
        return c;
    };
    auto dot = [&](const std::vector<double> &a, const std::vector<double> &b) {
        double s = 0.0;
        for (int k = 0; k < n; k++)
            if (!fixed[k])
                for (int q = 0; q < 6; q++) s += a[6 * (size_t)k + q] * b[6 * (size_t)k + q];
        return s;
    };
    bool any_free = false;
    for (int k = 0; k < n; k++) any_free = any_free || !fixed[k];
    double cost = total_cost(poses), lam = P.lambda0;
    dvo_graph_report R = {cost, cost, lam, 0.0, 0, 0, 0, DVO_GRAPH_MAX_ITERATIONS};
    int nt = 0;
    if (nt < trace_capacity) trace[nt] = cost;
    nt++;
    const int cgmax = P.cg_max_iterations > 0 ? P.cg_max_iterations : 12 * n;
    if (!any_free || ne == 0) R.status = DVO_GRAPH_CONVERGED;
    else if (!is_finite(cost)) R.status = DVO_GRAPH_NUMERIC;
    else for (int it = 0; it < P.max_iterations; it++) {
        R.iterations = it + 1;
        for (int e = 0; e < ne; e++) edge_linearise(poses, E + e, P.huber_delta, blk.data() + (size_t)e * kBlk);
        bool ok = true;
        for (int k = 0; k < n; k++)
            if (!fixed[k] && !node_assemble(k, ptr.data(), inc.data(), blk.data(), lam, node.data() + (size_t)k * kNode)) ok = false;
        double ms = 0.0, tc = 0.0;
        if (ok) {
            for (int k = 0; k < n; k++)
                for (int q = 0; q < 6; q++) {
                    const size_t o = 6 * (size_t)k + q;
                    x[o] = 0.0; r[o] = fixed[k] ? 0.0 : -node[(size_t)k * kNode + kB + q];
                }
            for (int k = 0; k < n; k++) {
                if (fixed[k]) { for (int q = 0; q < 6; q++) z[6 * (size_t)k + q] = 0.0; }
                else mulv6(node.data() + (size_t)k * kNode + kMinv, r.data() + 6 * (size_t)k, z.data() + 6 * (size_t)k);
                for (int q = 0; q < 6; q++) p[6 * (size_t)k + q] = z[6 * (size_t)k + q];
            }
            double rz = dot(r, z);
            const double rz0 = rz;
            int k_cg = 0;
            while (k_cg < cgmax) {
                if (!(rz > 0.0) || sqrt(rz) <= P.cg_tol * sqrt(rz0)) break;
                for (int k = 0; k < n; k++)
                    if (!fixed[k]) node_apply(k, ptr.data(), inc.data(), E, blk.data(), node.data() + (size_t)k * kNode, lam, p.data(), 6, Ap.data() + 6 * (size_t)k);
                const double pAp = dot(p, Ap);
                if (!(pAp > 0.0)) break;
                const double alpha = rz / pAp;
                for (int k = 0; k < n; k++) {
                    if (fixed[k]) continue;
                    double *xk = x.data() + 6 * (size_t)k, *rk = r.data() + 6 * (size_t)k;
                    for (int q = 0; q < 6; q++) { xk[q] = xk[q] + alpha * p[6 * (size_t)k + q]; rk[q] = rk[q] - alpha * Ap[6 * (size_t)k + q]; }
                    mulv6(node.data() + (size_t)k * kNode + kMinv, rk, z.data() + 6 * (size_t)k);
                }
                const double rzn = dot(r, z), beta = rzn / rz;
                for (int k = 0; k < n; k++)
                    if (!fixed[k])
                        for (int q = 0; q < 6; q++) p[6 * (size_t)k + q] = z[6 * (size_t)k + q] + beta * p[6 * (size_t)k + q];
                rz = rzn;
                k_cg++;
            }
            R.cg_iterations += k_cg;
            for (int k = 0; k < n; k++)
                if (!fixed[k])
                    for (int q = 0; q < 6; q++) {
                        const double v = fabs(x[6 * (size_t)k + q]);
                        if (!is_finite(v)) ok = false;
                        else if (v > ms) ms = v;
                    }
        }
        if (ok) {
            for (int k = 0; k < n; k++) {
                double *T = trial.data() + 12 * (size_t)k;
                if (fixed[k]) { for (int q = 0; q < 12; q++) T[q] = poses[12 * (size_t)k + q]; continue; }
                pose_step(poses + 12 * (size_t)k, x.data() + 6 * (size_t)k, T);
                polar3(T);
            }
            tc = total_cost(trial.data());
            if (!is_finite(tc)) ok = false;
        }
        bool stop = false;
        if (ok && tc <= cost) {
            const double dec = cost - tc;
            for (int k = 0; k < n; k++)
                if (!fixed[k]) for (int q = 0; q < 12; q++) poses[12 * (size_t)k + q] = trial[12 * (size_t)k + q];
            cost = tc;
            R.accepted++;
            R.max_step = ms;
            lam = lam * P.lambda_down > P.lambda_min ? lam * P.lambda_down : P.lambda_min;
            if (ms < P.step_tol || (P.cost_tol > 0.0 && dec <= P.cost_tol * cost)) { R.status = DVO_GRAPH_CONVERGED; stop = true; }
        } else if (lam >= P.lambda_max) {          /* a finite trial that no damping improves: the cost is at its rounding floor */
            R.status = ok ? DVO_GRAPH_CONVERGED : DVO_GRAPH_NUMERIC; stop = true;
        } else {
            lam = lam * P.lambda_up < P.lambda_max ? lam * P.lambda_up : P.lambda_max;
        }
        if (nt < trace_capacity) trace[nt] = cost;
        nt++;
        if (stop) break;
    }
    R.cost = cost;
    R.lambda = lam;
    *rep = R;
    return kOk;
}

/* ---- marginal covariances of the poses (include/dvo_amd.h, "pose graphs": dvo_graph_marginals_host is marginals_host() below) ----
 * The joint covariance of m listed nodes is the matching block of H^-1, H the UNDAMPED Gauss-Newton matrix over the free nodes at the
 * given poses, in the solver's convention (tangent order [translation, rotation], right perturbation, the truncated Jr^-1):
 *   1. every edge is linearised at the poses with edge_linearise, Huber weights at the current residuals with huber_delta;
 *   2. every free node is assembled with node_assemble at lambda = 0; a block without a Cholesky factor: DVO_GRAPH_NUMERIC, cov all zero;
 *   3. per listed node c = nodes[b] and k in 0..5 the column H x = e(c,k) is solved by the PCG loop of solve_host -- x = 0, r = e,
 *      z = Minv r, p = z; stop at sqrt(rz) <= cg_tol sqrt(rz0), after cg_max_iterations iterations (0: 12 n_nodes) or at pAp <= 0;
 *      node_apply with lambda = 0; fixed nodes stay zero.  A listed fixed node: x = 0, no iterations, residual 0;
 *   4. M[6a + q][6b + k] = x(nodes[b], k) at node nodes[a], component q; cov[u][v] = 0.5 (M[u][v] + M[v][u]).
 * So cov is exactly symmetric, and its block (a, b) depends on the graph, nodes[a] and nodes[b] alone -- not on m, the other listed
 * nodes or their order.  A column ends (marginal_column_end) with residual sqrt(rz) / sqrt(rz0) and the status DVO_GRAPH_NUMERIC if the
 * residual or a component of x is not finite, else DVO_GRAPH_CONVERGED if it met cg_tol, else DVO_GRAPH_MAX_ITERATIONS (the cap, or
 * pAp <= 0; the column is what the loop held).  The report holds the worst residual and status (NUMERIC over MAX_ITERATIONS over
 * CONVERGED), the iterations in total and of the longest column.  Of the parameters only huber_delta, cg_tol and cg_max_iterations are
 * used; the whole struct must pass params_ok all the same.
 * Unit: cov inherits the scale of the edges' information: the inverse of Omega's.  With edges from dvo_graph_information that scale is
 * the distance-transform residual's: relative and uncalibrated. */
DVO_PG_HD void marginal_column_end(double rz, double rz0, double cg_tol, bool x_finite, double *residual, int *status) {
    const double res = sqrt(rz) / sqrt(rz0);
    *residual = res;
    if (!is_finite(res) || !x_finite) *status = DVO_GRAPH_NUMERIC;
    else *status = sqrt(rz) <= cg_tol * sqrt(rz0) ? DVO_GRAPH_CONVERGED : DVO_GRAPH_MAX_ITERATIONS;
}

/* what a query may list: 1 .. DVO_GRAPH_MARGINAL_MAX_NODES nodes of the graph, none twice */
inline bool marginal_query_ok(int n, int m, const int *nodes) {
    if (n < 1 || n > DVO_GRAPH_MAX_NODES || m < 1 || m > DVO_GRAPH_MARGINAL_MAX_NODES || !nodes) return false;
    for (int a = 0; a < m; a++) {
        if (nodes[a] < 0 || nodes[a] >= n) return false;
        for (int b = 0; b < a; b++) if (nodes[b] == nodes[a]) return false;
    }
    return true;
}

/* cov from the columns: M (w x w row-major, w = 6 m) -> cov = (M + M^T) / 2 */
inline void marginal_symmetrise(int m, const double *M, double *cov) {
    const size_t w = 6 * (size_t)m;
    for (size_t u = 0; u < w; u++)
        for (size_t v = 0; v < w; v++) cov[u * w + v] = 0.5 * (M[u * w + v] + M[v * w + u]);
}

/* kInvalid, nothing written: what solve_host refuses in parameters and graph, m outside [1, DVO_GRAPH_MARGINAL_MAX_NODES], a NULL nodes,
 * cov or report, a node out of range or listed twice.  cov: (6 m)^2 doubles, row-major */
inline int marginals_host(const dvo_graph_params *prm, int n, const double *poses, const unsigned char *fixed, int ne, const dvo_graph_edge *E,
                          int m, const int *nodes, double *cov, dvo_graph_marginal_report *rep) {
    dvo_graph_params P;
    if (prm) P = *prm; else params_default(&P);
    if (!params_ok(&P) || !marginal_query_ok(n, m, nodes) || !cov || !rep) return kInvalid;
    std::vector<int> ptr(2 * (size_t)n + 2), inc;
    if (!graph_ok(n, poses, fixed, ne, E, ptr.data())) return kInvalid;
    inc.resize(2 * (size_t)ne);
    build_csr(n, ne, E, ptr.data(), inc.data());
    const size_t w = 6 * (size_t)m;
    std::vector<double> blk((size_t)ne * kBlk), node((size_t)n * kNode), x(6 * (size_t)n), r(x.size()), z(x.size()), p(x.size()), Ap(x.size()),
        M(w * w, 0.0);
    auto dot = [&](const std::vector<double> &a, const std::vector<double> &b) {
        double s = 0.0;
        for (int k = 0; k < n; k++)
            if (!fixed[k])
                for (int q = 0; q < 6; q++) s += a[6 * (size_t)k + q] * b[6 * (size_t)k + q];
        return s;
    };
    dvo_graph_marginal_report R = {0.0, 0, 0, DVO_GRAPH_CONVERGED};
    for (int e = 0; e < ne; e++) edge_linearise(poses, E + e, P.huber_delta, blk.data() + (size_t)e * kBlk);
    bool ok = true;
    for (int k = 0; k < n; k++)
        if (!fixed[k] && !node_assemble(k, ptr.data(), inc.data(), blk.data(), 0.0, node.data() + (size_t)k * kNode)) ok = false;
    if (!ok) {
        for (size_t u = 0; u < w * w; u++) cov[u] = 0.0;
        R.status = DVO_GRAPH_NUMERIC;
        *rep = R;
        return kOk;
    }
    const int cgmax = P.cg_max_iterations > 0 ? P.cg_max_iterations : 12 * n;
    for (int b = 0; b < m; b++)
        for (int col = 0; col < 6; col++) {
            const int c = nodes[b];
            for (size_t o = 0; o < x.size(); o++) { x[o] = 0.0; r[o] = 0.0; }
            int k_cg = 0, status = DVO_GRAPH_CONVERGED;
            double residual = 0.0;
            if (!fixed[c]) {
                r[6 * (size_t)c + col] = 1.0;
                for (int k = 0; k < n; k++) {
                    if (fixed[k]) { for (int q = 0; q < 6; q++) z[6 * (size_t)k + q] = 0.0; }
                    else mulv6(node.data() + (size_t)k * kNode + kMinv, r.data() + 6 * (size_t)k, z.data() + 6 * (size_t)k);
                    for (int q = 0; q < 6; q++) p[6 * (size_t)k + q] = z[6 * (size_t)k + q];
                }
                double rz = dot(r, z);
                const double rz0 = rz;
                while (k_cg < cgmax) {
                    if (!(rz > 0.0) || sqrt(rz) <= P.cg_tol * sqrt(rz0)) break;
                    for (int k = 0; k < n; k++)
                        if (!fixed[k]) node_apply(k, ptr.data(), inc.data(), E, blk.data(), node.data() + (size_t)k * kNode, 0.0, p.data(), 6, Ap.data() + 6 * (size_t)k);
                    const double pAp = dot(p, Ap);
                    if (!(pAp > 0.0)) break;
                    const double alpha = rz / pAp;
                    for (int k = 0; k < n; k++) {
                        if (fixed[k]) continue;
                        double *xk = x.data() + 6 * (size_t)k, *rk = r.data() + 6 * (size_t)k;
                        for (int q = 0; q < 6; q++) { xk[q] = xk[q] + alpha * p[6 * (size_t)k + q]; rk[q] = rk[q] - alpha * Ap[6 * (size_t)k + q]; }
                        mulv6(node.data() + (size_t)k * kNode + kMinv, rk, z.data() + 6 * (size_t)k);
                    }
                    const double rzn = dot(r, z), beta = rzn / rz;
                    for (int k = 0; k < n; k++)
                        if (!fixed[k])
                            for (int q = 0; q < 6; q++) p[6 * (size_t)k + q] = z[6 * (size_t)k + q] + beta * p[6 * (size_t)k + q];
                    rz = rzn;
                    k_cg++;
                }
                bool finite = true;
                for (int k = 0; k < n; k++)
                    if (!fixed[k])
                        for (int q = 0; q < 6; q++) finite = finite && is_finite(x[6 * (size_t)k + q]);
                marginal_column_end(rz, rz0, P.cg_tol, finite, &residual, &status);
            }
            for (int a = 0; a < m; a++)
                for (int q = 0; q < 6; q++) M[(6 * (size_t)a + q) * w + 6 * (size_t)b + col] = x[6 * (size_t)nodes[a] + q];
            R.cg_iterations += k_cg;
            if (k_cg > R.cg_iterations_max) R.cg_iterations_max = k_cg;
            if (status > R.status) R.status = status;
            if (residual > R.worst_residual || !is_finite(residual)) R.worst_residual = residual;      /* so a NaN stays */
        }
    marginal_symmetrise(m, M.data(), cov);
    *rep = R;
    return kOk;
}

/* The residual and the Jacobians of one edge at the poses Pi, Pj: r = Log(Z^-1 T_i^-1 T_j), J_j = Jr^-1(r), J_i = -Jr^-1(r) Ad(T_j^-1 T_i)
 * (6 x 6 row-major each), by the arithmetic of edge_linearise.  Host only: the gate below is its one user.  (edge_linearise keeps its own
 * copy of these lines: the device kernels compile it as one piece, and its text is what the solver's results are pinned to) */
inline void edge_jacobians(const double *Pi, const double *Pj, const dvo_graph_edge *E, double *r, double *Ji, double *Jj) {
    double Rij[9], tij[3];
    edge_residual(Pi, Pj, E, r, Rij, tij);
    jr_inv(r, Jj);
    {   /* Ad(T_j^-1 T_i) = [[R, t^ R], [0, R]] with R = Rij^T, t = -Rij^T tij */
        double Ad[36], R[9], t[3];
        DVO_PG_UNROLL
        for (int a = 0; a < 3; a++) {
            DVO_PG_UNROLL
            for (int b = 0; b < 3; b++) R[a * 3 + b] = Rij[b + 3 * a];          /* R row-major here: R(a,b) = Rij(b,a) */
            double s = 0.0;
            DVO_PG_UNROLL
            for (int k = 0; k < 3; k++) s += Rij[k + 3 * a] * tij[k];
            t[a] = -s;
        }
        DVO_PG_UNROLL
        for (int b = 0; b < 3; b++) {
            Ad[0 * 6 + b] = R[0 * 3 + b]; Ad[1 * 6 + b] = R[1 * 3 + b]; Ad[2 * 6 + b] = R[2 * 3 + b];
            Ad[3 * 6 + 3 + b] = R[0 * 3 + b]; Ad[4 * 6 + 3 + b] = R[1 * 3 + b]; Ad[5 * 6 + 3 + b] = R[2 * 3 + b];
            Ad[3 * 6 + b] = 0.0; Ad[4 * 6 + b] = 0.0; Ad[5 * 6 + b] = 0.0;
            Ad[0 * 6 + 3 + b] = t[1] * R[2 * 3 + b] - t[2] * R[1 * 3 + b];
            Ad[1 * 6 + 3 + b] = t[2] * R[0 * 3 + b] - t[0] * R[2 * 3 + b];
            Ad[2 * 6 + 3 + b] = t[0] * R[1 * 3 + b] - t[1] * R[0 * 3 + b];
        }
        mul6(Jj, Ad, Ji);
        DVO_PG_UNROLL
        for (int k = 0; k < 36; k++) Ji[k] = -Ji[k];
    }
}

/* The gate: is the measurement of `E` between two nodes compatible with what is believed about them?  r, J_i, J_j by edge_jacobians at
 * the poses; S = [J_i J_j] cov [J_i J_j]^T + Omega^-1 (cov: the joint 12 x 12 of (i, j), row-major, NULL = zero; every sum in index order
 * from 0, the product with cov first; Omega^-1 by inv6_spd); chi2 = r^T S^-1 r (S^-1 by inv6_spd).  The robust flag plays no part.
 * r6, S36, chi2: any may be NULL.  kInvalid, nothing written: a NULL pose or edge, a number that is not finite, an Omega or an S
 * without a Cholesky factor */
inline int edge_chi2(const double *Pi, const double *Pj, const double *cov144, const dvo_graph_edge *E, double *r6, double *S36, double *chi2) {
    if (!Pi || !Pj || !E) return kInvalid;
    for (int k = 0; k < 12; k++) if (!is_finite(Pi[k]) || !is_finite(Pj[k])) return kInvalid;
    for (int k = 0; k < 9; k++) if (!is_finite(E->R[k])) return kInvalid;
    for (int k = 0; k < 3; k++) if (!is_finite(E->t[k])) return kInvalid;
    for (int k = 0; k < 36; k++) if (!is_finite(E->info[k])) return kInvalid;
    if (cov144)
        for (int k = 0; k < 144; k++) if (!is_finite(cov144[k])) return kInvalid;
    double S[36], Sinv[36], r[6], Ji[36], Jj[36];
    if (!inv6_spd(E->info, S)) return kInvalid;
    edge_jacobians(Pi, Pj, E, r, Ji, Jj);
    if (cov144) {
        auto J = [&](int a, int k) { return k < 6 ? Ji[a * 6 + k] : Jj[a * 6 + k - 6]; };
        double T[72];
        for (int a = 0; a < 6; a++)
            for (int c = 0; c < 12; c++) {
                double s = 0.0;
                for (int k = 0; k < 12; k++) s += J(a, k) * cov144[k * 12 + c];
                T[a * 12 + c] = s;
            }
        for (int a = 0; a < 6; a++)
            for (int b = 0; b < 6; b++) {
                double s = 0.0;
                for (int k = 0; k < 12; k++) s += T[a * 12 + k] * J(b, k);
                S[a * 6 + b] = s + S[a * 6 + b];
            }
    }
    if (!inv6_spd(S, Sinv)) return kInvalid;
    const double c2 = edge_s2(Sinv, r);
    if (!is_finite(c2)) return kInvalid;
    if (r6) for (int k = 0; k < 6; k++) r6[k] = r[k];
    if (S36) for (int k = 0; k < 36; k++) S36[k] = S[k];
    if (chi2) *chi2 = c2;
    return kOk;
}

}  // namespace dvo_pg

#endif
