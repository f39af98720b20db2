/*
 * dvo_pose_graph.hip -- pose-graph optimisation on the device (include/dvo_amd.h, "pose graphs"; host side dvo_capi_graph.cpp; the
 * definition is dvo_pose_graph.h, whose per-edge and per-node functions this kernel shares with the host solver).  ONE launch per
 * dvo_graph_solve (DVO_GRAPH_LAUNCHES): workgroup b runs the whole Levenberg-Marquardt loop of listed graph b.  The marginal covariances
 * (dvo_graph_marginals, DVO_GRAPH_MARGINAL_LAUNCHES launches) follow the solve kernel below and share its building blocks.
 *
 *   edges across threads   linearisation (edge_linearise -> the graph's blocks in HBM) and the robust cost
 *   nodes across threads   assembly (node_assemble walks the node's incidence list in edge order: no atomics), the block-Jacobi
 *                          preconditioner, the matrix-free operator (node_apply), the CG updates, the trial poses
 *
 * Thread t owns edges and nodes t, t + 256, ...  A sum over edges or nodes is the thread's own partial in index order, then the 64
 * lanes of a wave by a butterfly of shuffles, then the four waves in wave order through LDS (block_sum).  Every thread reads the
 * same total, so every branch of the loop is uniform.  Nothing depends on gridDim, and blockIdx only selects the graph: a graph's
 * result is bit-identical run to run and whatever else the batch holds.
 *
 * The five CG vectors (x, r, z, p, A p: 240 bytes per node) live in LDS when the graph has at most SolveArgs.lds_nodes nodes, else
 * in the graph's workspace in HBM; per-edge blocks, per-node records and trial poses are always in HBM (L2-resident at the sizes
 * of interest).  Three barriers per CG iteration: two sums and the hand-over of p.
 *
 * Bounds: thread loops run over e < ne and n < nn of the graph's own descriptor; an incidence entry is below 2 ne and an edge's
 * nodes are below nn (validated by graph_ok before a graph is staged); the trace is written below trace_cap; every loop is capped
 * (max_iterations, cg_max_iterations or 12 nn, 32 polar steps).
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_launch.h"
#include "dvo_pose_graph_launch.h"

namespace dvo {

namespace {
using namespace dvo_pg;
constexpr int PG_BLOCK = kBlock, PG_WAVES = PG_BLOCK / 64;
/* on a call of the definition's per-edge and per-node functions that more than one kernel makes: inlined at every site, as it is where
 * a function has one caller -- its arrays stay in registers (out of line they go through scratch memory) */
#define PG_INLINE [[clang::always_inline]]

/* the workgroup's sum of v: lanes, then waves in wave order; one barrier (the slots alternate, so the next sum's barrier is what
 * separates this sum's reads from the writes of the one after it) */
DVO_DEV double block_sum(double v, double (*slot)[PG_WAVES], int &ph) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) slot[ph][threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[ph][0];
#pragma unroll
    for (int w = 1; w < PG_WAVES; w++) s += slot[ph][w];
    ph ^= 1;
    return s;
}
DVO_DEV double block_max(double v, double (*slot)[PG_WAVES], int &ph) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) slot[ph][threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[ph][0];
#pragma unroll
    for (int w = 1; w < PG_WAVES; w++) s = fmax(s, slot[ph][w]);
    ph ^= 1;
    return s;
}

/* a graph set since it last went up: its blob (poses | edges | ptr | inc | fixed, each padded to 8 bytes) -> the resident arrays.
 * The caller's barrier follows */
DVO_DEV void stage_graph(const unsigned char *src, int nn, int ne, double *poses, dvo_graph_edge *E, int *ptr, int *inc, unsigned char *fixed) {
    const int tid = threadIdx.x;
    const double *sp = reinterpret_cast<const double *>(src);
    for (int k = tid; k < 12 * nn; k += PG_BLOCK) poses[k] = sp[k];
    src += 96 * (size_t)nn;
    const double *se = reinterpret_cast<const double *>(src);
    double *de = reinterpret_cast<double *>(E);
    const int ew = (int)(sizeof(dvo_graph_edge) / 8) * ne;
    for (int k = tid; k < ew; k += PG_BLOCK) de[k] = se[k];
    src += sizeof(dvo_graph_edge) * (size_t)ne;
    const int *si = reinterpret_cast<const int *>(src);
    for (int k = tid; k <= nn; k += PG_BLOCK) ptr[k] = si[k];
    src += pad8(4 * ((size_t)nn + 1));
    si = reinterpret_cast<const int *>(src);
    for (int k = tid; k < 2 * ne; k += PG_BLOCK) inc[k] = si[k];
    src += pad8(8 * (size_t)ne);
    for (int k = tid; k < nn; k += PG_BLOCK) fixed[k] = src[k];
}
}  // namespace

__global__ void __launch_bounds__(PG_BLOCK)
pose_graph_solve_kernel(SolveArgs a) {
    __shared__ double slot[2][PG_WAVES];
    extern __shared__ __attribute__((aligned(16))) double pg_lds[];
    const DeviceGraph g = a.graphs[blockIdx.x];
    const int tid = threadIdx.x, nn = g.n, ne = g.ne;
    double *poses = a.poses + 12 * (size_t)g.node_off;
    unsigned char *fixed = a.fixed + g.node_off;
    dvo_graph_edge *E = a.edges + g.edge_off;
    int *ptr = a.ptr + g.ptr_off, *inc = a.inc + 2 * (size_t)g.edge_off;
    double *blk = a.blk + (size_t)kBlk * g.edge_off, *node = a.node + (size_t)kNodeWs * g.node_off;
    dvo_graph_report *rep = reinterpret_cast<dvo_graph_report *>(a.out + g.out_off);
    double *trace = reinterpret_cast<double *>(a.out + g.out_off + sizeof(dvo_graph_report));
    double *pose_out = trace + a.trace_cap;
    const dvo_graph_params P = a.prm;
    int ph = 0;

    if (g.blob_off >= 0) stage_graph(a.upload + g.blob_off, nn, ne, poses, E, ptr, inc, fixed);      /* set since its last solve: upload -> resident */
    __syncthreads();

    /* the CG vectors: 6 doubles per node each */
    const bool in_lds = nn <= a.lds_nodes;
    /* vector v (0: x, 1: r, 2: z, 3: p, 4: A p) of node n: in LDS one array per vector, in the workspace beside the node's record */
    auto vec = [&](int v, int n) -> double * {
        if (in_lds) return pg_lds + 6 * ((size_t)v * nn + n);
        return node + (size_t)kNodeWs * n + kWsVec + 6 * v;
    };

    auto total_cost = [&](const double *Q, size_t stride, size_t off) {
        double c = 0.0;
        for (int e = tid; e < ne; e += PG_BLOCK) {
            const dvo_graph_edge *Ee = E + e;
            double r[6];
            edge_residual(Q + stride * Ee->i + off, Q + stride * Ee->j + off, Ee, r, nullptr, nullptr);
            c += edge_rho(edge_s2(Ee->info, r), Ee->flags, P.huber_delta);
        }
        return block_sum(c, slot, ph);
    };

    double nfree = 0.0;
    for (int n = tid; n < nn; n += PG_BLOCK) nfree += fixed[n] ? 0.0 : 1.0;
    nfree = block_sum(nfree, slot, ph);
    double cost = total_cost(poses, 12, 0), lam = P.lambda0;
    const double cost0 = cost;
    double max_step = 0.0;
    int iterations = 0, accepted = 0, cg_total = 0, status = DVO_GRAPH_MAX_ITERATIONS, nt = 0;
    if (tid == 0 && nt < a.trace_cap) trace[nt] = cost;
    nt++;
    const int cgmax = P.cg_max_iterations > 0 ? P.cg_max_iterations : 12 * nn;

    if (nfree == 0.0 || ne == 0) status = DVO_GRAPH_CONVERGED;
    else if (!is_finite(cost)) status = DVO_GRAPH_NUMERIC;
    else for (int it = 0; it < P.max_iterations; it++) {
        iterations = it + 1;
        __syncthreads();                           /* the poses of the last accepted step */
        for (int e = tid; e < ne; e += PG_BLOCK) {
            /* the edge's poses stand where edge_linearise expects them: P + 12 i */
            PG_INLINE edge_linearise(poses, E + e, P.huber_delta, blk + (size_t)kBlk * e);
        }
        __syncthreads();
        /* assembly, preconditioner, CG start */
        double bad = 0.0, rz = 0.0;
        for (int n = tid; n < nn; n += PG_BLOCK) {
            double *x = vec(0, n), *r = vec(1, n), *z = vec(2, n), *p = vec(3, n);
            if (fixed[n]) {
#pragma unroll
                for (int k = 0; k < 6; k++) { x[k] = 0.0; r[k] = 0.0; z[k] = 0.0; p[k] = 0.0; }
                continue;
            }
            double *rec = node + (size_t)kNodeWs * n;
            bool factored;
            PG_INLINE factored = node_assemble(n, ptr, inc, blk, lam, rec);
            if (!factored) { bad += 1.0; continue; }
            double rr[6], zz[6];
#pragma unroll
            for (int k = 0; k < 6; k++) rr[k] = -rec[kB + k];
            mulv6(rec + kMinv, rr, zz);
#pragma unroll
            for (int k = 0; k < 6; k++) { x[k] = 0.0; r[k] = rr[k]; z[k] = zz[k]; p[k] = zz[k]; rz += rr[k] * zz[k]; }
        }
        bad = block_sum(bad, slot, ph);
        bool ok = bad == 0.0;
        double ms = 0.0, tc = 0.0;
        if (ok) {
            rz = block_sum(rz, slot, ph);          /* its barrier also hands p over */
            const double rz0 = rz;
            int k_cg = 0;
            while (k_cg < cgmax) {
                if (!(rz > 0.0) || sqrt(rz) <= P.cg_tol * sqrt(rz0)) break;
                double pAp = 0.0;
                for (int n = tid; n < nn; n += PG_BLOCK) {
                    if (fixed[n]) continue;
                    double Ap[6];
                    const double *pn = vec(3, n);
                    node_apply(n, ptr, inc, E, blk, node + (size_t)kNodeWs * n, lam, vec(3, 0), in_lds ? 6 : kNodeWs, Ap);
                    double *An = vec(4, n);
#pragma unroll
                    for (int k = 0; k < 6; k++) { An[k] = Ap[k]; pAp += pn[k] * Ap[k]; }
                }
                pAp = block_sum(pAp, slot, ph);
                if (!(pAp > 0.0)) break;
                const double alpha = rz / pAp;
                double rzn = 0.0;
                for (int n = tid; n < nn; n += PG_BLOCK) {
                    if (fixed[n]) continue;
                    double *x = vec(0, n), *r = vec(1, n), *z = vec(2, n);
                    const double *p = vec(3, n), *An = vec(4, n);
                    double rr[6], zz[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) { x[k] = x[k] + alpha * p[k]; rr[k] = r[k] - alpha * An[k]; r[k] = rr[k]; }
                    mulv6(node + (size_t)kNodeWs * n + kMinv, rr, zz);
#pragma unroll
                    for (int k = 0; k < 6; k++) { z[k] = zz[k]; rzn += rr[k] * zz[k]; }
                }
                rzn = block_sum(rzn, slot, ph);
                const double beta = rzn / rz;
                for (int n = tid; n < nn; n += PG_BLOCK) {
                    if (fixed[n]) continue;
                    double *p = vec(3, n);
                    const double *z = vec(2, n);
#pragma unroll
                    for (int k = 0; k < 6; k++) p[k] = z[k] + beta * p[k];
                }
                __syncthreads();                   /* p of every node before the next operator */
                rz = rzn;
                k_cg++;
            }
            cg_total += k_cg;
            double nonfinite = 0.0;
            for (int n = tid; n < nn; n += PG_BLOCK) {
                if (fixed[n]) continue;
                const double *x = vec(0, n);
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const double v = fabs(x[k]);
                    if (!is_finite(v)) nonfinite += 1.0;
                    else if (v > ms) ms = v;
                }
            }
            ms = block_max(ms, slot, ph);
            nonfinite = block_sum(nonfinite, slot, ph);
            if (nonfinite != 0.0) ok = false;
        }
        if (ok) {
            for (int n = tid; n < nn; n += PG_BLOCK) {
                double *T = node + (size_t)kNodeWs * n + kWsTrial;
                const double *Pn = poses + 12 * (size_t)n;
                if (fixed[n]) {
#pragma unroll
                    for (int k = 0; k < 12; k++) T[k] = Pn[k];
                    continue;
                }
                double Tn[12], xn[6];
                const double *x = vec(0, n);
#pragma unroll
                for (int k = 0; k < 6; k++) xn[k] = x[k];
                pose_step(Pn, xn, Tn);
                rotationize(Tn);
#pragma unroll
                for (int k = 0; k < 12; k++) T[k] = Tn[k];
            }
            __syncthreads();
            tc = total_cost(node, kNodeWs, kWsTrial);
            if (!is_finite(tc)) ok = false;
        }
        bool stop = false;
        if (ok && tc <= cost) {
            const double dec = cost - tc;
            for (int n = tid; n < nn; n += PG_BLOCK) {
                if (fixed[n]) continue;
                const double *T = node + (size_t)kNodeWs * n + kWsTrial;
#pragma unroll
                for (int k = 0; k < 12; k++) poses[12 * (size_t)n + k] = T[k];
            }
            cost = tc;
            accepted++;
            max_step = ms;
            lam = lam * P.lambda_down > P.lambda_min ? lam * P.lambda_down : P.lambda_min;
            if (ms < P.step_tol || (P.cost_tol > 0.0 && dec <= P.cost_tol * cost)) { status = DVO_GRAPH_CONVERGED; stop = true; }
        } else if (lam >= P.lambda_max) {
            status = ok ? DVO_GRAPH_CONVERGED : DVO_GRAPH_NUMERIC; stop = true;
        } else {
            lam = lam * P.lambda_up < P.lambda_max ? lam * P.lambda_up : P.lambda_max;
        }
        if (tid == 0 && nt < a.trace_cap) trace[nt] = cost;
        nt++;
        if (stop) break;
    }
    __syncthreads();
    for (int k = tid; k < 12 * nn; k += PG_BLOCK) pose_out[k] = poses[k];
    for (int k = nt + tid; k < a.trace_cap; k += PG_BLOCK) trace[k] = 0.0;
    if (tid == 0) {
        rep->cost0 = cost0; rep->cost = cost; rep->lambda = lam; rep->max_step = max_step;
        rep->iterations = iterations; rep->accepted = accepted; rep->cg_iterations = cg_total; rep->status = status;
    }
}

/* ---- marginal covariances (dvo_graph_marginals; the definition is marginals_host of dvo_pose_graph.h) ----
 * TWO launches.  prepare: workgroup b stages listed graph b where due, linearises its edges at the resident poses, assembles its free
 * nodes at lambda = 0 (the records and blocks in the graph's workspace, which a solve rewrites before it reads) and writes the graph's
 * flag.  columns: workgroup (b, node, k) solves H x = e(node, k) with the CG body of the solve kernel -- the same partials, the same
 * block_sum -- its five vectors in LDS up to lds_nodes nodes, else in its own slice of MarginalArgs.ws, and writes the m blocks of its
 * column.  blockIdx only selects the column, nothing depends on gridDim, no atomics: a column is bit-identical whatever the batch and
 * the query around it.  The poses are only read.
 * Bounds: as the solve kernel's; a listed node is below nn (marginal_query_ok on the host); a column writes 6 m + 2 doubles at its own
 * offset; the CG loop is capped by cg_max_iterations or 12 nn. */
__global__ void __launch_bounds__(PG_BLOCK)
pose_graph_marginal_prepare_kernel(MarginalArgs m) {
    __shared__ double slot[2][PG_WAVES];
    const SolveArgs &a = m.s;
    const DeviceGraph g = a.graphs[blockIdx.x];
    const int tid = threadIdx.x, nn = g.n, ne = g.ne;
    double *poses = a.poses + 12 * (size_t)g.node_off;
    unsigned char *fixed = a.fixed + g.node_off;
    dvo_graph_edge *E = a.edges + g.edge_off;
    int *ptr = a.ptr + g.ptr_off, *inc = a.inc + 2 * (size_t)g.edge_off;
    double *blk = a.blk + (size_t)kBlk * g.edge_off, *node = a.node + (size_t)kNodeWs * g.node_off;
    int ph = 0;
    if (g.blob_off >= 0) stage_graph(a.upload + g.blob_off, nn, ne, poses, E, ptr, inc, fixed);
    __syncthreads();
    for (int e = tid; e < ne; e += PG_BLOCK) PG_INLINE edge_linearise(poses, E + e, a.prm.huber_delta, blk + (size_t)kBlk * e);
    __syncthreads();
    double bad = 0.0;
    for (int n = tid; n < nn; n += PG_BLOCK) {
        if (fixed[n]) continue;
        bool factored;
        PG_INLINE factored = node_assemble(n, ptr, inc, blk, 0.0, node + (size_t)kNodeWs * n);
        if (!factored) bad += 1.0;
    }
    bad = block_sum(bad, slot, ph);
    if (tid == 0) reinterpret_cast<int *>(a.out)[blockIdx.x] = bad != 0.0 ? 1 : 0;
}

__global__ void __launch_bounds__(PG_BLOCK)
pose_graph_marginal_columns_kernel(MarginalArgs m) {
    __shared__ double slot[2][PG_WAVES];
    extern __shared__ __attribute__((aligned(16))) double pg_lds[];
    const SolveArgs &a = m.s;
    const int cols = 6 * m.m, gi = blockIdx.x / cols, col = blockIdx.x % cols, kc = col % 6;
    const int *listed = m.nodes + (size_t)gi * m.m;
    const int c = listed[col / 6];
    const DeviceGraph g = a.graphs[gi];
    const int tid = threadIdx.x, nn = g.n;
    const unsigned char *fixed = a.fixed + g.node_off;
    const dvo_graph_edge *E = a.edges + g.edge_off;
    const int *ptr = a.ptr + g.ptr_off, *inc = a.inc + 2 * (size_t)g.edge_off;
    const double *blk = a.blk + (size_t)kBlk * g.edge_off, *node = a.node + (size_t)kNodeWs * g.node_off;
    double *out = reinterpret_cast<double *>(a.out + g.out_off) + (size_t)col * (cols + 2);
    const bool bad = reinterpret_cast<const int *>(a.out)[gi] != 0;
    const dvo_graph_params P = a.prm;
    int ph = 0;

    const bool in_lds = nn <= a.lds_nodes;
    double *ws = in_lds ? nullptr : m.ws + m.ws_off[gi] + (size_t)kMargVec * nn * col;
    /* vector v (0: x, 1: r, 2: z, 3: p, 4: A p) of node n: in LDS one array per vector, in the workspace 30 doubles per node */
    auto vec = [&](int v, int n) -> double * {
        if (in_lds) return pg_lds + 6 * ((size_t)v * nn + n);
        return ws + (size_t)kMargVec * n + 6 * v;
    };

    int k_cg = 0, status = bad ? DVO_GRAPH_NUMERIC : DVO_GRAPH_CONVERGED;
    double residual = 0.0;
    const bool solve = !bad && !fixed[c];          /* uniform; a listed fixed node: x = 0, no iterations */
    if (solve) {
        double rz = 0.0;
        for (int n = tid; n < nn; n += PG_BLOCK) {
            double *x = vec(0, n), *r = vec(1, n), *z = vec(2, n), *p = vec(3, n);
            if (fixed[n]) {
#pragma unroll
                for (int k = 0; k < 6; k++) { x[k] = 0.0; r[k] = 0.0; z[k] = 0.0; p[k] = 0.0; }
                continue;
            }
            double rr[6], zz[6];
#pragma unroll
            for (int k = 0; k < 6; k++) rr[k] = (n == c && k == kc) ? 1.0 : 0.0;
            mulv6(node + (size_t)kNodeWs * n + kMinv, rr, zz);
#pragma unroll
            for (int k = 0; k < 6; k++) { x[k] = 0.0; r[k] = rr[k]; z[k] = zz[k]; p[k] = zz[k]; rz += rr[k] * zz[k]; }
        }
        rz = block_sum(rz, slot, ph);              /* its barrier also hands p over */
        const double rz0 = rz;
        const int cgmax = P.cg_max_iterations > 0 ? P.cg_max_iterations : 12 * nn;
        while (k_cg < cgmax) {
            if (!(rz > 0.0) || sqrt(rz) <= P.cg_tol * sqrt(rz0)) break;
            double pAp = 0.0;
            for (int n = tid; n < nn; n += PG_BLOCK) {
                if (fixed[n]) continue;
                double Ap[6];
                const double *pn = vec(3, n);
                node_apply(n, ptr, inc, E, blk, node + (size_t)kNodeWs * n, 0.0, vec(3, 0), in_lds ? 6 : kMargVec, Ap);
                double *An = vec(4, n);
#pragma unroll
                for (int k = 0; k < 6; k++) { An[k] = Ap[k]; pAp += pn[k] * Ap[k]; }
            }
            pAp = block_sum(pAp, slot, ph);
            if (!(pAp > 0.0)) break;
            const double alpha = rz / pAp;
            double rzn = 0.0;
            for (int n = tid; n < nn; n += PG_BLOCK) {
                if (fixed[n]) continue;
                double *x = vec(0, n), *r = vec(1, n), *z = vec(2, n);
                const double *p = vec(3, n), *An = vec(4, n);
                double rr[6], zz[6];
#pragma unroll
                for (int k = 0; k < 6; k++) { x[k] = x[k] + alpha * p[k]; rr[k] = r[k] - alpha * An[k]; r[k] = rr[k]; }
                mulv6(node + (size_t)kNodeWs * n + kMinv, rr, zz);
#pragma unroll
                for (int k = 0; k < 6; k++) { z[k] = zz[k]; rzn += rr[k] * zz[k]; }
            }
            rzn = block_sum(rzn, slot, ph);
            const double beta = rzn / rz;
            for (int n = tid; n < nn; n += PG_BLOCK) {
                if (fixed[n]) continue;
                double *p = vec(3, n);
                const double *z = vec(2, n);
#pragma unroll
                for (int k = 0; k < 6; k++) p[k] = z[k] + beta * p[k];
            }
            __syncthreads();                       /* p of every node before the next operator */
            rz = rzn;
            k_cg++;
        }
        double nonfinite = 0.0;
        for (int n = tid; n < nn; n += PG_BLOCK) {
            if (fixed[n]) continue;
            const double *x = vec(0, n);
#pragma unroll
            for (int k = 0; k < 6; k++) if (!is_finite(x[k])) nonfinite += 1.0;
        }
        nonfinite = block_sum(nonfinite, slot, ph);      /* its barrier: x of every node before the listed ones are read */
        marginal_column_end(rz, rz0, P.cg_tol, nonfinite == 0.0, &residual, &status);
    }
    if (tid < cols) out[tid] = solve ? vec(0, listed[tid / 6])[tid % 6] : 0.0;
    if (tid == 0) {
        out[cols] = residual;
        int *tail = reinterpret_cast<int *>(out + cols + 1);
        tail[0] = k_cg; tail[1] = status;
    }
}

}  // namespace dvo

namespace dvo_pg {
int launch_pose_graph_solve(const SolveArgs &a, int count, void *stream) {
    if (count < 1 || a.trace_cap < 1 || a.lds_nodes < 0 || a.lds_nodes > kLdsNodesMost) return (int)hipErrorInvalidValue;
    const size_t dyn = 240 * (size_t)a.lds_nodes;
    /* always the same value, the most any launch asks for: solves of two handles on two threads cannot undercut one another */
    const hipError_t e = hipFuncSetAttribute((const void *)dvo::pose_graph_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytesMost);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::pose_graph_solve_kernel, dim3((unsigned)count), dim3(dvo_pg::kBlock), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_pose_graph_marginals(const MarginalArgs &a, int count, void *stream) {
    if (count < 1 || a.m < 1 || a.m > DVO_GRAPH_MARGINAL_MAX_NODES || a.s.lds_nodes < 0 || a.s.lds_nodes > kLdsNodesMost) return (int)hipErrorInvalidValue;
    const size_t dyn = 240 * (size_t)a.s.lds_nodes;
    hipError_t e = hipFuncSetAttribute((const void *)dvo::pose_graph_marginal_columns_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytesMost);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::pose_graph_marginal_prepare_kernel, dim3((unsigned)count), dim3(dvo_pg::kBlock), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dvo::pose_graph_marginal_columns_kernel, dim3((unsigned)count * 6u * (unsigned)a.m), dim3(dvo_pg::kBlock), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
}  // namespace dvo_pg
