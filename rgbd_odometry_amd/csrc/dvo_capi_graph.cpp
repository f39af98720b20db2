/*
 * dvo_capi_graph.cpp -- pose graphs (include/dvo_amd.h, "pose graphs"): the host solver's entry point (dvo_pose_graph.h is the
 * definition), the stand-alone batch handle and its one-launch solve (dvo_pose_graph.hip).  The handle touches no dvo_ctx and no
 * tracker.  Host side only; no CPU compute path behind the handle's entry points.
 */
#include "../../include/dvo_amd.h"
#include "dvo_handle.h"
#include "dvo_launch.h"
#include "dvo_pose_graph_launch.h"

#include <cstring>
#include <string>
#include <vector>

using namespace dvo_host;
using namespace dvo_pg;

/* A graph is staged on the host by dvo_graph_set (validated there, its incidence lists built there) and goes up with the next solve
 * that lists it.  The host copy of the poses is always current: a solve copies the solved poses back.  Resident device arrays are
 * indexed by node and edge offsets, the prefix sums of the set graphs' sizes in graph order; when a graph's size changes the offsets
 * move, and every set graph is uploaded again with the solve that next lists it. */
struct dvo_graph_batch : Handle {
    int max_graphs = 0, max_nodes = 0, max_edges = 0;
    struct Graph {
        bool set = false, dirty = false, solved = false;
        int n = 0, ne = 0, node_off = 0, edge_off = 0;
        std::vector<double> poses, trace;
        std::vector<unsigned char> fixed;
        std::vector<dvo_graph_edge> edges;
        std::vector<int> ptr, inc;
        dvo_graph_report rep = {};
    };
    std::vector<Graph> g;
    bool layout_dirty = true;
    int nodes_set = 0, edges_set = 0;
    DevBuf<double> d_poses, d_blk, d_node;
    DevBuf<double> d_marg_ws;                      /* CG vectors of the marginals' columns of graphs too large for the LDS; grows on demand */
    DevBuf<unsigned char> d_fixed;
    DevBuf<dvo_graph_edge> d_edges;
    DevBuf<int> d_ptr, d_inc;
    Staging upload, out;                           /* the one upload of a call (sized at creation); its results (grow on demand) */
};

namespace {
thread_local std::string g_graph_create_error;     /* of the calling thread's last failed creation */

int gfail(dvo_graph_batch *b, int code, const std::string &msg) {
    (b ? b->err : g_graph_create_error) = msg;
    return code;
}
#define GHIP(b, expr) DVO_HIP_CHECK(gfail, b, expr, #expr)

size_t upload_capacity(const dvo_graph_batch &b) {
    return pad8(sizeof(DeviceGraph) * (size_t)b.max_graphs) + 96 * (size_t)b.max_nodes + sizeof(dvo_graph_edge) * (size_t)b.max_edges +
           4 * (size_t)b.max_nodes + 8 * (size_t)b.max_edges + (size_t)b.max_nodes + 32 * (size_t)b.max_graphs +
           marg_query_bytes(b.max_graphs, DVO_GRAPH_MARGINAL_MAX_NODES);      /* a marginals call lists its nodes behind the descriptors */
}

/* what a solve and a marginals call refuse in their list: DVO_OK, or the code with the handle's message set */
int list_ok(dvo_graph_batch *b, int count, const int *graphs) {
    if (!graphs || count < 1 || count > b->max_graphs) return gfail(b, DVO_ERR_INVALID, "count outside [1, max_graphs] or a NULL list");
    std::vector<char> seen((size_t)b->max_graphs, 0);
    for (int k = 0; k < count; k++) {
        const int q = graphs[k];
        if (q < 0 || q >= b->max_graphs) return gfail(b, DVO_ERR_INVALID, "a listed graph is outside [0, max_graphs)");
        if (seen[(size_t)q]) return gfail(b, DVO_ERR_INVALID, "graph " + std::to_string(q) + " is listed twice");
        if (!b->g[(size_t)q].set) return gfail(b, DVO_ERR_STATE, "graph " + std::to_string(q) + " was never set (dvo_graph_set)");
        seen[(size_t)q] = 1;
    }
    return DVO_OK;
}

/* the offsets of the set graphs in the resident arrays, when a graph's size changed since they were last assigned */
void assign_layout(dvo_graph_batch *b) {
    if (!b->layout_dirty) return;
    int no = 0, eo = 0;
    for (dvo_graph_batch::Graph &G : b->g) {
        if (!G.set) continue;
        G.node_off = no; G.edge_off = eo; G.dirty = true;
        no += G.n; eo += G.ne;
    }
    b->layout_dirty = false;
}

/* the bytes of an upload whose descriptors and the like take `head`: behind them the data of the listed graphs set since they last went up */
size_t upload_bytes(const dvo_graph_batch *b, int count, const int *graphs, size_t head) {
    for (int k = 0; k < count; k++) {
        const dvo_graph_batch::Graph &G = b->g[(size_t)graphs[k]];
        if (G.dirty) head += blob_bytes(G.n, G.ne);
    }
    return head;
}

/* descriptor k of the list (out_off is the caller's) and, for a graph set since it last went up, its data at upload.host + up; returns the
 * new end of the upload */
size_t stage_listed(dvo_graph_batch *b, int q, DeviceGraph &D, size_t up) {
    const dvo_graph_batch::Graph &G = b->g[(size_t)q];
    D.n = G.n; D.ne = G.ne; D.node_off = G.node_off; D.edge_off = G.edge_off; D.ptr_off = G.node_off + q; D.pad_ = 0;
    D.blob_off = -1;
    if (!G.dirty) return up;
    D.blob_off = (long long)up;
    unsigned char *dst = b->upload.host + up;
    std::memset(dst, 0, blob_bytes(G.n, G.ne));
    std::memcpy(dst, G.poses.data(), 96 * (size_t)G.n);
    dst += 96 * (size_t)G.n;
    if (G.ne) std::memcpy(dst, G.edges.data(), sizeof(dvo_graph_edge) * (size_t)G.ne);
    dst += sizeof(dvo_graph_edge) * (size_t)G.ne;
    std::memcpy(dst, G.ptr.data(), 4 * ((size_t)G.n + 1));
    dst += pad8(4 * ((size_t)G.n + 1));
    if (G.ne) std::memcpy(dst, G.inc.data(), 8 * (size_t)G.ne);
    dst += pad8(8 * (size_t)G.ne);
    std::memcpy(dst, G.fixed.data(), (size_t)G.n);
    return up + blob_bytes(G.n, G.ne);
}
}  // namespace

extern "C" {

int dvo_graph_params_default(dvo_graph_params *p) {
    if (!p) return DVO_ERR_INVALID;
    params_default(p);
    return DVO_OK;
}

int dvo_graph_solve_host(const dvo_graph_params *p, int n_nodes, double *poses12, const unsigned char *fixed, int n_edges,
                         const dvo_graph_edge *edges, dvo_graph_report *report, double *cost_trace, int trace_capacity) {
    return solve_host(p, n_nodes, poses12, fixed, n_edges, edges, report, cost_trace, trace_capacity) == kOk ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_graph_marginals_host(const dvo_graph_params *p, int n_nodes, const double *poses12, const unsigned char *fixed, int n_edges,
                             const dvo_graph_edge *edges, int m, const int *nodes, double *cov, dvo_graph_marginal_report *report) {
    return marginals_host(p, n_nodes, poses12, fixed, n_edges, edges, m, nodes, cov, report) == kOk ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_graph_edge_chi2(const double *pose_i12, const double *pose_j12, const double *cov144, const dvo_graph_edge *edge, double *r6, double *S36,
                        double *chi2) {
    return edge_chi2(pose_i12, pose_j12, cov144, edge, r6, S36, chi2) == kOk ? DVO_OK : DVO_ERR_INVALID;
}

int dvo_graph_information(const double *H36, double sum_eps2, int n_visible, double *info36) {
    if (!H36 || !info36 || n_visible <= 6 || !is_finite(sum_eps2) || !(sum_eps2 > 0.0)) return DVO_ERR_INVALID;
    for (int k = 0; k < 36; k++) if (!is_finite(H36[k])) return DVO_ERR_INVALID;
    double L[36];
    if (!chol6(H36, L)) return DVO_ERR_INVALID;
    const double scale = (double)(n_visible - 6) / sum_eps2;
    for (int k = 0; k < 36; k++) info36[k] = H36[k] * scale;
    return DVO_OK;
}

int dvo_graph_create(int max_graphs, int max_nodes_total, int max_edges_total, dvo_graph_batch **out) {
    if (!out) return gfail(nullptr, DVO_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (max_graphs < 1 || max_nodes_total < 1 || max_edges_total < 0 || max_graphs > max_nodes_total)
        return gfail(nullptr, DVO_ERR_INVALID, "bad capacities (max_graphs >= 1, max_nodes_total >= max_graphs, max_edges_total >= 0)");
    std::string why;
    if (const int rc = device_check(&why)) return gfail(nullptr, rc, why);
    dvo_graph_batch *b = new dvo_graph_batch();
    b->max_graphs = max_graphs; b->max_nodes = max_nodes_total; b->max_edges = max_edges_total;
    b->g.resize((size_t)max_graphs);
    const size_t N = (size_t)max_nodes_total, M = (size_t)(max_edges_total > 0 ? max_edges_total : 1), up = upload_capacity(*b);
    hipError_t r = b->open();
    if (r == hipSuccess) r = b->d_poses.alloc(12 * N);
    if (r == hipSuccess) r = b->d_fixed.alloc(N);
    if (r == hipSuccess) r = b->d_edges.alloc(M);
    if (r == hipSuccess) r = b->d_ptr.alloc(N + (size_t)max_graphs);
    if (r == hipSuccess) r = b->d_inc.alloc(2 * M);
    if (r == hipSuccess) r = b->d_blk.alloc((size_t)kBlk * M);
    if (r == hipSuccess) r = b->d_node.alloc((size_t)kNodeWs * N);
    if (r == hipSuccess) r = b->upload.reserve(up);
    if (r != hipSuccess) {
        const std::string msg = std::string("pose-graph buffers: ") + hipGetErrorString(r);
        dvo_graph_destroy(b);
        return gfail(nullptr, hip_status(r), msg);
    }
    *out = b;
    return DVO_OK;
}

int dvo_graph_destroy(dvo_graph_batch *b) {
    if (!b) return DVO_ERR_INVALID;
    OnDevice guard(b->device);
    b->close();
    delete b;                                      /* the buffers go here, on the handle's device */
    return DVO_OK;
}

const char *dvo_graph_last_error(const dvo_graph_batch *b) { return b ? b->err.c_str() : g_graph_create_error.c_str(); }

int dvo_graph_set(dvo_graph_batch *b, int graph, int n_nodes, const double *poses12, const unsigned char *fixed, int n_edges,
                  const dvo_graph_edge *edges) {
    if (!b) return DVO_ERR_INVALID;
    if (graph < 0 || graph >= b->max_graphs) return gfail(b, DVO_ERR_INVALID, "graph outside [0, max_graphs)");
    if (n_nodes < 1 || n_nodes > DVO_GRAPH_MAX_NODES) return gfail(b, DVO_ERR_INVALID, "n_nodes outside [1, DVO_GRAPH_MAX_NODES]");
    std::vector<int> scratch(2 * (size_t)n_nodes);
    if (!graph_ok(n_nodes, poses12, fixed, n_edges, edges, scratch.data()))
        return gfail(b, DVO_ERR_INVALID, "bad graph (NULL array, counts, edge indices, a number that is not finite, an information matrix that is "
                                         "not symmetric positive definite, unknown flags, or a connected component without a fixed node)");
    dvo_graph_batch::Graph &G = b->g[(size_t)graph];
    const int nodes_after = b->nodes_set - (G.set ? G.n : 0) + n_nodes, edges_after = b->edges_set - (G.set ? G.ne : 0) + n_edges;
    if (nodes_after > b->max_nodes || edges_after > b->max_edges)
        return gfail(b, DVO_ERR_INVALID, "the set graphs would hold more nodes or edges than the handle was created for");
    if (!G.set || G.n != n_nodes || G.ne != n_edges) b->layout_dirty = true;
    b->nodes_set = nodes_after; b->edges_set = edges_after;
    G.set = true; G.dirty = true; G.solved = false;
    G.n = n_nodes; G.ne = n_edges;
    G.poses.assign(poses12, poses12 + 12 * (size_t)n_nodes);
    G.fixed.assign(fixed, fixed + n_nodes);
    G.edges.assign(edges, edges + n_edges);
    G.ptr.assign((size_t)n_nodes + 1, 0);
    G.inc.assign(2 * (size_t)n_edges, 0);
    build_csr(n_nodes, n_edges, G.edges.data(), G.ptr.data(), G.inc.data());
    G.trace.clear();
    return DVO_OK;
}

int dvo_graph_solve(dvo_graph_batch *b, const dvo_graph_params *p, int count, const int *graphs) {
    if (!b) return DVO_ERR_INVALID;
    dvo_graph_params P;
    if (p) P = *p; else params_default(&P);
    /* refusals first: a refused call changes nothing */
    if (!params_ok(&P)) return gfail(b, DVO_ERR_INVALID, "bad parameters (counts >= 0, lambda_up > 1, lambda_down inside (0, 1), every number finite)");
    if (const int rc = list_ok(b, count, graphs)) return rc;
    OnDevice guard(b->device);
    assign_layout(b);
    const int trace_cap = P.max_iterations + 1;
    size_t out_total = 0;
    for (int k = 0; k < count; k++) out_total += out_bytes(b->g[(size_t)graphs[k]].n, trace_cap);
    const size_t up_total = upload_bytes(b, count, graphs, pad8(sizeof(DeviceGraph) * (size_t)count));
    if (up_total > b->upload.host.size()) return gfail(b, DVO_ERR_STATE, "internal: the upload does not fit its buffer");
    /* the result block grows with max_iterations and the listed sizes: then, and only then, a solve allocates */
    GHIP(b, b->out.reserve(out_total));
    /* the one upload: the list's descriptors, then the data of the listed graphs that were set since they last went up */
    DeviceGraph *desc = reinterpret_cast<DeviceGraph *>(b->upload.host.get());
    size_t up = pad8(sizeof(DeviceGraph) * (size_t)count), out_off = 0;
    int lds_nodes = 0;
    for (int k = 0; k < count; k++) {
        const dvo_graph_batch::Graph &G = b->g[(size_t)graphs[k]];
        desc[k].out_off = (long long)out_off;
        out_off += out_bytes(G.n, trace_cap);
        if (G.n <= kLdsNodesMost && G.n > lds_nodes) lds_nodes = G.n;
        up = stage_listed(b, graphs[k], desc[k], up);
    }
    CallStats stats(*b, dvo::g_kernel_launches);
    /* from here on a failure leaves the device copies undefined: the listed graphs go up again next time, from the host's poses */
    for (int k = 0; k < count; k++) b->g[(size_t)graphs[k]].dirty = true;
    GHIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up, hipMemcpyHostToDevice, b->stream));
    SolveArgs a;
    a.graphs = reinterpret_cast<const DeviceGraph *>(b->upload.dev.get());
    a.upload = b->upload.dev;
    a.poses = b->d_poses; a.fixed = b->d_fixed; a.edges = b->d_edges; a.ptr = b->d_ptr; a.inc = b->d_inc;
    a.blk = b->d_blk; a.node = b->d_node; a.out = b->out.dev;
    a.prm = P; a.trace_cap = trace_cap; a.lds_nodes = lds_nodes;
    GHIP(b, (hipError_t)launch_pose_graph_solve(a, count, b->stream));
    stats.launched();
    GHIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    GHIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    for (int k = 0; k < count; k++) {
        dvo_graph_batch::Graph &G = b->g[(size_t)graphs[k]];
        const unsigned char *src = b->out.host + desc[k].out_off;
        std::memcpy(&G.rep, src, sizeof(dvo_graph_report));
        G.trace.resize((size_t)trace_cap);
        std::memcpy(G.trace.data(), src + sizeof(dvo_graph_report), 8 * (size_t)trace_cap);
        std::memcpy(G.poses.data(), src + sizeof(dvo_graph_report) + 8 * (size_t)trace_cap, 96 * (size_t)G.n);
        G.trace.resize((size_t)G.rep.iterations + 1);
        G.dirty = false; G.solved = true;
    }
    return DVO_OK;
}

int dvo_graph_marginals(dvo_graph_batch *b, const dvo_graph_params *p, int count, const int *graphs, int m, const int *nodes, double *cov,
                        dvo_graph_marginal_report *reports) {
    if (!b) return DVO_ERR_INVALID;
    dvo_graph_params P;
    if (p) P = *p; else params_default(&P);
    /* refusals first: a refused call changes nothing */
    if (!params_ok(&P)) return gfail(b, DVO_ERR_INVALID, "bad parameters (counts >= 0, lambda_up > 1, lambda_down inside (0, 1), every number finite)");
    if (const int rc = list_ok(b, count, graphs)) return rc;
    if (m < 1 || m > DVO_GRAPH_MARGINAL_MAX_NODES || !nodes || !cov || !reports)
        return gfail(b, DVO_ERR_INVALID, "m outside [1, DVO_GRAPH_MARGINAL_MAX_NODES] or a NULL nodes, cov or reports");
    for (int k = 0; k < count; k++)
        if (!marginal_query_ok(b->g[(size_t)graphs[k]].n, m, nodes + (size_t)k * m))
            return gfail(b, DVO_ERR_INVALID, "a listed node of graph " + std::to_string(graphs[k]) + " is out of range or listed twice");
    OnDevice guard(b->device);
    /* a graph above the LDS keeps the five CG vectors of each of its 6 m columns in the workspace: 240 bytes per node and column */
    std::vector<long long> ws_off((size_t)count, -1);
    size_t ws_total = 0;
    int lds_nodes = 0;
    for (int k = 0; k < count; k++) {
        const dvo_graph_batch::Graph &G = b->g[(size_t)graphs[k]];
        if (G.n <= kLdsNodesMost) { if (G.n > lds_nodes) lds_nodes = G.n; continue; }
        ws_off[(size_t)k] = (long long)ws_total;
        ws_total += (size_t)kMargVec * (size_t)G.n * 6 * (size_t)m;
    }
    const size_t w = 6 * (size_t)m, out_total = marg_flags_bytes(count) + (size_t)count * marg_out_bytes(m);
    /* the workspace and the result block grow on demand, before anything else changes: a call they do not fit is refused */
    if (ws_total > b->d_marg_ws.size()) GHIP(b, b->d_marg_ws.alloc(ws_total));
    GHIP(b, b->out.reserve(out_total));
    assign_layout(b);
    const size_t head = pad8(sizeof(DeviceGraph) * (size_t)count), query = marg_query_bytes(count, m);
    const size_t up_total = upload_bytes(b, count, graphs, head + query);
    if (up_total > b->upload.host.size()) return gfail(b, DVO_ERR_STATE, "internal: the upload does not fit its buffer");
    /* the one upload: the list's descriptors, the listed nodes, the workspace offsets, then the data of the graphs that are due */
    DeviceGraph *desc = reinterpret_cast<DeviceGraph *>(b->upload.host.get());
    std::memset(b->upload.host + head, 0, query);
    std::memcpy(b->upload.host + head, nodes, 4 * (size_t)count * (size_t)m);
    std::memcpy(b->upload.host + head + pad8(4 * (size_t)count * (size_t)m), ws_off.data(), 8 * (size_t)count);
    size_t up = head + query;
    for (int k = 0; k < count; k++) {
        desc[k].out_off = (long long)(marg_flags_bytes(count) + (size_t)k * marg_out_bytes(m));
        up = stage_listed(b, graphs[k], desc[k], up);
    }
    CallStats stats(*b, dvo::g_kernel_launches);
    /* from here on a failure leaves the device copies undefined: the listed graphs go up again next time, from the host's poses */
    for (int k = 0; k < count; k++) b->g[(size_t)graphs[k]].dirty = true;
    GHIP(b, hipMemcpyAsync(b->upload.dev, b->upload.host, up, hipMemcpyHostToDevice, b->stream));
    MarginalArgs a;
    a.s.graphs = reinterpret_cast<const DeviceGraph *>(b->upload.dev.get());
    a.s.upload = b->upload.dev;
    a.s.poses = b->d_poses; a.s.fixed = b->d_fixed; a.s.edges = b->d_edges; a.s.ptr = b->d_ptr; a.s.inc = b->d_inc;
    a.s.blk = b->d_blk; a.s.node = b->d_node; a.s.out = b->out.dev;
    a.s.prm = P; a.s.trace_cap = 1; a.s.lds_nodes = lds_nodes;
    a.nodes = reinterpret_cast<const int *>(b->upload.dev.get() + head);
    a.ws_off = reinterpret_cast<const long long *>(b->upload.dev.get() + head + pad8(4 * (size_t)count * (size_t)m));
    a.ws = b->d_marg_ws;
    a.m = m; a.pad_ = 0;
    GHIP(b, (hipError_t)launch_pose_graph_marginals(a, count, b->stream));
    stats.launched();
    GHIP(b, hipMemcpyAsync(b->out.host, b->out.dev, out_total, hipMemcpyDeviceToHost, b->stream));
    GHIP(b, hipStreamSynchronize(b->stream));
    stats.synced();
    /* the graphs are resident as a solve would have left them; poses, reports and traces on the host are untouched */
    for (int k = 0; k < count; k++) b->g[(size_t)graphs[k]].dirty = false;
    std::vector<double> M(w * w);
    const int *flags = reinterpret_cast<const int *>(b->out.host.get());
    for (int k = 0; k < count; k++) {
        const double *cols = reinterpret_cast<const double *>(b->out.host + desc[k].out_off);
        double *C = cov + (size_t)k * w * w;
        dvo_graph_marginal_report R = {0.0, 0, 0, DVO_GRAPH_CONVERGED};
        if (flags[k]) {                            /* a free node's block has no Cholesky factor */
            for (size_t u = 0; u < w * w; u++) C[u] = 0.0;
            R.status = DVO_GRAPH_NUMERIC;
            reports[k] = R;
            continue;
        }
        for (size_t c = 0; c < w; c++) {
            const double *col = cols + c * marg_column_doubles(m);
            for (size_t u = 0; u < w; u++) M[u * w + c] = col[u];
            const double residual = col[w];
            int tail[2];
            std::memcpy(tail, col + w + 1, sizeof(tail));
            R.cg_iterations += tail[0];
            if (tail[0] > R.cg_iterations_max) R.cg_iterations_max = tail[0];
            if (tail[1] > R.status) R.status = tail[1];
            if (residual > R.worst_residual || !is_finite(residual)) R.worst_residual = residual;
        }
        marginal_symmetrise(m, M.data(), C);
        reports[k] = R;
    }
    return DVO_OK;
}

int dvo_graph_get_poses(dvo_graph_batch *b, int graph, double *poses12) {
    if (!b) return DVO_ERR_INVALID;
    if (graph < 0 || graph >= b->max_graphs || !poses12) return gfail(b, DVO_ERR_INVALID, "graph outside [0, max_graphs) or a NULL buffer");
    const dvo_graph_batch::Graph &G = b->g[(size_t)graph];
    if (!G.set) return gfail(b, DVO_ERR_STATE, "graph " + std::to_string(graph) + " was never set (dvo_graph_set)");
    std::memcpy(poses12, G.poses.data(), 96 * (size_t)G.n);
    return DVO_OK;
}

int dvo_graph_get_report(dvo_graph_batch *b, int graph, dvo_graph_report *report, double *cost_trace, int trace_capacity) {
    if (!b) return DVO_ERR_INVALID;
    if (graph < 0 || graph >= b->max_graphs || !report || trace_capacity < 0 || (trace_capacity > 0 && !cost_trace))
        return gfail(b, DVO_ERR_INVALID, "graph outside [0, max_graphs), a NULL report, or a trace buffer that does not match its capacity");
    const dvo_graph_batch::Graph &G = b->g[(size_t)graph];
    if (!G.set || !G.solved) return gfail(b, DVO_ERR_STATE, "graph " + std::to_string(graph) + " has not been solved since it was set");
    *report = G.rep;
    for (size_t k = 0; k < G.trace.size() && k < (size_t)trace_capacity; k++) cost_trace[k] = G.trace[k];
    return DVO_OK;
}

int dvo_graph_stats(dvo_graph_batch *b, int *last_launches, int *last_syncs) {
    return b ? b->stats(last_launches, last_syncs) : DVO_ERR_INVALID;
}

}  // extern "C"
