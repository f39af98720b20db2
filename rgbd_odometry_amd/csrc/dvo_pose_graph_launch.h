/*
 * dvo_pose_graph_launch.h -- internal interface between the pose-graph host code (dvo_capi_graph.cpp) and the device solver
 * (dvo_pose_graph.hip).  Not installed; plain structs only.  The solver's definition is dvo_pose_graph.h.
 */
#ifndef DVO_POSE_GRAPH_LAUNCH_H_
#define DVO_POSE_GRAPH_LAUNCH_H_

#include "dvo_pose_graph.h"

namespace dvo_pg {

/* ---- what the device solver (dvo_pose_graph.hip) is launched with; plain structs, filled by dvo_capi_graph.cpp ----
 * One listed graph.  Its resident data: poses at poses + 12 node_off, fixed at fixed + node_off, edges at edges + edge_off, the
 * incidence lists at ptr + ptr_off (n + 1 entries) and inc + 2 edge_off; its workspace: blk + kBlk edge_off, node + kNodeWs node_off.
 * blob_off >= 0: the graph was set since it was last solved, and its workgroup first copies poses | edges | ptr | inc | fixed (each
 * section padded to 8 bytes) from upload + blob_off into the resident arrays.  Its results go to out + out_off:
 * dvo_graph_report | trace_cap doubles | 12 n doubles */
struct DeviceGraph {
    int n, ne, node_off, edge_off, ptr_off, pad_;
    long long blob_off, out_off;
};
/* per-node workspace in HBM: the record of node_assemble, the five CG vectors (used when they do not fit the LDS), the trial pose */
constexpr int kNodeWs = kNode + 30 + 12, kWsVec = kNode, kWsTrial = kNode + 30;
constexpr int kBlock = 256;                        /* threads of the solver's workgroup */
struct SolveArgs {
    const DeviceGraph *graphs;                     /* device: the head of the upload */
    const unsigned char *upload;
    double *poses; unsigned char *fixed; dvo_graph_edge *edges; int *ptr; int *inc;
    double *blk, *node;
    unsigned char *out;
    dvo_graph_params prm;
    int trace_cap;                                 /* max_iterations + 1 */
    int lds_nodes;                                 /* a graph of at most this many nodes keeps its CG vectors in LDS */
};
DVO_PG_HD size_t pad8(size_t b) { return (b + 7) / 8 * 8; }
inline size_t blob_bytes(int n, int ne) {
    return 96 * (size_t)n + sizeof(dvo_graph_edge) * (size_t)ne + pad8(4 * ((size_t)n + 1)) + pad8(8 * (size_t)ne) + pad8((size_t)n);
}
inline size_t out_bytes(int n, int trace_cap) { return sizeof(dvo_graph_report) + 8 * (size_t)trace_cap + 96 * (size_t)n; }
/* ONE launch, one workgroup per listed graph (stream: a hipStream_t); returns the hipError_t */
int launch_pose_graph_solve(const SolveArgs &a, int count, void *stream);
/* the most nodes whose CG vectors (240 bytes each) fit the dynamic LDS of a launch: 160 KiB less the kernel's static part */
constexpr int kLdsBytesMost = 160 * 1024 - 256, kLdsNodesMost = kLdsBytesMost / 240;

/* ---- what the marginal-covariance kernels are launched with (dvo_graph_marginals) ----
 * s: as for a solve, except that a listed graph's out_off leads to its columns.  The upload holds, behind the descriptors, the listed
 * nodes (m per listed graph) and ws_off; behind those the blobs.  The results, at s.out: one int per listed graph (pad8'd), 1 where a
 * free node's undamped block has no Cholesky factor; then per listed graph, at out_off, 6 m columns -- column 6 b + k is the solve of
 * H x = e(nodes[b], k) -- of kMargColumn(m) doubles each: x at nodes[0 .. m) (6 doubles per node), the residual, and one double's room
 * for {int iterations, int status}.
 * ws: the CG vectors of the columns of graphs above s.lds_nodes nodes: column c of listed graph k at ws + ws_off[k] + 30 n c doubles, 30
 * per node (ws_off[k] is -1 for a graph whose vectors are in LDS) */
struct MarginalArgs {
    SolveArgs s;
    const int *nodes;
    const long long *ws_off;
    double *ws;
    int m, pad_;
};
constexpr int kMargVec = 30;                       /* doubles per node and column: x, r, z, p, A p */
inline size_t marg_column_doubles(int m) { return 6 * (size_t)m + 2; }
inline size_t marg_flags_bytes(int count) { return pad8(4 * (size_t)count); }
inline size_t marg_out_bytes(int m) { return 8 * 6 * (size_t)m * marg_column_doubles(m); }
/* the marginals' own part of an upload, behind the descriptors: nodes | ws_off */
inline size_t marg_query_bytes(int count, int m) { return pad8(4 * (size_t)count * (size_t)m) + 8 * (size_t)count; }
constexpr int kMarginalLaunches = 2;               /* == DVO_GRAPH_MARGINAL_LAUNCHES */
/* TWO launches: prepare (one workgroup per listed graph: the upload where due, every edge linearised, every free node assembled at
 * lambda = 0, the graph's flag) and columns (one workgroup per listed graph, node and k); returns the hipError_t */
int launch_pose_graph_marginals(const MarginalArgs &a, int count, void *stream);

}  // namespace dvo_pg
#endif
