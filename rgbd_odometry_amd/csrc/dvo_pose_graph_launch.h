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

}  // namespace dvo_pg
#endif
