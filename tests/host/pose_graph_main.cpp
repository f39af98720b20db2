/*
 * pose_graph_main.cpp -- dvo_pg::solve_host (rgbd_odometry_amd/csrc/dvo_pose_graph.h: the body of dvo_graph_solve_host) as a
 * stand-alone program, so that tests/test_pose_graph_cpu.py can run it under the address and undefined-behaviour sanitizers.
 *
 *   pose_graph_main CASE_FILE
 *
 * CASE_FILE: int32 count, then per case int32 n_nodes, int32 n_edges, the bytes of one dvo_graph_params, 12 n_nodes doubles, n_nodes
 * bytes of fixed flags, n_edges dvo_graph_edge.  Output per case: "case k refused", or "case k ok" followed by the bytes of the
 * report, of the max_iterations + 1 trace entries and of the poses in hex, one line each.  Poses, flags, edges and the trace are
 * allocated to their exact sizes, so that an access past an end is the sanitizer's to see.
 */
#include "dvo_pose_graph.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) std::printf("%02x", b[i]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s case_file\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    int count = 0;
    if (!f || std::fread(&count, 4, 1, f) != 1 || count < 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int k = 0; k < count; k++) {
        int n = 0, ne = 0;
        dvo_graph_params prm;
        if (std::fread(&n, 4, 1, f) != 1 || std::fread(&ne, 4, 1, f) != 1 || std::fread(&prm, sizeof(prm), 1, f) != 1 || n < 0 || ne < 0) {
            std::fprintf(stderr, "case %d: short file\n", k);
            return 2;
        }
        std::vector<double> poses(12 * (size_t)n);
        std::vector<unsigned char> fixed((size_t)n);
        std::vector<dvo_graph_edge> edges((size_t)ne);
        if ((n && std::fread(poses.data(), 96, (size_t)n, f) != (size_t)n) || (n && std::fread(fixed.data(), 1, (size_t)n, f) != (size_t)n) ||
            (ne && std::fread(edges.data(), sizeof(dvo_graph_edge), (size_t)ne, f) != (size_t)ne)) {
            std::fprintf(stderr, "case %d: short file\n", k);
            return 2;
        }
        const std::vector<double> before = poses;
        const int cap = prm.max_iterations >= 0 ? prm.max_iterations + 1 : 1;
        std::vector<double> trace((size_t)cap, 0.0);
        dvo_graph_report rep;
        std::memset(&rep, 0xAB, sizeof(rep));
        if (dvo_pg::solve_host(&prm, n, poses.data(), fixed.data(), ne, edges.data(), &rep, trace.data(), cap) != dvo_pg::kOk) {
            if (poses != before) { std::fprintf(stderr, "a refused call wrote its poses\n"); return 4; }
            std::printf("case %d refused\n", k);
            continue;
        }
        std::printf("case %d ok\n", k);
        hex(&rep, sizeof(rep));
        hex(trace.data(), 8 * trace.size());
        hex(poses.data(), 8 * poses.size());
    }
    std::fclose(f);
    return 0;
}
