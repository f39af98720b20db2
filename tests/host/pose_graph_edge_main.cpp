/*
 * pose_graph_edge_main.cpp -- the per-edge functions of rgbd_odometry_amd/csrc/dvo_pose_graph.h (dvo_pg::se3_exp, se3_log, jr_inv,
 * edge_residual, edge_linearise, edge_jacobians) as a stand-alone program, so that tests/test_pose_graph_pins_cpu.py can compare what
 * they return with an independent reference, and run them under the address and undefined-behaviour sanitizers.
 *
 *   pose_graph_edge_main CASE_FILE
 *
 * CASE_FILE: int32 count, then per record an int32 kind and its payload:
 *   0  exp    6 doubles d                                   -> 12 doubles {R column-major, t}
 *   1  log    12 doubles {R column-major, t}                -> 6 doubles r
 *   2  jr     6 doubles r                                   -> 36 doubles Jr^-1 (row-major)
 *   3  edge   12 doubles P_i, 12 doubles P_j, one dvo_graph_edge (its i, j are ignored), 1 double huber_delta
 *             -> 6 doubles r of edge_residual, 120 doubles of edge_linearise, then r (6), J_i (36), J_j (36) of edge_jacobians
 * Output: one line per record, the doubles as hex floats separated by blanks.  Every array is allocated to its exact size, so that an
 * access past an end is the sanitizer's to see.
 */
#include "dvo_pose_graph.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool get(FILE *f, std::vector<double> &v) { return v.empty() || std::fread(v.data(), 8, v.size(), f) == v.size(); }

static void put(const std::vector<double> &v, bool end) {
    for (size_t k = 0; k < v.size(); k++) std::printf("%s%a", k ? " " : "", v[k]);
    std::printf(end ? "\n" : " ");
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s case_file\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    int count = 0;
    if (!f || std::fread(&count, 4, 1, f) != 1 || count < 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int k = 0; k < count; k++) {
        int kind = -1;
        if (std::fread(&kind, 4, 1, f) != 1 || kind < 0 || kind > 3) { std::fprintf(stderr, "record %d: bad kind\n", k); return 2; }
        bool ok = true;
        if (kind == 0) {
            std::vector<double> d(6), R(9), t(3);
            ok = get(f, d);
            if (ok) { dvo_pg::se3_exp(d.data(), R.data(), t.data()); put(R, false); put(t, true); }
        } else if (kind == 1) {
            std::vector<double> R(9), t(3), r(6);
            ok = get(f, R) && get(f, t);
            if (ok) { dvo_pg::se3_log(R.data(), t.data(), r.data()); put(r, true); }
        } else if (kind == 2) {
            std::vector<double> r(6), J(36);
            ok = get(f, r);
            if (ok) { dvo_pg::jr_inv(r.data(), J.data()); put(J, true); }
        } else {
            std::vector<double> P(24), delta(1), r(6), blk(dvo_pg::kBlk), r2(6), Ji(36), Jj(36);
            std::vector<dvo_graph_edge> E(1);
            ok = get(f, P) && std::fread(E.data(), sizeof(dvo_graph_edge), 1, f) == 1 && get(f, delta);
            if (ok) {
                E[0].i = 0; E[0].j = 1;                     /* the two poses stand where edge_linearise expects them */
                dvo_pg::edge_residual(P.data(), P.data() + 12, E.data(), r.data(), nullptr, nullptr);
                dvo_pg::edge_linearise(P.data(), E.data(), delta[0], blk.data());
                dvo_pg::edge_jacobians(P.data(), P.data() + 12, E.data(), r2.data(), Ji.data(), Jj.data());
                put(r, false); put(blk, false); put(r2, false); put(Ji, false); put(Jj, true);
            }
        }
        if (!ok) { std::fprintf(stderr, "record %d: short file\n", k); return 2; }
    }
    std::fclose(f);
    return 0;
}
