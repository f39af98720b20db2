/*
 * pose_graph_marginals_hpp_main.cpp -- the marginal-covariance part of the C++ mirror (include/dvo_amd.hpp: PoseGraphs::marginals and
 * edgeChi2) compiled and used: tests/test_pose_graph_marginals_cpu.py builds it with plain g++ and every warning on, against the library.
 *
 * A chain of three nodes; the gate on its second edge with no covariance on the host, and, where a device is present, with the joint
 * covariance of the edge's nodes from PoseGraphs::marginals.  Output: "host chi2 X", then "device none (...)" or "device status S chi2 Y".
 */
#include "dvo_amd.hpp"

#include <cstdio>
#include <exception>

int main() {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0}, step[3] = {1.0, 0.1, 0.0}, seen[3] = {1.02, 0.1, 0.0};
    double info[36] = {0};
    for (int k = 0; k < 6; k++) info[k * 7] = 400.0 + 50.0 * k;
    dvo_amd::PoseGraph g;
    g.addNode(I, zero, true);
    g.addNodeAfter(0, I, step);
    g.addNodeAfter(1, I, step);
    g.addEdge(0, 1, I, step, info, false);
    g.addEdge(1, 2, I, seen, info, false);
    double chi2 = -1.0, r[6];
    if (!dvo_amd::edgeChi2(&g.poses[12], &g.poses[24], nullptr, g.edges[1], chi2, r)) { std::printf("host refused\n"); return 1; }
    std::printf("host chi2 %.6f\n", chi2);
    try {
        dvo_amd::PoseGraphs graphs(1, 4, 4);
        graphs.set(0, g);
        graphs.solve({0});
        std::vector<dvo_graph_marginal_report> rep;
        const std::vector<double> cov = graphs.marginals({0}, {1, 2}, &rep);
        const std::vector<double> p = graphs.poses(0);
        double gated = -1.0;
        if (cov.size() != 144 || !dvo_amd::edgeChi2(&p[12], &p[24], cov.data(), g.edges[1], gated)) { std::printf("device refused\n"); return 1; }
        std::printf("device status %d chi2 %.6f\n", rep[0].status, gated);
    } catch (const std::exception &e) {
        std::printf("device none (%s)\n", e.what());
    }
    return 0;
}
