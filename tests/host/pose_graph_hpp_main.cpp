/*
 * pose_graph_hpp_main.cpp -- the pose-graph part of the C++ mirror (include/dvo_amd.hpp: PoseGraph, addOdometryEdge, the addClosureEdge
 * template on SolveDVOStreams::Candidate, PoseGraphs) compiled and used: tests/test_pose_graph_cpu.py builds it with plain g++ against
 * the library and runs it.
 *
 * A chain of four nodes built with addNodeAfter from relative poses, odometry edges from information records, one closure edge from a
 * candidate record; solved on the host through the C entry point and, where a device is present, through PoseGraphs.  Output:
 * "edges N", "host status S iterations I x X" (X: the last node's t.x), then "device none" or "device status S diff D" (D: the largest
 * difference between the host's and the device's poses).
 */
#include "dvo_amd.hpp"

#include <cmath>
#include <cstdio>
#include <exception>

int main() {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0}, step[3] = {1.0, 0.1, 0.0};
    double H[36] = {0};
    for (int k = 0; k < 6; k++) H[k * 7] = 400.0 + 50.0 * k;
    dvo_amd::PoseGraph g;
    g.addNode(I, zero, true);
    bool ok = true;
    for (int n = 1; n < 4; n++) {
        const int node = g.addNodeAfter(n - 1, I, step);
        ok = ok && node == n && dvo_amd::addOdometryEdge(g, n - 1, n, I, step, H, 50.0, 500);
    }
    ok = ok && !dvo_amd::addOdometryEdge(g, 0, 1, I, step, H, 50.0, 6);          /* no information matrix from six points */
    dvo_amd::SolveDVOStreams::Candidate c;                                       /* a closure that says node 3 is at 2.7, not 3.0 */
    c.t[0] = 2.7; c.t[1] = 0.3;
    for (int k = 0; k < 36; k++) c.rec.H36[k] = H[k];
    c.rec.sum_eps2 = 20.0; c.rec.n_visible = 300;
    ok = ok && dvo_amd::addClosureEdge(g, 0, 3, c);
    if (!ok || g.nodes() != 4 || g.edges.size() != 4 || g.edges[3].flags != DVO_GRAPH_EDGE_ROBUST) { std::printf("build failed\n"); return 1; }
    std::printf("edges %zu\n", g.edges.size());
    dvo_amd::PoseGraph h = g;
    dvo_graph_report rep{};
    if (dvo_graph_solve_host(nullptr, h.nodes(), h.poses.data(), h.fixed.data(), (int)h.edges.size(), h.edges.data(), &rep, nullptr, 0) != DVO_OK) {
        std::printf("host refused\n");
        return 1;
    }
    std::printf("host status %d iterations %d x %.6f\n", rep.status, rep.iterations, h.poses[12 * 3 + 9]);
    try {
        dvo_amd::PoseGraphs graphs(2, 8, 8);
        graphs.set(1, g);
        graphs.solve({1});
        std::vector<double> trace;
        const dvo_graph_report r = graphs.report(1, &trace);
        const std::vector<double> p = graphs.poses(1);
        double d = 0.0;
        for (size_t k = 0; k < p.size(); k++) d = std::fmax(d, std::fabs(p[k] - h.poses[k]));
        std::printf("device status %d diff %.3e trace %zu\n", r.status, d, trace.size());
    } catch (const std::exception &e) {
        std::printf("device none (%s)\n", e.what());
    }
    return 0;
}
