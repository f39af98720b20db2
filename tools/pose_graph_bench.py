#!/usr/bin/env python3
"""Times of the pose-graph solver (include/dvo_amd.h, "pose graphs") on ring(200) graphs of tests/pose_graph_reference.py:

  * one graph alone on the device (a single workgroup: latency-bound),
  * --batch graphs (different seeds) in one dvo_graph_solve,
  * the host definition dvo_graph_solve_host on one core for the first --host-graphs of them.

A device time is the host clock around set + solve (the solve ends in its one synchronisation); every timed solve starts from the
graph's initial poses, because dvo_graph_set stages them again.  The first solve of every shape is a warm-up.  Prints one JSON line.
Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--host-graphs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import pose_graph_reference as pg
    from rgbd_odometry_amd import capi

    graphs = [pg.ring(a.nodes, seed=100 + k) for k in range(a.batch)]
    staged = [(pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g)) for g in graphs]
    n_edges = len(graphs[0]["i"])

    def timed(h, slots):
        best, reports = [], None
        for rep in range(a.repeats + 1):                  # the first is the warm-up
            t0 = time.perf_counter()
            for k in slots:
                h.set(k, *staged[k])
            t1 = time.perf_counter()
            h.solve(slots)
            t2 = time.perf_counter()
            if rep:
                best.append((t2 - t1, t1 - t0))
            reports = [h.report(k) for k in slots]
        solve = sorted(b[0] for b in best)
        return dict(solve_ms_median=1e3 * solve[len(solve) // 2], solve_ms_min=1e3 * solve[0], solve_ms_max=1e3 * solve[-1],
                    set_ms_median=1e3 * sorted(b[1] for b in best)[len(best) // 2],
                    outer_iterations=[r["iterations"] for r in reports][:8], cg_iterations_total=int(sum(r["cg_iterations"] for r in reports)),
                    statuses=sorted(set(r["status"] for r in reports)))

    out = dict(nodes=a.nodes, edges=n_edges, batch=a.batch, repeats=a.repeats)
    with capi.DvoPoseGraphs(a.batch, a.batch * a.nodes, a.batch * n_edges) as h:
        out["single"] = timed(h, [0])
        out["batched"] = timed(h, list(range(a.batch)))
        dev_poses = [h.poses(k) for k in range(min(a.host_graphs, a.batch))]
    for key in ("single", "batched"):
        out[key]["cg_iterations_per_second"] = out[key]["cg_iterations_total"] / (1e-3 * out[key]["solve_ms_median"])
    t0 = time.perf_counter()
    host = [capi.pose_graph_solve_host(*staged[k]) for k in range(min(a.host_graphs, a.batch))]
    dt = time.perf_counter() - t0
    cg = sum(r["cg_iterations"] for _, r in host)
    out["host_one_core"] = dict(graphs=len(host), ms_per_graph=1e3 * dt / len(host), cg_iterations_total=int(cg), cg_iterations_per_second=cg / dt)
    out["max_pose_difference_host_device"] = max(pg.pose_distance(*pg.from_poses12(P), *pg.from_poses12(D)) for (P, _), D in zip(host, dev_poses))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
