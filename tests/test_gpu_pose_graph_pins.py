"""Pose graphs on the device against the independent reference (tests/pose_graph_independent.py) and on the paths no test had run:
cost0 as a probe of the kernel's residual mathematics on a sweep of angles that ends at a half turn, a graph that starts next to a
half turn, a start cost that is not finite, and the parameters the device had never been given.  Everything here is an ordinary
solve of a valid graph through capi.DvoPoseGraphs.

Tolerances: cost0 against the reference to ind.COST0_TOLERANCE, a hundred times what the host definition was measured at on the same
graphs (the device's sin / cos / atan2 are its own library's and its sums run in lane order); device against host as everywhere, poses
to 1e-7 and the final cost to 1e-9 relative."""
import numpy as np
import pytest

import pose_graph_independent as ind
import pose_graph_reference as pg

pytestmark = pytest.mark.gpu


def _set(h, slot, g):
    h.set(slot, pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g))


def test_cost0_probes_the_residual_of_the_kernel():
    """max_iterations = 0 returns cost0 and the untouched poses: every probe graph (a third of the Log sweep, Omega = I and anisotropic)
    in ONE handle and one launch, cost0 against the reference's r^T Omega r.  Near pi the cost is about pi^2 Omega: a Log that reports
    no rotation there misses by orders of magnitude (it did, from pi - 1e-9 on, before the symmetric-part branch)"""
    from rgbd_odometry_amd import capi
    graphs = ind.probe_graphs()
    n = len(graphs)
    assert 0 < n <= 512
    worst = {}
    with capi.DvoPoseGraphs(n, 2 * n, n) as h:
        for k, g in enumerate(graphs):
            _set(h, k, g)
        h.solve(list(range(n)), capi.DvoGraphParams.default(max_iterations=0))
        assert h.stats() == (1, 1)
        for k, g in enumerate(graphs):
            rep = h.report(k)
            assert rep["status"] == pg.MAX_ITERATIONS and rep["iterations"] == 0 and rep["accepted"] == 0, g["name"]
            assert rep["cost"] == rep["cost0"] and len(rep["cost_trace"]) == 1 and rep["cost_trace"][0] == rep["cost0"], g["name"]
            assert h.poses(k).tobytes() == pg.poses12(g["R0"], g["t0"]).tobytes(), g["name"]
            worst[g["label"]] = max(worst.get(g["label"], 0.0), ind.cost_error(rep["cost0"], g))
    for label, e in worst.items():
        print("theta %-12s device cost0 against the reference %.3e" % (label, e))
    print("worst %.3e of %.3e allowed" % (max(worst.values()), ind.COST0_TOLERANCE))
    bad = {k: v for k, v in worst.items() if not v <= ind.COST0_TOLERANCE}
    assert not bad, bad


def test_half_turn_start():
    """ring_half_turn: two edges start with residuals of pi - 0.021 and pi - 0.056, inside Log's symmetric-part branch.  Host and device
    report the true start cost, lower it and agree with one another.  Neither is asked to reach the truth: the host definition does not from this start (established on the CPU,
    tests/test_pose_graph_pins_cpu.py: it settles in a local minimum 2.45 rad away), so the distance is printed only"""
    from rgbd_odometry_amd import capi
    g = pg.ring_half_turn()
    want = float(ind.graph_cost(g, g["R0"], g["t0"], pg.DEFAULTS["huber_delta"]))
    Rh, th, host = pg.host_solved_graph(g)
    with capi.DvoPoseGraphs(1, g["n"], len(g["i"])) as h:
        _set(h, 0, g)
        h.solve([0])
        dev = h.report(0)
        R, t = pg.from_poses12(h.poses(0))
    d = pg.pose_distance(Rh, th, R, t)
    rel = abs(dev["cost"] - host["cost"]) / max(abs(host["cost"]), 1e-300) if host["cost"] > 1e-20 else abs(dev["cost"] - host["cost"])
    for who, rep, Rs, ts in (("host", host, Rh, th), ("device", dev, R, t)):
        print("%s: cost0 %.6e (reference %.6e, relative %.2e), cost %.3e, %d iterations, status %d, to the truth %.3e" % (
            who, rep["cost0"], want, abs(rep["cost0"] - want) / want, rep["cost"], rep["iterations"], rep["status"],
            pg.pose_distance(*g["truth"], Rs, ts)))
        assert abs(rep["cost0"] - want) <= ind.COST0_TOLERANCE * want
        assert rep["status"] != pg.NUMERIC and rep["cost"] < rep["cost0"]
    print("device against host: poses %.3e, cost %.3e" % (d, rel))
    assert dev["status"] == host["status"]
    assert d <= 1e-7 and rel <= 1e-9


def test_a_start_cost_that_is_not_finite():
    """pair_overflow: every input is finite and the graph is accepted, r^T Omega r overflows.  Host and device: DVO_GRAPH_NUMERIC, no
    iteration, the poses as they came.  (Omega is 1e308 I: with 1e300 I and a residual of order 1 the cost is 1e300, which is finite)"""
    from rgbd_odometry_amd import capi
    g = pg.pair_overflow()
    P0 = pg.poses12(g["R0"], g["t0"])
    assert 1.5 < np.linalg.norm(pg.residuals(g, g["R0"], g["t0"])[0]) < 3.0
    P, host = capi.pose_graph_solve_host(P0, g["fixed"], pg.c_edges(g))
    with capi.DvoPoseGraphs(1, 2, 1) as h:
        _set(h, 0, g)
        h.solve([0])
        dev, Pd = h.report(0), h.poses(0)
    for who, rep, Q in (("host", host, P), ("device", dev, Pd)):
        print("%s: status %d, iterations %d, cost0 %r" % (who, rep["status"], rep["iterations"], rep["cost0"]))
        assert rep["status"] == pg.NUMERIC and rep["iterations"] == 0 and rep["accepted"] == 0 and rep["cg_iterations"] == 0
        assert not np.isfinite(rep["cost0"]) and len(rep["cost_trace"]) == 1
        assert Q.tobytes() == P0.tobytes()


PARAMS = {"huber_delta = 0": dict(huber_delta=0.0), "huber_delta = 0.25": dict(huber_delta=0.25), "cg_max_iterations = 3": dict(cg_max_iterations=3),
          "lambda0 = lambda_min = 0": dict(lambda0=0.0, lambda_min=0.0), "no tolerances, 12 iterations": dict(step_tol=0.0, cost_tol=0.0, max_iterations=12)}
PARAM_GRAPHS = ["ring(65)", "outlier"]


@pytest.fixture(scope="module")
def param_handle():
    from rgbd_odometry_amd import capi
    n = max(pg.cases()[name]["n"] for name in PARAM_GRAPHS)
    ne = max(len(pg.cases()[name]["i"]) for name in PARAM_GRAPHS)
    with capi.DvoPoseGraphs(1, n, ne) as h:
        yield h


@pytest.mark.parametrize("name", PARAM_GRAPHS)
@pytest.mark.parametrize("what", list(PARAMS))
def test_parameters_the_device_had_not_been_given(param_handle, what, name):
    """The device against the host definition under parameters away from the defaults, on ring(65) and on `outlier` (robust edges): poses
    to 1e-7, the final cost to 1e-9 relative, a trace of iterations + 1 entries, equal statuses.

    With step_tol = cost_tol = 0 no tolerance can stop the loop (a tolerance of 0 is off: not even a trial of exactly equal cost counts as
    a decrease <= 0), so it ends by the cap or by a rejection at lambda_max.  Before that rule ring(65) told device and host apart here:
    it reaches the rounding floor of its cost after six steps, the device (sums over lanes and waves) met a trial of bit-equal cost at
    iteration 11 and reported CONVERGED, the host (sums in index order) met none in 12 and reported MAX_ITERATIONS, with poses 9.2e-16
    apart -- a status decided by the last bit of a sum"""
    from rgbd_odometry_amd import capi
    h, changes, g = param_handle, PARAMS[what], pg.cases()[name]
    _set(h, 0, g)
    h.solve([0], capi.DvoGraphParams.default(**changes))
    Rh, th, host = pg.host_solved_graph(g, **changes)
    dev = h.report(0)
    R, t = pg.from_poses12(h.poses(0))
    d = pg.pose_distance(Rh, th, R, t)
    rel = abs(dev["cost"] - host["cost"]) / max(abs(host["cost"]), 1e-300)
    print("%s, %s: device status %d, iterations %d, accepted %d, cg %d (host %d, %d, %d, %d), lambda %.1e (host %.1e), poses %.3e, cost %.3e" % (
        what, name, dev["status"], dev["iterations"], dev["accepted"], dev["cg_iterations"], host["status"], host["iterations"],
        host["accepted"], host["cg_iterations"], dev["lambda_"], host["lambda_"], d, rel))
    assert len(dev["cost_trace"]) == dev["iterations"] + 1 and dev["cost_trace"][0] == dev["cost0"] and dev["cost_trace"][-1] == dev["cost"]
    assert len(host["cost_trace"]) == host["iterations"] + 1
    if "max_iterations" in changes:
        assert dev["iterations"] <= changes["max_iterations"] and host["iterations"] <= changes["max_iterations"]
        for rep in (dev, host):                              # the cap, or a rejection at lambda_max: nothing else can end it
            assert (rep["status"] == pg.MAX_ITERATIONS and rep["iterations"] == changes["max_iterations"]) or rep["lambda_"] >= pg.DEFAULTS["lambda_max"]
    assert d <= 1e-7
    assert rel <= 1e-9
    assert dev["status"] == host["status"]
