"""Pose graphs on the device (include/dvo_amd.h, "pose graphs"): dvo_graph_solve against the host definition on every case and size of
tests/pose_graph_reference.py, optimality and ground truth of the device's poses, the contract (a graph's result is byte-identical
whatever the batch, its order, and run to run), the cost of a solve, a second solve, the iteration cap, and the link from the
tracker's information and match records to a graph.

Tolerances: host and device run the same loop, but the device sums over lanes and waves where the host sums in index order, and its
sin / cos / atan2 are the device library's; both stop CG at cg_tol = 1e-6.  Poses agree to 1e-7 (three orders above step_tol), the
final cost, stationary at the solution, to 1e-9 relative."""
import numpy as np
import pytest

import pose_graph_reference as pg

pytestmark = pytest.mark.gpu

NAMES = list(pg.cases())
BATCH = ["ring(65)", "star", "ring(24)", "single"]


_STAGED = {}


def put(h, slot, name):
    if name not in _STAGED:                              # the ctypes edges of a graph are built once
        g = pg.case(name)
        _STAGED[name] = (pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g))
    h.set(slot, *_STAGED[name])


def handle(names):
    from rgbd_odometry_amd import capi
    gs = [pg.case(n) for n in names]
    return capi.DvoPoseGraphs(len(names), sum(g["n"] for g in gs), sum(len(g["i"]) for g in gs))


@pytest.fixture(scope="module")
def device():
    """every case solved in ONE batch: name -> (R, t, report); the handle stays open for the tests that solve again"""
    h = handle(NAMES)
    for k, name in enumerate(NAMES):
        put(h, k, name)
    h.solve(list(range(len(NAMES))))
    assert h.stats() == (1, 1)
    out = {name: pg.from_poses12(h.poses(k)) + (h.report(k),) for k, name in enumerate(NAMES)}
    yield h, out
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_definition(device, name):
    _, out = device
    R, t, rep = out[name]
    Rh, th, want = pg.host_solved(name)
    d = pg.pose_distance(Rh, th, R, t)
    rel = abs(rep["cost"] - want["cost"]) / max(abs(want["cost"]), 1e-300) if want["cost"] > 1e-20 else abs(rep["cost"] - want["cost"])
    print("%s: device iterations %d (host %d), cg %d (host %d), poses %.3e, cost %.3e" % (
        name, rep["iterations"], want["iterations"], rep["cg_iterations"], want["cg_iterations"], d, rel))
    assert rep["status"] == want["status"] == pg.CONVERGED
    assert d <= 1e-7
    assert rel <= 1e-9
    assert rep["cost0"] == pytest.approx(want["cost0"], rel=1e-12, abs=1e-20)
    if rep["lambda_"] >= pg.DEFAULTS["lambda_max"]:       # converged at the cost's rounding floor: the last trial was a rejection
        assert rep["accepted"] < rep["iterations"] and rep["cost_trace"][-1] == rep["cost_trace"][-2]
        print("%s: ended by a rejection at lambda_max" % name)
    assert len(rep["cost_trace"]) == rep["iterations"] + 1 and rep["cost_trace"][0] == rep["cost0"] and rep["cost_trace"][-1] == rep["cost"]
    g = pg.cases()[name]
    f = g["fixed"] != 0
    assert pg.poses12(R[f], t[f]).tobytes() == pg.poses12(g["R0"][f], g["t0"][f]).tobytes()       # fixed nodes: byte for byte


@pytest.mark.parametrize("name", [n for n in NAMES if n != "single"])
def test_optimality_of_the_device_poses(device, name):
    g = pg.cases()[name]
    R, t, _ = device[1][name]
    g0, g1 = pg.gradient(g, g["R0"], g["t0"]), pg.gradient(g, R, t)
    print("%s: gradient %.3e -> %.3e (%.1e)" % (name, g0, g1, g1 / g0))
    assert g0 > 0 and g1 <= 1e-6 * g0


def test_ground_truth_of_the_device_poses(device):
    out = device[1]
    g = pg.cases()["ring_clean(24)"]
    assert pg.pose_distance(*g["truth"], *out["ring_clean(24)"][:2]) <= 1e-7
    g = pg.cases()["pair"]
    R, t, _ = out["pair"]
    assert pg.pose_distance(*pg.compose(g["R0"][:1], g["t0"][:1], g["R"], g["t"]), R[1:], t[1:]) <= 1e-12
    g = pg.cases()["single"]
    assert pg.poses12(*out["single"][:2]).tobytes() == pg.poses12(g["R0"], g["t0"]).tobytes()
    plain = pg.pose_distance(*pg.cases()["outlier_plain"]["truth"], *out["outlier_plain"][:2])
    robust = pg.pose_distance(*pg.cases()["outlier"]["truth"], *out["outlier"][:2])
    print("ground-truth error: plain %.3f, robust %.3f" % (plain, robust))
    assert plain >= 1.0 and robust <= 0.3


def solve_batch(h, names, order):
    """set the named graphs into slots 0 .., solve the slots in `order`: slot -> (pose bytes, report bytes)"""
    for k, name in enumerate(names):
        put(h, k, name)
    h.solve(order)
    assert h.stats() == (1, 1)
    out = {}
    for k in order:
        rep = h.report(k)
        out[names[k]] = (h.poses(k).tobytes(), tuple((key, np.asarray(v).tobytes()) for key, v in sorted(rep.items())))
    return out


def test_contract():
    """a graph's poses and report are byte-identical in a batch, in the reversed batch, alone, and in a second identical run"""
    with handle(BATCH) as h:
        together = solve_batch(h, BATCH, [0, 1, 2, 3])
        again = solve_batch(h, BATCH, [0, 1, 2, 3])
        reverse = solve_batch(h, BATCH, [3, 2, 1, 0])
        assert again == together
        assert reverse == together
        for k, name in enumerate(BATCH):
            assert solve_batch(h, BATCH, [k])[name] == together[name], name
    with handle(BATCH[::-1]) as h:                       # other slots, other offsets in the resident arrays
        assert solve_batch(h, BATCH[::-1], [0, 1, 2, 3]) == together


LARGE = list(pg.large_cases())                       # ring(681): the last graph with its CG vectors in LDS; ring(682), ring(700): in HBM
MIXED = [LARGE[2], "ring(24)", LARGE[0], LARGE[1]]


@pytest.fixture(scope="module")
def mixed():
    """LDS-resident and HBM-resident graphs in one launch, then reversed, then the HBM-resident ones alone"""
    with handle(MIXED) as h:
        together = solve_batch(h, MIXED, [0, 1, 2, 3])
        poses = {name: pg.from_poses12(h.poses(k)) + (h.report(k),) for k, name in enumerate(MIXED)}
        reverse = solve_batch(h, MIXED, [3, 2, 1, 0])
        alone = {MIXED[k]: solve_batch(h, MIXED, [k])[MIXED[k]] for k in (0, 3)}
    return together, reverse, alone, poses


def test_contract_across_the_lds_boundary(mixed):
    together, reverse, alone, _ = mixed
    assert reverse == together
    for name, got in alone.items():
        assert got == together[name], name


@pytest.mark.parametrize("name", LARGE)
def test_graphs_at_and_above_the_lds_boundary(mixed, name):
    """the same bounds as for the smaller cases, on the sizes where the CG vectors leave the LDS"""
    R, t, rep = mixed[3][name]
    Rh, th, want = pg.host_solved(name)
    g = pg.case(name)
    d = pg.pose_distance(Rh, th, R, t)
    rel = abs(rep["cost"] - want["cost"]) / abs(want["cost"])
    g0, g1 = pg.gradient(g, g["R0"], g["t0"]), pg.gradient(g, R, t)
    print("%s: device iterations %d (host %d), cg %d (host %d), poses %.3e, cost %.3e, gradient %.1e" % (
        name, rep["iterations"], want["iterations"], rep["cg_iterations"], want["cg_iterations"], d, rel, g1 / g0))
    assert rep["status"] == want["status"] == pg.CONVERGED
    assert d <= 1e-7 and rel <= 1e-9
    assert g1 <= 1e-6 * g0


def test_second_solve_and_iteration_cap(device):
    from rgbd_odometry_amd import capi
    h, out = device
    k = NAMES.index("ring(65)")
    before = h.poses(k)
    h.solve([k])                                         # nothing was set: the solve continues from the solved poses
    assert h.stats() == (capi.DVO_GRAPH_LAUNCHES, 1)
    rep = h.report(k)
    moved = pg.pose_distance(*pg.from_poses12(before), *pg.from_poses12(h.poses(k)))
    print("second solve: %d iterations, moved %.3e" % (rep["iterations"], moved))
    assert rep["iterations"] <= 2 and rep["status"] == pg.CONVERGED and moved <= 1e-9
    with handle(["ring(24)"]) as h1:
        put(h1, 0, "ring(24)")
        h1.solve([0], capi.DvoGraphParams.default(max_iterations=1))
        rep = h1.report(0)
        want = pg.host_solved("ring(24)")[2]
        assert rep["status"] == pg.MAX_ITERATIONS and rep["iterations"] == 1 and rep["accepted"] == 1
        assert rep["cost"] == pytest.approx(want["cost_trace"][1], rel=1e-9)
        assert rep["cost"] < rep["cost0"]


def test_refusals_change_nothing():
    from rgbd_odometry_amd import capi
    with handle(["ring(24)", "pair"]) as h:
        put(h, 0, "ring(24)")
        P0 = h.poses(0)

        def refused(code, msg, fn, *a):
            with pytest.raises(capi.DvoError) as ei:
                fn(*a)
            assert ei.value.code == code, str(ei.value)
            assert str(ei.value) == "dvo error %d: %s" % (code, msg)
            assert np.array_equal(h.poses(0), P0)

        # the words of every refusal, as dvo_capi_graph.cpp has had them since the handle was added
        COUNT = "count outside [1, max_graphs] or a NULL list"
        refused(capi.DVO_ERR_STATE, "graph 1 was never set (dvo_graph_set)", h.solve, [0, 1])
        refused(capi.DVO_ERR_INVALID, "graph 0 is listed twice", h.solve, [0, 0])
        refused(capi.DVO_ERR_INVALID, COUNT, h.solve, [])
        refused(capi.DVO_ERR_INVALID, COUNT, h.solve, [0, 1, 0])
        refused(capi.DVO_ERR_INVALID, "a listed graph is outside [0, max_graphs)", h.solve, [2])
        refused(capi.DVO_ERR_INVALID, "bad parameters (counts >= 0, lambda_up > 1, lambda_down inside (0, 1), every number finite)", h.solve, [0],
                capi.DvoGraphParams.default(lambda_up=1.0))
        refused(capi.DVO_ERR_STATE, "graph 0 has not been solved since it was set", h.report, 0)
        g = pg.cases()["ring(24)"]
        refused(capi.DVO_ERR_INVALID, "bad graph (NULL array, counts, edge indices, a number that is not finite, an information matrix that is not "
                "symmetric positive definite, unknown flags, or a connected component without a fixed node)", h.set, 0,
                pg.poses12(g["R0"], g["t0"]), np.zeros(24, np.uint8), pg.c_edges(g))
        refused(capi.DVO_ERR_INVALID, "graph outside [0, max_graphs)", h.set, 2, pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g))
        big = pg.cases()["ring(63)"]                                          # more nodes than the handle was created for
        refused(capi.DVO_ERR_INVALID, "the set graphs would hold more nodes or edges than the handle was created for", h.set, 1,
                pg.poses12(big["R0"], big["t0"]), big["fixed"], pg.c_edges(big))
        h.solve([0])
        Rh, th, _ = pg.host_solved("ring(24)")
        assert pg.pose_distance(Rh, th, *pg.from_poses12(h.poses(0))) <= 1e-7


def test_tracker_link():
    """an out-and-back sequence on one stream: odometry edges from the step poses and their information records, one closure to the first
    key frame from dvo_tracker_match, both through dvo_graph_information; the solve must reduce the closure's residual.  A smoke test of
    the link, not of accuracy"""
    from rgbd_odometry_amd import capi
    import frame_gen
    import test_gpu_tracker_archive as TA
    import test_gpu_tracker_information as TI
    n_t = TA.N_T
    seq = TI.sequence(900, n_t, TI.MOTIONS[0])
    # back to one pixel beside where it started: a pixel-identical revisit has sum_eps2 = 0, hence no finite information matrix
    seq[n_t - 1] = frame_gen.camera_frame(900, TI.ROWS, TI.COLS, shift=(1, 0), holes=True)
    tr = TA.make(1)
    try:
        R, t = [np.eye(3)], [np.zeros(3)]                                     # world poses by chaining: T_n = T_key Z
        key, first_id, edges = 0, None, []
        for n in range(n_t):
            Rs, ts, ev = tr.step([0], [seq[n][0]], [seq[n][1]])
            if n == 0:
                first_id = tr.key_frame_id(0)
                continue
            if ev[0] >= 2:
                key = n - 1                                                   # the previous frame became the key frame
            rec = tr.information(0)
            edges.append(capi.DvoGraphEdge.make(key, n, Rs[0], ts[0], capi.graph_information(rec["H"], rec["sum_eps2"], rec["n_visible"])))
            R.append(R[key] @ Rs[0])
            t.append(R[key] @ ts[0] + t[key])
        Rm, tm, recs = tr.match([0], [first_id])
        info = capi.graph_information(recs[0]["H"], recs[0]["sum_eps2"], recs[0]["n_visible"])
        edges.append(capi.DvoGraphEdge.make(0, n_t - 1, Rm[0], tm[0], info))
    finally:
        tr.close()
    R, t = np.array(R), np.array(t)
    fixed = np.zeros(n_t, np.uint8)
    fixed[0] = 1
    closure = pg._graph("closure", R, t, fixed, [0], [n_t - 1], Rm[:1], tm[:1], info[None], [0], None)
    with capi.DvoPoseGraphs(1, n_t, len(edges)) as h:
        h.set(0, pg.poses12(R, t), fixed, edges)
        h.solve([0])
        rep = h.report(0)
        Rs, ts = pg.from_poses12(h.poses(0))
    before = np.linalg.norm(pg.residuals(closure, R, t)[0])
    after = np.linalg.norm(pg.residuals(closure, Rs, ts)[0])
    print("closure residual %.3e -> %.3e, cost %.4g -> %.4g in %d iterations" % (before, after, rep["cost0"], rep["cost"], rep["iterations"]))
    assert rep["status"] == pg.CONVERGED and rep["cost"] < rep["cost0"]
    assert after < before
