"""Marginal covariances of pose graphs on the device (include/dvo_amd.h, "pose graphs", MARGINAL COVARIANCES): dvo_graph_marginals
against the host definition at the sizes where its kernels can go wrong, the contract (a block is byte-identical whatever the batch, its
order, m and the other listed nodes, and run to run), the cost of a call, that a call changes nothing a solve can see, a graph set and
never solved, fixed nodes, every refusal, and the gate on a held-out loop closure of a tracked sequence.

Sizes: pair (2 nodes); ring(63), ring(64), ring(65) around a wave; ring(257), one node beyond a workgroup's threads; ring(681) and
ring(682), the last size with the CG vectors in LDS and the first with them in the workspace; star with its degree-300 node; two_fixed.

Tolerance: mr.TOLERANCE, 100 times the distance of the HOST definition from the dense inverse measured on the CPU
(tests/pose_graph_marginals_reference.py; 4.42e-13 measured).  Host and device run the same loop at cg_tol = 1e-12; the device sums over
lanes and waves where the host sums in index order, and the margin covers that and nothing else."""
import numpy as np
import pytest

import pose_graph_marginals_reference as mr
import pose_graph_reference as pg

pytestmark = pytest.mark.gpu

LARGE = list(pg.large_cases())                       # ring(681), ring(682), ring(700)
CASES = ["pair", "ring(63)", "ring(64)", "ring(65)", "ring(257)", LARGE[0], LARGE[1], "star", "two_fixed"]
DENSE = ["pair", "ring(63)", "ring(64)", "ring(65)"]
NODES = {"pair": [1, 0], "star": [0, 300], "two_fixed": [11, 12]}       # pair and two_fixed list a fixed node

_OWN = {}


def case(name):
    if name == "ring(257)":
        if name not in _OWN:
            _OWN[name] = pg.ring(257)
        return _OWN[name]
    return pg.case(name)


def nodes_of(name):
    return NODES.get(name, [1, case(name)["n"] - 1])


_STAGED = {}


def staged(name):
    if name not in _STAGED:                              # the ctypes edges of a graph are built once
        g = case(name)
        _STAGED[name] = (pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g))
    return _STAGED[name]


def handle(names):
    from rgbd_odometry_amd import capi
    gs = [case(n) for n in names]
    return capi.DvoPoseGraphs(len(names), sum(g["n"] for g in gs), sum(len(g["i"]) for g in gs))


def tight():
    from rgbd_odometry_amd import capi
    return capi.DvoGraphParams.default(cg_tol=mr.CG_TOL)


def as_bytes(cov, reps):
    return [(cov[k].tobytes(), tuple(sorted((key, np.asarray(v).tobytes()) for key, v in reps[k].items()))) for k in range(len(reps))]


@pytest.fixture(scope="module")
def device():
    """every case set and solved in one batch, then ONE marginals call for all of them with m = 2 at cg_tol = 1e-12; the handle stays
    open for the tests that ask again"""
    from rgbd_odometry_amd import capi
    h = handle(CASES)
    for k, name in enumerate(CASES):
        h.set(k, *staged(name))
    every = list(range(len(CASES)))
    h.solve(every)
    nodes = [nodes_of(name) for name in CASES]
    cov, reps = h.marginals(every, nodes, tight())
    assert h.stats() == (capi.DVO_GRAPH_MARGINAL_LAUNCHES, 1)
    poses = {name: h.poses(k) for k, name in enumerate(CASES)}
    yield h, cov, reps, poses, nodes
    h.close()


_HOST = {}


def host_at(name, P, nodes):
    """the host definition at the poses P, once per case"""
    from rgbd_odometry_amd import capi
    key = (name, tuple(nodes), P.tobytes())
    if key not in _HOST:
        _HOST[key] = capi.pose_graph_marginals_host(P, staged(name)[1], staged(name)[2], nodes, tight())
    return _HOST[key]


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_host_definition(device, name):
    _, cov, reps, poses, nodes = device
    k = CASES.index(name)
    want, wrep = host_at(name, poses[name], nodes[k])
    d = mr.distance(cov[k], want)
    print("%s nodes %s: device against host %.3e; status %d (host %d), longest column %d (host %d), residual %.1e" % (
        name, nodes[k], d, reps[k]["status"], wrep["status"], reps[k]["cg_iterations_max"], wrep["cg_iterations_max"], reps[k]["worst_residual"]))
    assert reps[k]["status"] == wrep["status"] == pg.CONVERGED
    assert reps[k]["worst_residual"] <= 1e-12
    assert d <= mr.TOLERANCE
    assert cov[k].tobytes() == cov[k].T.tobytes()
    g = case(name)
    for a, c in enumerate(nodes[k]):
        if g["fixed"][c]:
            assert not cov[k][6 * a:6 * a + 6].any() and not cov[k][:, 6 * a:6 * a + 6].any()
    if name in DENSE:
        R, t = pg.from_poses12(poses[name])
        dd = mr.distance(cov[k], mr.joint(mr.dense_covariance(g, R, t), nodes[k]))
        print("%s: device against the dense inverse %.3e" % (name, dd))
        assert dd <= mr.TOLERANCE


def test_determinism(device):
    """the batch against a second run, the reversed batch and each case alone; and a block against the same block of another query, in
    another batch, at another position"""
    h, cov, reps, _, nodes = device
    together = as_bytes(cov, reps)
    every = list(range(len(CASES)))
    assert as_bytes(*h.marginals(every, nodes, tight())) == together
    rev = every[::-1]
    assert as_bytes(*h.marginals(rev, [nodes[k] for k in rev], tight())) == together[::-1]
    for k in every:
        assert as_bytes(*h.marginals([k], [nodes[k]], tight())) == [together[k]], CASES[k]
    # (i, j) of the query (i, j) is (i, j) of the query (j, k, i)
    trio = [CASES.index("ring(65)"), CASES.index(LARGE[1]), CASES.index("star")]
    a, _ = h.marginals(trio, [[5, 17], [5, 600], [0, 7]], tight())
    b, _ = h.marginals(trio[::-1], [[7, 300, 0], [600, 9, 5], [17, 9, 5]], tight())
    for x, y in zip(a, b[::-1]):
        assert x[0:6, 6:12].tobytes() == y[12:18, 0:6].tobytes()
        assert x[0:6, 0:6].tobytes() == y[12:18, 12:18].tobytes() and x[6:12, 6:12].tobytes() == y[0:6, 0:6].tobytes()


def test_cost(device):
    from rgbd_odometry_amd import capi
    h, _, _, _, nodes = device
    assert capi.DVO_GRAPH_MARGINAL_LAUNCHES == 2
    h.marginals([3], [nodes[3]])
    assert h.stats() == (capi.DVO_GRAPH_MARGINAL_LAUNCHES, 1)
    h.marginals(list(range(len(CASES))), nodes)
    assert h.stats() == (capi.DVO_GRAPH_MARGINAL_LAUNCHES, 1)
    h.marginals([0, 7], [[1], [300]])                    # another m
    assert h.stats() == (capi.DVO_GRAPH_MARGINAL_LAUNCHES, 1)


TWINS = ["ring(65)", LARGE[1], "star"]


def state(h, slots):
    out = []
    for k in slots:
        rep = h.report(k)
        out.append((h.poses(k).tobytes(), tuple(sorted((key, np.asarray(v).tobytes()) for key, v in rep.items()))))
    return out


def test_a_call_changes_nothing_a_solve_can_see():
    slots = list(range(len(TWINS)))
    with handle(TWINS) as h, handle(TWINS) as twin:
        for x in (h, twin):
            for k, name in enumerate(TWINS):
                x.set(k, *staged(name))
            x.solve(slots)
        before = state(h, slots)
        assert before == state(twin, slots)
        h.marginals(slots, [nodes_of(n) for n in TWINS], tight())
        h.marginals([1], [[3, 4, 5]])
        assert state(h, slots) == before                 # poses and last report are what they were
        h.solve(slots)
        twin.solve(slots)
        assert state(h, slots) == state(twin, slots)     # and the next solve is the twin's, byte for byte


def test_a_graph_set_and_never_solved():
    from rgbd_odometry_amd import capi
    slots = list(range(len(TWINS)))
    with handle(TWINS) as h, handle(TWINS) as twin:
        for x in (h, twin):
            for k, name in enumerate(TWINS):
                x.set(k, *staged(name))
        nodes = [nodes_of(n) for n in TWINS]
        cov, reps = h.marginals(slots, nodes, tight())
        assert h.stats() == (capi.DVO_GRAPH_MARGINAL_LAUNCHES, 1)
        for k, name in enumerate(TWINS):
            assert np.array_equal(h.poses(k), staged(name)[0])
            want, wrep = host_at(name, staged(name)[0], nodes[k])
            d = mr.distance(cov[k], want)
            print("%s at the set poses: device against host %.3e, status %d" % (name, d, reps[k]["status"]))
            assert reps[k]["status"] == wrep["status"] == pg.CONVERGED and d <= mr.TOLERANCE
            with pytest.raises(capi.DvoError) as ei:     # still not solved
                h.report(k)
            assert ei.value.code == capi.DVO_ERR_STATE
        h.solve(slots)
        twin.solve(slots)
        assert state(h, slots) == state(twin, slots)


def test_fixed_nodes_and_refusals(device):
    from rgbd_odometry_amd import capi
    h, cov, reps, _, nodes = device
    k = CASES.index("two_fixed")
    one, rep = h.marginals([k], [[12]], tight())         # a listed fixed node alone: zeros, no iterations
    assert not one.any() and rep[0]["cg_iterations"] == 0 and rep[0]["status"] == pg.CONVERGED and rep[0]["worst_residual"] == 0.0
    # a batch whose graphs are all fully fixed
    g = case("ring(65)")
    with capi.DvoPoseGraphs(2, 70, 80) as hf:
        hf.set(0, staged("ring(65)")[0], np.ones(65, np.uint8), staged("ring(65)")[2])
        hf.set(1, staged("pair")[0], np.ones(2, np.uint8), [])
        c2, r2 = hf.marginals([0, 1], [[3, 64], [0, 1]])
        assert hf.stats() == (capi.DVO_GRAPH_MARGINAL_LAUNCHES, 1)
        assert not c2.any() and all(r["cg_iterations"] == 0 and r["status"] == pg.CONVERGED for r in r2)
    # refusals: outputs and handle state unchanged
    with handle(["ring(24)", "pair"]) as hr:
        hr.set(0, *staged("ring(24)"))
        hr.solve([0])
        before = state(hr, [0])
        lib = capi.load_library()
        import ctypes as C

        def refused(code, graphs, nodes, m, params=None, null=()):
            gs = (C.c_int * max(len(graphs), 1))(*graphs)
            q = (C.c_int * max(len(nodes), 1))(*nodes)
            out = np.full((6 * 17) ** 2 * 2, 7.5)
            rp = (capi.DvoGraphMarginalReport * 2)()
            C.memset(rp, 0x5A, C.sizeof(rp))
            rp0 = bytes(rp)
            rc = lib.dvo_graph_marginals(hr._h, C.byref(params) if params is not None else None, len(graphs), None if "graphs" in null else gs, m,
                                         None if "nodes" in null else q, None if "cov" in null else capi._ptr(out), None if "reports" in null else rp)
            assert rc == code, (graphs, nodes, m, rc)
            assert np.all(out == 7.5) and bytes(rp) == rp0 and state(hr, [0]) == before

        refused(capi.DVO_ERR_STATE, [0, 1], [1, 2, 0, 1], 2)                   # graph 1 was never set
        refused(capi.DVO_ERR_INVALID, [0], [3, 3], 2)                          # a node listed twice
        refused(capi.DVO_ERR_INVALID, [0], list(range(17)), 17)
        refused(capi.DVO_ERR_INVALID, [0], [], 0)
        refused(capi.DVO_ERR_INVALID, [0, 0], [1, 2, 1, 2], 2)                 # a graph listed twice
        refused(capi.DVO_ERR_INVALID, [0], [1, 24], 2)                         # a node out of range
        refused(capi.DVO_ERR_INVALID, [0], [-1, 2], 2)
        refused(capi.DVO_ERR_INVALID, [2], [1, 2], 2)
        refused(capi.DVO_ERR_INVALID, [], [1, 2], 2)
        refused(capi.DVO_ERR_INVALID, [0], [1, 2], 2, params=capi.DvoGraphParams.default(lambda_up=1.0))
        refused(capi.DVO_ERR_INVALID, [0], [1, 2], 2, params=capi.DvoGraphParams.default(cg_tol=float("nan")))
        for null in ("graphs", "nodes", "cov", "reports"):
            refused(capi.DVO_ERR_INVALID, [0], [1, 2], 2, null=(null,))
        ok, _ = hr.marginals([0], [[1, 2]], tight())
        want, _ = host_at("ring(24)", hr.poses(0), [1, 2])
        assert mr.distance(ok[0], want) <= mr.TOLERANCE


def test_gate_on_a_held_out_closure():
    """the out-and-back sequence of the tracker-link test: odometry edges from the step poses and their information records, the closure
    to the first key frame from dvo_tracker_match held out of the graph.  Under the joint covariance of its two end nodes the true
    closure is less surprising than the same closure displaced by 0.5 m.  The ordering is the test; the unit of the information is
    relative (dvo_graph_information)"""
    from rgbd_odometry_amd import capi
    import frame_gen
    import test_gpu_tracker_archive as TA
    import test_gpu_tracker_information as TI
    n_t = TA.N_T
    seq = TI.sequence(900, n_t, TI.MOTIONS[0])
    seq[n_t - 1] = frame_gen.camera_frame(900, TI.ROWS, TI.COLS, shift=(1, 0), holes=True)
    tr = TA.make(1)
    try:
        R, t = [np.eye(3)], [np.zeros(3)]
        key, first_id, edges = 0, None, []
        for n in range(n_t):
            Rs, ts, ev = tr.step([0], [seq[n][0]], [seq[n][1]])
            if n == 0:
                first_id = tr.key_frame_id(0)
                continue
            if ev[0] >= 2:
                key = n - 1
            rec = tr.information(0)
            edges.append(capi.DvoGraphEdge.make(key, n, Rs[0], ts[0], capi.graph_information(rec["H"], rec["sum_eps2"], rec["n_visible"])))
            R.append(R[key] @ Rs[0])
            t.append(R[key] @ ts[0] + t[key])
        Rm, tm, recs = tr.match([0], [first_id])
        info = capi.graph_information(recs[0]["H"], recs[0]["sum_eps2"], recs[0]["n_visible"])
    finally:
        tr.close()
    fixed = np.zeros(n_t, np.uint8)
    fixed[0] = 1
    with capi.DvoPoseGraphs(1, n_t, len(edges)) as h:
        h.set(0, pg.poses12(np.array(R), np.array(t)), fixed, edges)
        h.solve([0])
        P = h.poses(0)
        cov, rep = h.marginals([0], [[0, n_t - 1]], tight())
    assert rep[0]["status"] == pg.CONVERGED
    assert not cov[0][:6].any() and (np.diag(cov[0])[6:] > 0.0).all()                    # node 0 is the gauge; the last node is uncertain
    true = capi.DvoGraphEdge.make(0, n_t - 1, Rm[0], tm[0], info)
    wrong = capi.DvoGraphEdge.make(0, n_t - 1, Rm[0], tm[0] + np.array([0.5, 0.0, 0.0]), info)
    c_true = capi.pose_graph_edge_chi2(P[0], P[n_t - 1], cov[0], true)[2]
    c_wrong = capi.pose_graph_edge_chi2(P[0], P[n_t - 1], cov[0], wrong)[2]
    print("chi2 of the held-out closure %.4g, displaced by 0.5 m %.4g" % (c_true, c_wrong))
    assert c_true < c_wrong
