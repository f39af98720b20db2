"""Marginal covariances of pose graphs on the CPU (include/dvo_amd.h, "pose graphs", MARGINAL COVARIANCES): dvo_graph_marginals_host
against the dense inverse of the Gauss-Newton matrix (tests/pose_graph_marginals_reference.py) on every case, its exact properties, its
stop rules, every refusal, dvo_graph_edge_chi2 against its numpy restatement, the bindings' layouts, and the definition's own code
(rgbd_odometry_amd/csrc/dvo_pose_graph.h) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/host/pose_graph_marginals_main.cpp).  No GPU: the host definition needs neither a device nor a handle.

Tolerance: mr.TOLERANCE is 100 times the worst distance of the host definition from the dense inverse measured over these cases
(mr.HOST_AGAINST_DENSE_MEASURED, 4.42e-13 on `star`, condition number 3.7e6; profiles/pose_graph_marginals/README.md), relative to the
largest entry of the joint block."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_marginals_reference as mr
import pose_graph_reference as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["pair", "ring(2)", "ring(24)", "ring_aniso(24)", "ring_clean(24)", "outlier", "outlier_plain", "two_fixed", "star", "ring(63)",
         "ring(64)", "ring(65)", "ring(513)"]


def poses_at(name, at):
    g = pg.cases()[name]
    return (g["R0"], g["t0"]) if at == "start" else pg.solved(name)[:2]


_EDGES = {}


def host(name, at, nodes, **params):
    """dvo_graph_marginals_host on a case at its start or solved poses: (cov, report)"""
    from rgbd_odometry_amd import capi
    g = pg.cases()[name]
    if name not in _EDGES:
        _EDGES[name] = pg.c_edges(g)
    R, t = poses_at(name, at)
    return capi.pose_graph_marginals_host(pg.poses12(R, t), g["fixed"], _EDGES[name], nodes, capi.DvoGraphParams.default(**params))


@pytest.mark.parametrize("at", ["start", "solved"])
@pytest.mark.parametrize("name", CASES)
def test_host_definition_against_the_dense_inverse(name, at):
    g = pg.cases()[name]
    R, t = poses_at(name, at)
    if name == "outlier" and at == "start":          # the Huber weight of the wrong chord is in play
        s = np.sqrt(pg._s2(g["info"], pg.residuals(g, R, t)[0]))
        assert (s[g["flags"] != 0] > pg.DEFAULTS["huber_delta"]).any()
    D = mr.dense_covariance(g, R, t, key=(name, at))
    queries = mr.queries(g)
    if g["n"] > 500 and at == "start":               # the long columns: six of them at the start poses, all of the queries at the solved ones
        queries = queries[:1]
    worst = 0.0
    for q in queries:
        cov, rep = host(name, at, q, cg_tol=mr.CG_TOL)
        d = mr.distance(cov, mr.joint(D, q))
        print("%s at %s, nodes %s: %.3e, longest column %d of %d, residual %.1e" % (name, at, q, d, rep["cg_iterations_max"], 12 * g["n"], rep["worst_residual"]))
        assert rep["status"] == pg.CONVERGED and rep["worst_residual"] <= 1e-12
        assert cov.tobytes() == cov.T.tobytes()
        worst = max(worst, d)
    assert worst <= mr.TOLERANCE


def test_exact_properties():
    from rgbd_odometry_amd import capi
    for name in ("ring(24)", "star", "two_fixed", "ring_aniso(24)"):
        g = pg.cases()[name]
        q = mr.queries(g)[-1]
        cov, rep = host(name, "solved", q, cg_tol=mr.CG_TOL)
        assert cov.tobytes() == cov.T.tobytes()                             # symmetric byte for byte
        assert np.linalg.eigvalsh(cov).min() >= -mr.TOLERANCE * np.abs(cov).max()
        for a, c in enumerate(q):
            if g["fixed"][c]:
                assert not cov[6 * a:6 * a + 6].any() and not cov[:, 6 * a:6 * a + 6].any()
    g = pg.cases()["two_fixed"]
    assert g["fixed"][12] and mr.queries(g)[-1][1] == 12                    # one listed node is fixed
    # every node fixed: all zero, no iterations
    g = pg.cases()["ring(24)"]
    cov, rep = capi.pose_graph_marginals_host(pg.poses12(g["R0"], g["t0"]), np.ones(24, np.uint8), pg.c_edges(g), [3, 4])
    assert not cov.any() and rep["cg_iterations"] == 0 and rep["cg_iterations_max"] == 0 and rep["status"] == pg.CONVERGED
    cov, rep = capi.pose_graph_marginals_host(pg.poses12(g["R0"], g["t0"]), np.ones(24, np.uint8), [], [3])
    assert not cov.any() and rep["cg_iterations"] == 0 and rep["status"] == pg.CONVERGED
    # pair: one free node and one edge
    g = pg.cases()["pair"]
    for at in ("start", "solved"):
        R, t = poses_at("pair", at)
        cov, _ = host("pair", at, [1], cg_tol=mr.CG_TOL)
        _, _, Jj = mr.edge_jacobians(g, 0, R, t)
        want = np.linalg.inv(Jj.T @ g["info"][0] @ Jj)
        assert mr.distance(cov, want) <= mr.TOLERANCE
    # a block depends on its two nodes alone: (i, j) of the query (i, j) is, byte for byte, (i, j) of the query (j, k, i)
    for name, (i, j, k) in (("ring(24)", (5, 17, 9)), ("star", (0, 7, 300)), ("two_fixed", (11, 12, 3))):
        a, _ = host(name, "solved", [i, j], cg_tol=mr.CG_TOL)
        b, _ = host(name, "solved", [j, k, i], cg_tol=mr.CG_TOL)
        assert a[0:6, 6:12].tobytes() == b[12:18, 0:6].tobytes(), name
        assert a[0:6, 0:6].tobytes() == b[12:18, 12:18].tobytes() and a[6:12, 6:12].tobytes() == b[0:6, 0:6].tobytes(), name
        one, _ = host(name, "solved", [i], cg_tol=mr.CG_TOL)
        assert one.tobytes() == np.ascontiguousarray(a[0:6, 0:6]).tobytes(), name


def test_stop_rules():
    for name in ("ring(24)", "star", "ring(65)"):
        q = mr.queries(pg.cases()[name])[-1]
        cov, rep = host(name, "solved", q)                                   # the default cg_tol, 1e-6
        assert rep["status"] == pg.CONVERGED and rep["worst_residual"] <= 1e-6
        assert 0 < rep["cg_iterations_max"] <= rep["cg_iterations"]
    cov, rep = host("ring(24)", "solved", [1, 2], cg_max_iterations=3, cg_tol=mr.CG_TOL)
    assert rep["status"] == pg.MAX_ITERATIONS and np.isfinite(cov).all() and cov.any()
    assert rep["cg_iterations_max"] == 3 and rep["cg_iterations"] == 36


def test_refusals():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    g = pg.cases()["ring(24)"]
    P0 = pg.poses12(g["R0"], g["t0"])
    n, ne = g["n"], len(g["i"])
    good = pg.c_edges(g)

    def call(edit=None, params=None, poses=None, fixed=None, n_nodes=n, n_edges=ne, nodes=(3, 4), m=None, null=()):
        P = np.ascontiguousarray(P0 if poses is None else poses)
        f = np.ascontiguousarray(g["fixed"] if fixed is None else fixed, dtype=np.uint8)
        edges = [capi.DvoGraphEdge.make(e.i, e.j, np.array(e.R).reshape(3, 3).T, e.t, np.array(e.info).reshape(6, 6), bool(e.flags)) for e in good]
        if edit:
            edit(edges)
        arr = (capi.DvoGraphEdge * max(len(edges), 1))(*edges)
        p = capi.DvoGraphParams.default(**(params or {}))
        q = (C.c_int * max(len(nodes), 1))(*nodes)
        m = len(nodes) if m is None else m
        rep = capi.DvoGraphMarginalReport()
        C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
        rep0 = bytes(rep)
        cov = np.full((6 * 17) ** 2, 1.2345e300)
        rc = lib.dvo_graph_marginals_host(C.byref(p), n_nodes, None if "poses" in null else capi._ptr(P), None if "fixed" in null else capi._ptr(f),
                                          n_edges, None if "edges" in null else arr, m, None if "nodes" in null else q,
                                          None if "cov" in null else capi._ptr(cov), None if "report" in null else C.byref(rep))
        if rc != capi.DVO_OK:
            assert bytes(rep) == rep0 and np.all(cov == 1.2345e300), "a refused call must write nothing"
        else:
            assert np.all(cov[(6 * m) ** 2:] == 1.2345e300)
        return rc

    def ed(k, field, index, value):
        def edit(edges):
            if index is None:
                setattr(edges[k], field, value)
            else:
                getattr(edges[k], field)[index] = value
        return edit

    assert call() == capi.DVO_OK
    assert call(nodes=tuple(range(16))) == capi.DVO_OK
    assert call(nodes=(0,)) == capi.DVO_OK                                    # a listed fixed node is fine
    bad = [dict(null=("poses",)), dict(null=("fixed",)), dict(null=("report",)), dict(null=("edges",)), dict(null=("nodes",)), dict(null=("cov",)),
           dict(n_nodes=0), dict(n_nodes=-1), dict(n_nodes=capi.DVO_GRAPH_MAX_NODES + 1), dict(n_edges=-1), dict(n_edges=capi.DVO_GRAPH_MAX_EDGES + 1),
           dict(edit=ed(5, "i", None, -1)), dict(edit=ed(5, "j", None, n)), dict(edit=ed(5, "j", None, 5)), dict(n_nodes=n - 1),
           dict(edit=ed(3, "flags", None, 2)), dict(edit=ed(2, "info", 1, 3.0)), dict(edit=ed(2, "info", 0, -1.0)), dict(edit=ed(2, "info", 35, 0.0)),
           dict(fixed=np.zeros(n, np.uint8)), dict(n_edges=0),
           dict(params=dict(max_iterations=-1)), dict(params=dict(cg_max_iterations=-1)), dict(params=dict(lambda_up=1.0)),
           dict(params=dict(lambda_down=1.0)), dict(params=dict(lambda0=-1.0)), dict(params=dict(cg_tol=float("nan"))),
           dict(params=dict(huber_delta=float("inf"))), dict(params=dict(lambda_max=1e-13)),
           dict(nodes=(), m=0), dict(m=-1), dict(nodes=tuple(range(17))), dict(nodes=(3, 3)), dict(nodes=(3, 4, 3)), dict(nodes=(-1,)), dict(nodes=(n,)),
           dict(nodes=(3, n))]
    for v in (float("nan"), float("inf")):
        for idx in (0, 12 * n - 1):
            P = P0.copy()
            P.ravel()[idx] = v
            bad.append(dict(poses=P))
        bad += [dict(edit=ed(7, "R", 4, v)), dict(edit=ed(7, "t", 2, v)), dict(edit=ed(7, "info", 14, v))]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
    assert call(n_edges=0, fixed=np.ones(n, np.uint8)) == capi.DVO_OK         # no edges, every node fixed: valid, zeros
    with pytest.raises(capi.DvoError) as ei:
        capi.pose_graph_marginals_host(P0, g["fixed"], good, [3, 3])
    assert ei.value.code == capi.DVO_ERR_INVALID


def test_edge_chi2_against_the_restatement():
    """r, S and chi2 of every edge of ring(24) under the host marginals of its end nodes.  Both sides are given the same cov, so they
    differ by the rounding of two 6 x 6 inversions and a few products: a small multiple of eps cond(S), and cond(S) stays below 1e4 here
    (asserted), hence below 1e-11; 1e-9 is asserted"""
    from rgbd_odometry_amd import capi
    g = pg.cases()["ring(24)"]
    R, t = pg.solved("ring(24)")[:2]
    P = pg.poses12(R, t)
    edges = pg.c_edges(g)
    worst = 0.0
    for e in range(len(g["i"])):
        i, j = int(g["i"][e]), int(g["j"][e])
        cov, _ = host("ring(24)", "solved", [i, j], cg_tol=mr.CG_TOL)
        r, S, chi2 = capi.pose_graph_edge_chi2(P[i], P[j], cov, edges[e])
        rw, Sw, cw = mr.edge_chi2(g, e, R, t, cov)
        assert np.linalg.cond(Sw) < 1e4
        d = max(np.abs(r - rw).max() / np.abs(rw).max(), np.abs(S - Sw).max() / np.abs(Sw).max(), abs(chi2 - cw) / cw)
        worst = max(worst, d)
        assert d <= 1e-9, (e, d)
        # no covariance: S = Omega^-1 and chi2 is the edge's s^2
        r0, S0, c0 = capi.pose_graph_edge_chi2(P[i], P[j], None, edges[e])
        s2 = float(pg._s2(g["info"][e:e + 1], rw[None])[0])
        assert abs(c0 - s2) <= 1e-12 * s2 and np.array_equal(r0, r)
        assert chi2 < c0                                                      # an uncertain pair of poses makes the same residual less surprising
        assert capi.pose_graph_edge_chi2(P[i], P[j], 4.0 * cov, edges[e])[2] < chi2
    print("edge_chi2 against the restatement: %.3e" % worst)


def test_edge_chi2_refusals():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    g = pg.cases()["ring(24)"]
    P = pg.poses12(g["R0"], g["t0"])
    e = pg.c_edges(g)[1]
    cov, _ = host("ring(24)", "start", [1, 2])

    def call(pi=P[1], pj=P[2], cv=cov, edge=e, outs=(True, True, True)):
        r, S, c = np.full(6, 7.0), np.full(36, 7.0), C.c_double(7.0)
        as_c = lambda a: None if a is None else capi._ptr(np.ascontiguousarray(a, dtype=np.float64))
        rc = lib.dvo_graph_edge_chi2(as_c(pi), as_c(pj), as_c(cv), None if edge is None else C.byref(edge), capi._ptr(r) if outs[0] else None,
                                     capi._ptr(S) if outs[1] else None, C.byref(c) if outs[2] else None)
        if rc != capi.DVO_OK:
            assert np.all(r == 7.0) and np.all(S == 7.0) and c.value == 7.0, "a refused call must write nothing"
        return rc, c.value

    rc, full = call()
    assert rc == capi.DVO_OK
    for outs in ((False, True, True), (True, False, True), (False, False, True)):      # any output pointer may be NULL
        assert call(outs=outs) == (capi.DVO_OK, full)
    assert call(outs=(True, True, False))[0] == capi.DVO_OK and call(outs=(False, False, False))[0] == capi.DVO_OK

    def edited(field, index, value):
        x = capi.DvoGraphEdge.from_buffer_copy(bytes(e))
        getattr(x, field)[index] = value
        return x

    def poked(a, index, value):
        b = np.array(a, dtype=np.float64)
        b.ravel()[index] = value
        return b

    bad = [dict(pi=None), dict(pj=None), dict(edge=None), dict(edge=edited("info", 0, -1.0)), dict(edge=edited("info", 35, 0.0)),
           dict(cv=-1e6 * np.eye(12))]                                        # S without a Cholesky factor
    for v in (float("nan"), float("inf")):
        bad += [dict(pi=poked(P[1], 3, v)), dict(pj=poked(P[2], 11, v)), dict(cv=poked(cov, 143, v)), dict(edge=edited("R", 2, v)),
                dict(edge=edited("t", 1, v)), dict(edge=edited("info", 7, v))]
    for kw in bad:
        assert call(**kw)[0] == capi.DVO_ERR_INVALID, kw
    flagged = capi.DvoGraphEdge.from_buffer_copy(bytes(e))
    flagged.flags = capi.DVO_GRAPH_EDGE_ROBUST                                # the robust flag plays no part
    assert call(edge=flagged) == (capi.DVO_OK, full)
    with pytest.raises(capi.DvoError):
        capi.pose_graph_edge_chi2(P[1], P[2], -1e6 * np.eye(12), e)


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in ("dvo_graph_marginals_host", "dvo_graph_marginals", "dvo_graph_edge_chi2"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    for macro in ("DVO_GRAPH_MARGINAL_MAX_NODES", "DVO_GRAPH_MARGINAL_LAUNCHES"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == getattr(capi, macro), macro
    assert capi.DVO_GRAPH_MARGINAL_MAX_NODES == 16
    # the report is declared twice under one guard (the public header and the definition's own): the two texts must be the same
    own = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_pose_graph.h")).read(), flags=re.S)
    pat = r"#ifndef DVO_GRAPH_MARGINAL_TYPES_DEFINED_.*?#endif"
    assert re.search(pat, text, re.S).group(0).split() == re.search(pat, own, re.S).group(0).split()
    launch = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_pose_graph_launch.h")).read()
    assert int(re.search(r"kMarginalLaunches\s*=\s*(\d+)", launch).group(1)) == capi.DVO_GRAPH_MARGINAL_LAUNCHES


def test_report_layout_matches_header(tmp_path):
    from rgbd_odometry_amd import capi
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu", '
                   'sizeof(dvo_graph_marginal_report), offsetof(dvo_graph_marginal_report, worst_residual), '
                   'offsetof(dvo_graph_marginal_report, cg_iterations), offsetof(dvo_graph_marginal_report, cg_iterations_max), '
                   'offsetof(dvo_graph_marginal_report, status));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = tuple(int(x) for x in subprocess.check_output([exe]).split())
    M = capi.DvoGraphMarginalReport
    assert got == (C.sizeof(M), M.worst_residual.offset, M.cg_iterations.offset, M.cg_iterations_max.offset, M.status.offset)


def test_device_marginals_need_a_device():
    """dvo_graph_marginals runs on a handle, and without a device there is none: no CPU path behind it"""
    import torch
    from rgbd_odometry_amd import capi
    if torch.cuda.is_available():
        with capi.DvoPoseGraphs(1, 8, 8) as h:
            with pytest.raises(capi.DvoError) as ei:
                h.marginals([0], [[0]])
            assert ei.value.code == capi.DVO_ERR_STATE                        # never set
        return
    with pytest.raises(capi.DvoError) as ei:
        capi.DvoPoseGraphs(1, 8, 8)
    assert ei.value.code == capi.DVO_ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)
    q, g1 = (C.c_int * 1)(0), (C.c_int * 1)(0)
    cov, rep = np.zeros(36), capi.DvoGraphMarginalReport()
    assert capi.load_library().dvo_graph_marginals(None, None, 1, g1, 1, q, capi._ptr(cov), C.byref(rep)) == capi.DVO_ERR_INVALID


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_graph_marginals")
    exe = str(d / "pose_graph_marginals_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "pose_graph_marginals_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/pose_graph_marginals_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def _case_bytes(g, params, nodes):
    edges = pg.c_edges(g)
    return (struct.pack("<iii", g["n"], len(edges), len(nodes)) + bytes(params) + pg.poses12(g["R0"], g["t0"]).tobytes() +
            np.ascontiguousarray(g["fixed"], dtype=np.uint8).tobytes() + b"".join(bytes(e) for e in edges) + struct.pack("<%di" % len(nodes), *nodes))


def test_definition_under_sanitizers(host_program):
    """the same code the library compiles, with every array allocated to its exact size: reports, covariances and the gate's outputs
    byte-equal to the library's entry points, clean under -fsanitize=address,undefined; a refused graph is refused there too"""
    from rgbd_odometry_amd import capi
    d, exe = host_program
    p = capi.DvoGraphParams.default(cg_tol=mr.CG_TOL)
    free = dict(pg.cases()["ring(24)"])
    free["fixed"] = np.zeros(24, np.uint8)
    runs = [("ring(24)", pg.cases()["ring(24)"], [1, 2]), ("two_fixed", pg.cases()["two_fixed"], [11, 12]),
            ("ring(24)", pg.cases()["ring(24)"], [23, 5, 6]), ("free", free, [1, 2])]
    path = str(d / "cases.bin")
    open(path, "wb").write(struct.pack("<i", len(runs)) + b"".join(_case_bytes(g, p, q) for _, g, q in runs))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    at = 0
    for k, (name, g, q) in enumerate(runs):
        if name == "free":
            assert lines[at] == "case %d refused" % k
            at += 1
            continue
        assert lines[at] == "case %d ok" % k, (name, lines[at])
        rep = capi.DvoGraphMarginalReport.from_buffer_copy(bytes.fromhex(lines[at + 1]))
        cov = np.frombuffer(bytes.fromhex(lines[at + 2]), np.float64)
        P = pg.poses12(g["R0"], g["t0"])
        want, wrep = capi.pose_graph_marginals_host(P, g["fixed"], pg.c_edges(g), q, p)
        assert cov.tobytes() == want.tobytes(), name
        assert (rep.worst_residual, rep.cg_iterations, rep.cg_iterations_max, rep.status) == (
            wrep["worst_residual"], wrep["cg_iterations"], wrep["cg_iterations_max"], wrep["status"]), name
        at += 3
        if len(q) != 2:
            assert lines[at] == "gate none"
            at += 1
            continue
        assert lines[at] == "gate ok", (name, lines[at])
        e = [k for k in range(len(g["i"])) if (g["i"][k], g["j"][k]) == tuple(q)][0]
        r, S, chi2 = capi.pose_graph_edge_chi2(P[q[0]], P[q[1]], want, pg.c_edges(g)[e])
        assert bytes.fromhex(lines[at + 1]) == r.tobytes() and bytes.fromhex(lines[at + 2]) == S.tobytes(), name
        assert bytes.fromhex(lines[at + 3]) == struct.pack("<d", chi2), name
        at += 4
    assert at == len(lines)


def test_cpp_mirror_builds_and_gates(tmp_path):
    """include/dvo_amd.hpp's PoseGraphs::marginals and edgeChi2: tests/host/pose_graph_marginals_hpp_main.cpp compiles with plain g++ and
    every warning on and links against the library; the gate runs on the host, and through the device where there is one"""
    import torch
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "pose_graph_marginals_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "pose_graph_marginals_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    tok = lines[0].split()
    assert tok[:2] == ["host", "chi2"] and abs(float(tok[2]) - 0.16) <= 1e-6   # 400 * 0.02^2
    if torch.cuda.is_available():
        tok = lines[1].split()
        assert tok[:3] == ["device", "status", "0"] and 0.0 <= float(tok[4]) < 0.16, lines[1]
    else:
        assert lines[1].startswith("device none") and "no CPU fallback" in lines[1]
