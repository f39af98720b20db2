"""Pose graphs on the CPU (include/dvo_amd.h, "pose graphs"): dvo_graph_solve_host against the numpy restatement of the definition
(tests/pose_graph_reference.py) on every case, optimality and exactness of its results, the robust edges, every refusal,
dvo_graph_information against pose_covariance, the bindings' layouts, creation without a device, and the solver's own code
(rgbd_odometry_amd/csrc/dvo_pose_graph.h) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/host/pose_graph_main.cpp).  No GPU: the host solver needs neither a device nor a handle."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_reference as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(pg.cases())

host = pg.host_solved


@pytest.mark.parametrize("name", NAMES)
def test_host_solver_equals_the_restatement(name):
    """iteration counts agree, cost traces to 1e-9 relative, poses to 1e-7 (three orders above step_tol; measured: 0, the two are
    bit-equal on this platform)"""
    R, t, rep = host(name)
    Rr, tr, ref = pg.solved(name)
    assert (rep["iterations"], rep["accepted"], rep["status"]) == (ref["iterations"], ref["accepted"], ref["status"])
    assert rep["cg_iterations"] == ref["cg_iterations"]
    assert len(rep["cost_trace"]) == len(ref["cost_trace"]) == rep["iterations"] + 1
    rel = np.abs(rep["cost_trace"] - ref["cost_trace"]) / np.maximum(np.abs(ref["cost_trace"]), 1e-300)
    d = pg.pose_distance(Rr, tr, R, t)
    print("%s: iterations %d, trace %.3e, poses %.3e" % (name, rep["iterations"], rel.max(), d))
    assert rel.max() <= 1e-9
    assert d <= 1e-7
    assert rep["cost0"] == rep["cost_trace"][0] and rep["cost"] == rep["cost_trace"][-1]
    assert rep["status"] == pg.CONVERGED


@pytest.mark.parametrize("name", [n for n in NAMES if n != "single"])
def test_optimality(name):
    """at the returned poses the restatement's gradient is at most 1e-6 of its value at the initial poses"""
    g = pg.cases()[name]
    R, t, _ = host(name)
    g0, g1 = pg.gradient(g, g["R0"], g["t0"]), pg.gradient(g, R, t)
    print("%s: gradient %.3e -> %.3e (%.1e)" % (name, g0, g1, g1 / g0))
    assert g0 > 0 and g1 <= 1e-6 * g0


def test_exactness():
    g = pg.cases()["ring_clean(24)"]
    R, t, _ = host("ring_clean(24)")
    assert pg.pose_distance(*g["truth"], R, t) <= 1e-7
    g = pg.cases()["pair"]
    R, t, _ = host("pair")
    want = pg.compose(g["R0"][:1], g["t0"][:1], g["R"], g["t"])           # T_0 Z
    assert pg.pose_distance(*want, R[1:], t[1:]) <= 1e-12
    assert np.array_equal(R[0], g["R0"][0]) and np.array_equal(t[0], g["t0"][0])
    g = pg.cases()["single"]
    R, t, rep = host("single")
    assert pg.poses12(R, t).tobytes() == pg.poses12(g["R0"], g["t0"]).tobytes()
    assert rep["iterations"] == 0 and rep["status"] == pg.CONVERGED and rep["cost"] == 0.0
    # fixed nodes never move, byte for byte
    for name in ("two_fixed", "star", "ring(65)"):
        g = pg.cases()[name]
        R, t, _ = host(name)
        f = g["fixed"] != 0
        assert pg.poses12(R[f], t[f]).tobytes() == pg.poses12(g["R0"][f], g["t0"][f]).tobytes()


def test_robust_edges():
    err = {}
    for name in ("outlier", "outlier_plain"):
        R, t, _ = host(name)
        err[name] = pg.pose_distance(*pg.cases()[name]["truth"], R, t)
    print("ground-truth error: plain %.3f, robust %.3f" % (err["outlier_plain"], err["outlier"]))
    assert err["outlier_plain"] >= 1.0
    assert err["outlier"] <= 0.3
    # huber_delta <= 0 makes robust edges plain
    from rgbd_odometry_amd import capi
    g = pg.cases()["outlier"]
    P, _ = capi.pose_graph_solve_host(pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g), capi.DvoGraphParams.default(huber_delta=0.0))
    Rp, tp, _ = host("outlier_plain")
    assert pg.poses12(Rp, tp).tobytes() == P.tobytes()


def test_refusals():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    g = pg.cases()["ring(24)"]
    P0 = pg.poses12(g["R0"], g["t0"])
    n, ne = g["n"], len(g["i"])
    good = pg.c_edges(g)
    SENT = 1.2345e300

    def call(edit=None, params=None, poses=None, fixed=None, n_nodes=n, n_edges=ne, null=(), cap=4):
        P = P0.copy() if poses is None else poses.copy()
        before = P.copy()
        f = np.ascontiguousarray(g["fixed"] if fixed is None else fixed, dtype=np.uint8)
        edges = [capi.DvoGraphEdge.make(e.i, e.j, np.array(e.R).reshape(3, 3).T, e.t, np.array(e.info).reshape(6, 6), bool(e.flags)) for e in good]
        if edit:
            edit(edges)
        arr = (capi.DvoGraphEdge * max(len(edges), 1))(*edges)
        p = capi.DvoGraphParams.default(**(params or {}))
        rep = capi.DvoGraphReport()
        C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
        rep0 = bytes(rep)
        trace = np.full(8, SENT)
        rc = lib.dvo_graph_solve_host(C.byref(p), n_nodes, None if "poses" in null else capi._ptr(P), None if "fixed" in null else capi._ptr(f),
                                      n_edges, None if "edges" in null else arr, None if "report" in null else C.byref(rep),
                                      None if "trace" in null else capi._ptr(trace), cap)
        if rc != capi.DVO_OK:
            assert np.array_equal(P, before, equal_nan=True) and bytes(rep) == rep0 and np.all(trace == SENT), "a refused call must write nothing"
        return rc

    def ed(k, field, index, value):
        def edit(edges):
            if index is None:
                setattr(edges[k], field, value)
            else:
                getattr(edges[k], field)[index] = value
        return edit

    assert call() == capi.DVO_OK
    assert call(null=("trace",), cap=0) == capi.DVO_OK
    bad = [dict(null=("poses",)), dict(null=("fixed",)), dict(null=("report",)), dict(null=("edges",)), dict(null=("trace",)), dict(cap=-1),
           dict(n_nodes=0), dict(n_nodes=-1), dict(n_nodes=capi.DVO_GRAPH_MAX_NODES + 1), dict(n_edges=-1), dict(n_edges=capi.DVO_GRAPH_MAX_EDGES + 1),
           dict(edit=ed(5, "i", None, -1)), dict(edit=ed(5, "j", None, n)), dict(edit=ed(5, "j", None, 5)), dict(n_nodes=n - 1),
           dict(edit=ed(3, "flags", None, 2)), dict(edit=ed(3, "flags", None, -1)),
           dict(edit=ed(2, "info", 1, 3.0)),                                  # not symmetric
           dict(edit=ed(2, "info", 0, -1.0)), dict(edit=ed(2, "info", 35, 0.0)),  # no Cholesky factor
           dict(fixed=np.zeros(n, np.uint8)),                                 # the gauge of the only component is free
           dict(params=dict(max_iterations=-1)), dict(params=dict(cg_max_iterations=-1)), dict(params=dict(lambda_up=1.0)),
           dict(params=dict(lambda_up=0.5)), dict(params=dict(lambda_down=0.0)), dict(params=dict(lambda_down=1.0)),
           dict(params=dict(lambda_down=-0.1)), dict(params=dict(lambda0=-1.0)), dict(params=dict(cg_tol=float("nan"))),
           dict(params=dict(huber_delta=float("inf"))), dict(params=dict(lambda_max=1e-13))]
    for v in (float("nan"), float("inf"), float("-inf")):
        for idx in (0, 9, 12 * n - 1):
            P = P0.copy()
            P.ravel()[idx] = v
            bad.append(dict(poses=P))
        bad += [dict(edit=ed(7, "R", 4, v)), dict(edit=ed(7, "t", 2, v)), dict(edit=ed(7, "info", 14, v))]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
    # a symmetric perturbation below 1e-9 relative passes
    assert call(edit=ed(2, "info", 1, 1e-7)) == capi.DVO_ERR_INVALID            # info[0][1] = 1e-7 against info[1][0] = 0
    def tiny(edges):
        edges[2].info[1] = 10.0
        edges[2].info[6] = 10.0 * (1.0 + 5e-10)
    assert call(edit=tiny) == capi.DVO_OK
    # a second component without a fixed node
    def split(edges):
        for e in edges:
            if (e.i < 12) != (e.j < 12):
                e.i, e.j = (0, 1) if e.i < 12 else (12, 13)
    assert call(edit=split) == capi.DVO_ERR_INVALID
    f2 = g["fixed"].copy()
    f2[17] = 1
    assert call(edit=split, fixed=f2) == capi.DVO_OK
    # n_edges = 0 with every node fixed is valid and returns the input
    assert call(n_edges=0, fixed=np.ones(n, np.uint8)) == capi.DVO_OK
    assert call(n_edges=0) == capi.DVO_ERR_INVALID
    with pytest.raises(capi.DvoError) as ei:
        capi.pose_graph_solve_host(P0, np.zeros(n, np.uint8), good)
    assert ei.value.code == capi.DVO_ERR_INVALID
    p = capi.DvoGraphParams()
    assert lib.dvo_graph_params_default(None) == capi.DVO_ERR_INVALID and lib.dvo_graph_params_default(C.byref(p)) == capi.DVO_OK
    assert {k: getattr(p, k) for k, _ in capi.DvoGraphParams._fields_} == pg.DEFAULTS


def test_graph_information_inverts_pose_covariance():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    rng = np.random.default_rng(3)
    for _ in range(5):
        A = rng.normal(size=(6, 6))
        H = A @ A.T * 1e4 + np.eye(6)
        H = 0.5 * (H + H.T)
        s2, nv = float(rng.uniform(10, 1e4)), int(rng.integers(7, 5000))
        info = capi.graph_information(H, s2, nv)
        Cv = capi.pose_covariance(H, s2, nv)
        assert np.abs(info @ Cv - np.eye(6)).max() <= 1e-9
        assert np.array_equal(info, info.T)
    H = np.eye(6) * 100.0
    out = np.full(36, 7.0)
    bad = [(H, 5.0, 6), (H, 5.0, 0), (H * np.nan, 5.0, 100), (-H, 5.0, 100), (np.ones((6, 6)), 5.0, 100)]
    for Hb, s2, nv in bad:
        assert capi.pose_covariance(Hb, s2, nv) is None
        Hc = np.ascontiguousarray(Hb, dtype=np.float64)
        assert lib.dvo_graph_information(capi._ptr(Hc), s2, nv, capi._ptr(out)) == capi.DVO_ERR_INVALID
    for s2 in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dvo_graph_information(capi._ptr(H), s2, 100, capi._ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_graph_information(None, 5.0, 100, capi._ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_graph_information(capi._ptr(H), 5.0, 100, None) == capi.DVO_ERR_INVALID
    assert np.all(out == 7.0), "a refused call must write nothing"
    with pytest.raises(capi.DvoError):
        capi.graph_information(H, 5.0, 6)


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in ("dvo_graph_params_default", "dvo_graph_solve_host", "dvo_graph_create", "dvo_graph_destroy", "dvo_graph_last_error",
                 "dvo_graph_set", "dvo_graph_solve", "dvo_graph_get_poses", "dvo_graph_get_report", "dvo_graph_stats", "dvo_graph_information"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    for macro in ("DVO_GRAPH_EDGE_ROBUST", "DVO_GRAPH_MAX_NODES", "DVO_GRAPH_MAX_EDGES", "DVO_GRAPH_LAUNCHES", "DVO_GRAPH_CONVERGED",
                  "DVO_GRAPH_MAX_ITERATIONS", "DVO_GRAPH_NUMERIC"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == getattr(capi, macro), macro
    assert (capi.DVO_GRAPH_MAX_NODES, capi.DVO_GRAPH_MAX_EDGES, capi.DVO_GRAPH_LAUNCHES) == (4096, 32768, 1)
    assert (pg.CONVERGED, pg.MAX_ITERATIONS, pg.NUMERIC, pg.ROBUST) == (capi.DVO_GRAPH_CONVERGED, capi.DVO_GRAPH_MAX_ITERATIONS,
                                                                          capi.DVO_GRAPH_NUMERIC, capi.DVO_GRAPH_EDGE_ROBUST)
    # the types are declared twice under one guard (the public header and the definition's own): the two texts must be the same
    own = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_pose_graph.h")).read(), flags=re.S)
    pat = r"#ifndef DVO_GRAPH_TYPES_DEFINED_.*?#endif"
    assert re.search(pat, text, re.S).group(0).split() == re.search(pat, own, re.S).group(0).split()


def test_struct_layouts_match_header(tmp_path):
    """the ctypes mirrors must have the layouts the C compiler gives the three structs"""
    from rgbd_odometry_amd import capi
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", '
                   'sizeof(dvo_graph_edge), offsetof(dvo_graph_edge, R), offsetof(dvo_graph_edge, info), offsetof(dvo_graph_edge, flags), '
                   'sizeof(dvo_graph_params), offsetof(dvo_graph_params, lambda0), offsetof(dvo_graph_params, huber_delta), '
                   'sizeof(dvo_graph_report), offsetof(dvo_graph_report, iterations));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = tuple(int(x) for x in subprocess.check_output([exe]).split())
    E, P, R = capi.DvoGraphEdge, capi.DvoGraphParams, capi.DvoGraphReport
    assert got == (C.sizeof(E), E.R.offset, E.info.offset, E.flags.offset, C.sizeof(P), P.lambda0.offset, P.huber_delta.offset,
                   C.sizeof(R), R.iterations.offset)


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    from rgbd_odometry_amd import capi
    with pytest.raises(capi.DvoError) as ei:
        capi.DvoPoseGraphs(1, 8, 8)
    assert ei.value.code == capi.DVO_ERR_NO_DEVICE
    assert "no CPU fallback" in str(ei.value)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_graph")
    exe = str(d / "pose_graph_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "pose_graph_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/pose_graph_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def _case_bytes(g, params):
    from rgbd_odometry_amd import capi
    edges = pg.c_edges(g)
    return (struct.pack("<ii", g["n"], len(edges)) + bytes(params) + pg.poses12(g["R0"], g["t0"]).tobytes() +
            np.ascontiguousarray(g["fixed"], dtype=np.uint8).tobytes() + b"".join(bytes(e) for e in edges))


def test_solver_under_sanitizers(host_program):
    """the same code the library compiles, with every array allocated to its exact size: reports, traces and poses byte-equal to the
    library's host entry point, clean under -fsanitize=address,undefined; a refused graph is refused there too"""
    from rgbd_odometry_amd import capi
    d, exe = host_program
    names = list(NAMES)
    p = capi.DvoGraphParams.default()
    blobs = [_case_bytes(pg.cases()[n], p) for n in names]
    free = dict(pg.cases()["ring(24)"])
    free["fixed"] = np.zeros(24, np.uint8)
    blobs.append(_case_bytes(free, p))
    blobs.append(_case_bytes(pg.cases()["ring(24)"], capi.DvoGraphParams.default(max_iterations=2)))
    path = str(d / "cases.bin")
    open(path, "wb").write(struct.pack("<i", len(blobs)) + b"".join(blobs))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    at = 0
    for k, name in enumerate(names + ["free", "capped"]):
        if name == "free":
            assert lines[at] == "case %d refused" % k
            at += 1
            continue
        assert lines[at] == "case %d ok" % k, (name, lines[at])
        rep = capi.DvoGraphReport.from_buffer_copy(bytes.fromhex(lines[at + 1]))
        trace = np.frombuffer(bytes.fromhex(lines[at + 2]), np.float64)
        poses = np.frombuffer(bytes.fromhex(lines[at + 3]), np.float64).reshape(-1, 12)
        at += 4
        if name == "capped":
            g = pg.cases()["ring(24)"]
            P, want = capi.pose_graph_solve_host(pg.poses12(g["R0"], g["t0"]), g["fixed"], pg.c_edges(g), capi.DvoGraphParams.default(max_iterations=2))
            assert rep.status == capi.DVO_GRAPH_MAX_ITERATIONS and rep.iterations == 2
        else:
            R, t, want = host(name)
            P = pg.poses12(R, t)
        assert (rep.iterations, rep.accepted, rep.cg_iterations, rep.status) == (want["iterations"], want["accepted"], want["cg_iterations"],
                                                                                 want["status"]), name
        assert (rep.cost0, rep.cost, rep.lambda_, rep.max_step) == (want["cost0"], want["cost"], want["lambda_"], want["max_step"]), name
        assert trace[:rep.iterations + 1].tobytes() == want["cost_trace"].tobytes(), name
        assert poses.tobytes() == P.tobytes(), name
    assert at == len(lines)


def test_cpp_mirror_builds_and_solves(tmp_path):
    """include/dvo_amd.hpp's PoseGraph, addOdometryEdge, addClosureEdge (instantiated on SolveDVOStreams::Candidate) and PoseGraphs:
    tests/host/pose_graph_hpp_main.cpp compiles with plain g++ and every warning on, builds a graph from records and solves it on the
    host; with a device it solves it through PoseGraphs too, and the poses agree to 1e-7"""
    import torch
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "pose_graph_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "pose_graph_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[0] == "edges 4"
    tok = lines[1].split()
    assert tok[:3] == ["host", "status", "0"] and 2.7 < float(tok[6]) < 3.0            # between the closure's 2.7 and the chain's 3.0
    if torch.cuda.is_available():
        tok = lines[2].split()
        assert tok[:3] == ["device", "status", "0"] and float(tok[4]) <= 1e-7, lines[2]
    else:
        assert lines[2].startswith("device none") and "no CPU fallback" in lines[2]
