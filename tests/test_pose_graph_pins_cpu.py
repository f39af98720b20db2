"""The per-edge mathematics of the pose graphs (rgbd_odometry_amd/csrc/dvo_pose_graph.h) against an independent reference in mpmath
(tests/pose_graph_independent.py): Exp and Log on a sweep of angles that ends AT a half turn, the truncated Jr^-1 against the exact one,
edge_linearise and edge_jacobians against differenced Jacobians, the solver's results against the gradient of the true cost, and the
marginal covariances against a dense inverse built from the differenced Jacobians.

The functions under test run in a stand-alone program (tests/host/pose_graph_edge_main.cpp) compiled with the library's host flags and
-ffp-contract=off, once more under the address and undefined-behaviour sanitizers.  No GPU.

The other pose-graph tests compare the host solver with a numpy restatement of the same formulas and the device with the host solver:
a mistake in the shared formulas is invisible to them.  These are the tests that see one."""
import os
import struct
import subprocess

import mpmath as mp
import numpy as np
import pytest

import pose_graph_independent as ind
import pose_graph_marginals_reference as mr
import pose_graph_reference as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]          # CXXFLAGS of csrc/Makefile

JR_NORMS = [1e-6, 1e-4, 1e-3, 1e-2, 0.1, 0.3, 0.5, 1.0, 1.3, 1.6]
EDGE_NORMS = [1e-3, 0.05, 0.5, 1.5]
DIRECTIONS = np.array([[0.4, -0.3, 0.5, 0.35, -0.45, 0.4], [0.1, 0.7, -0.2, -0.6, 0.1, 0.3], [0.0, 0.0, 0.0, 0.5, 0.5, -0.7],
                       [0.6, -0.6, 0.5, 0.0, 0.0, 0.0]])
EDGE_TI = np.array([0.5, -1.0, 0.3, 0.2, 0.4, -0.6])
EDGE_Z = np.array([1.2, 0.4, -0.3, -0.3, 0.5, 0.7])


def _unit(d):
    return d / np.linalg.norm(d)


def _col(R):
    return np.asarray(R, dtype=np.float64).T.reshape(9)


# ---- the cases, the reference's answers and the program's ---------------------------------------------------------------------------

_EDGE_CASES = []


def edge_cases():
    """poses whose residual has a given norm, each under Omega = I and the anisotropic Omega, plain and robust with s just below, at and
    just above huber_delta: dicts with the float64 inputs and the reference's r, J_i, J_j (differenced once per norm)"""
    from rgbd_odometry_amd import capi
    if _EDGE_CASES:
        return _EDGE_CASES
    with mp.workdps(ind.DPS):
        Tim, Zm = ind.se3_exp(EDGE_TI), ind.se3_exp(EDGE_Z)
        Ri, ti, ZR, Zt = ind.f64(Tim[0]), ind.f64(Tim[1]), ind.f64(Zm[0]), ind.f64(Zm[1])
        Ti, Z = ind.pose(Ri, ti), ind.pose(ZR, Zt)
        for norm in EDGE_NORMS:
            Tjm = ind.compose(Ti, Z, ind.se3_exp(norm * _unit(DIRECTIONS[0])))
            Rj, tj = ind.f64(Tjm[0]), ind.f64(Tjm[1])
            Tj = ind.pose(Rj, tj)
            r, Ji, Jj = ind.edge_jacobians(Ti, Tj, Z)
            RE, tE = ind._rel(*Z, *ind._rel(*Ti, *Tj))
            for kind, info in (("I", np.eye(6)), ("aniso", ind.aniso_information())):
                s = float(mp.sqrt(ind.weight_and_rho(r, ind._m(info), False, mp.mpf(0))[0]))
                for robust, delta, where in ((False, 1.0, "plain"), (True, s * (1.0 + 1e-6), "below"), (True, s, "at"), (True, s * (1.0 - 1e-6), "above")):
                    edge = capi.DvoGraphEdge.make(7, 9, ZR, Zt, info, robust=robust)           # i, j: the program sets them
                    _EDGE_CASES.append(dict(norm=norm, kind=kind, where=where, robust=robust, delta=delta, info=info, s=s,
                                            Pi=np.concatenate([_col(Ri), ti]), Pj=np.concatenate([_col(Rj), tj]), edge=edge, r=r, Ji=Ji, Jj=Jj,
                                            tE=float(ind._norm(tE)), blocks=ind.edge_blocks(r, Ji, Jj, info, robust, delta)))
    return _EDGE_CASES


def jr_cases():
    return [norm * _unit(d) for norm in JR_NORMS for d in DIRECTIONS]


def case_file():
    rec = []
    for item in ind.sweep():
        with mp.workdps(ind.DPS):
            rec.append(struct.pack("<i", 0) + ind.f64(item["r"]).tobytes())                       # Exp of the reference's Log, rounded
        rec.append(struct.pack("<i", 1) + _col(item["R"]).tobytes() + item["t"].tobytes())
    for r in jr_cases():
        rec.append(struct.pack("<i", 2) + r.tobytes())
    for c in edge_cases():
        rec.append(struct.pack("<i", 3) + c["Pi"].tobytes() + c["Pj"].tobytes() + bytes(c["edge"]) + struct.pack("<d", c["delta"]))
    return struct.pack("<i", len(rec)) + b"".join(rec)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the program's output on every case: lists of float64 arrays for exp, log, jr and edge records; (directory, case file) too"""
    d = tmp_path_factory.mktemp("pose_graph_edge")
    exe = str(d / "pose_graph_edge_main")
    build = subprocess.run(["g++"] + HOST_FLAGS + ["-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "pose_graph_edge_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    path = str(d / "cases.bin")
    open(path, "wb").write(case_file())
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    rows = [np.array([float.fromhex(x) for x in line.split()]) for line in run.stdout.splitlines()]
    n = len(ind.sweep())
    assert len(rows) == 2 * n + len(jr_cases()) + len(edge_cases())
    return dict(exp=rows[0:2 * n:2], log=rows[1:2 * n:2], jr=rows[2 * n:2 * n + len(jr_cases())], edge=rows[2 * n + len(jr_cases()):],
                dir=d, cases=path, stdout=run.stdout)


def test_program_under_sanitizers(program):
    """the same program and the same cases under -fsanitize=address,undefined: clean, and the same numbers"""
    exe = str(program["dir"] / "pose_graph_edge_main_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "pose_graph_edge_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/pose_graph_edge_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    run = subprocess.run([exe, program["cases"]], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout == program["stdout"]


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------

def test_reference_exp_and_log_against_the_matrix_exponential():
    """the closed forms of the reference against mp.expm of the 4 x 4 twist, and Log as its inverse, to 1e-60"""
    with mp.workdps(ind.DPS):
        for d in (0.7 * _unit(DIRECTIONS[0]), 3.1 * _unit(DIRECTIONS[1]), 1e-9 * _unit(DIRECTIONS[0]), np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0])):
            R, t = ind.se3_exp(d)
            v, w = [mp.mpf(float(x)) for x in d[:3]], [mp.mpf(float(x)) for x in d[3:]]
            X = mp.zeros(4)
            X[0, 1], X[0, 2], X[1, 0], X[1, 2], X[2, 0], X[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
            for k in range(3):
                X[k, 3] = v[k]
            E = mp.expm(X, method="taylor")
            assert max(abs(E[i, j] - R[i][j]) for i in range(3) for j in range(3)) < mp.mpf(10) ** -60
            assert max(abs(E[i, 3] - t[i]) for i in range(3)) < mp.mpf(10) ** -60
            back = ind.se3_log(R, t)
            assert max(abs(back[k] - mp.mpf(float(d[k]))) for k in range(6)) < mp.mpf(10) ** -60
        # the differenced J_j is the exact Jr^-1(r): two independent routes to the same matrix
        c = [c for c in edge_cases() if c["norm"] == 1.5][0]
        J = ind.jr_inv(c["r"])
        assert max(abs(J[a][b] - c["Jj"][a][b]) for a in range(6) for b in range(6)) < mp.mpf(10) ** -25


# ---- Exp and Log ---------------------------------------------------------------------------------------------------------------------

def _pose_error(R, t, Rc, tc):
    """max|dR|, max|dt| / max(1, |t|) of float64 (Rc column-major, tc) against mp (R, t)"""
    with mp.workdps(ind.DPS):
        eR = max(abs(mp.mpf(float(Rc[i + 3 * j])) - R[i][j]) for i in range(3) for j in range(3))
        et = max(abs(mp.mpf(float(tc[i])) - t[i]) for i in range(3)) / max(1, ind._norm(t))
        return float(max(eR, et))


def test_log_on_the_whole_sweep(program):
    """se3_log against the reference on every angle up to and including pi, every axis and translation: LOG_TOLERANCE, which is ten times
    the worst error measured below pi - 1e-2 with the formula that took w from the antisymmetric part alone.  The round trip through the
    reference's Exp is held to the same number.

    Measured (profiles/pose_graph_pins/README.md): before the symmetric-part branch 5.1e-13 at pi - 1e-4, 5.8e-9 at pi - 1e-8 and 3.14
    from pi - 1e-9 on (a half turn was "no rotation"), so this test failed from pi - 1e-4 on; with the branch at most 9.5e-16 anywhere."""
    worst, below, worst_trip = {}, 0.0, 0.0
    for item, r in zip(ind.sweep(), program["log"]):
        e = ind.log_error(r, item)
        worst[item["label"]] = max(worst.get(item["label"], 0.0), e)
        if item["theta"] <= mp.pi - mp.mpf("1e-2"):
            below = max(below, e)
        R, t = ind.se3_exp(r)
        with mp.workdps(ind.DPS):
            T = ind.pose(item["R"], item["t"])
            trip = float(max(max(abs(R[i][j] - T[0][i][j]) for i in range(3) for j in range(3)),
                             max(abs(t[i] - T[1][i]) for i in range(3)) / max(1, ind._norm(T[1]))))
        worst_trip = max(worst_trip, trip)
        worst["trip " + item["label"]] = max(worst.get("trip " + item["label"], 0.0), trip)
    for label, _ in ind.angles():
        print("theta %-12s log %.3e   Exp_ref(Log) %.3e" % (label, worst[label], worst["trip " + label]))
    print("worst at theta <= pi - 1e-2: %.3e (LOG_HOST_AGAINST_REFERENCE_MEASURED %.3e)" % (below, ind.LOG_HOST_AGAINST_REFERENCE_MEASURED))
    bad = {k: v for k, v in worst.items() if not v <= ind.LOG_TOLERANCE}
    assert not bad, bad


def test_exp_on_the_whole_sweep(program):
    """se3_exp at the rounded reference Log of every sweep item against the reference's Exp of that same float64 vector"""
    worst = 0.0
    for item, out in zip(ind.sweep(), program["exp"]):
        with mp.workdps(ind.DPS):
            d = ind.f64(item["r"])
        R, t = ind.se3_exp(d)
        worst = max(worst, _pose_error(R, t, out[:9], out[9:]))
    print("Exp: worst %.3e" % worst)
    assert worst <= ind.LOG_TOLERANCE


def test_sweep_reaches_both_sides_of_every_switch():
    """the angles next to theta^2 = 1e-4 and next to the hand-over of Log straddle them, as the code decides them"""
    lab = {item["label"]: item for item in ind.sweep() if item["kx"] == 4 and item["kt"] == 0}
    th2 = {k: float(lab[k]["theta"]) ** 2 for k in ("small-", "small+")}
    assert th2["small-"] < 1e-4 <= th2["small+"]
    def sin_cos(item):
        R = item["R"]
        s = 0.5 * np.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
        return s, 0.5 * (np.trace(R) - 1.0)
    lo, hi = sin_cos(lab["switch-1e-6"]), sin_cos(lab["switch+1e-6"])
    assert lo[1] < 0 and hi[1] < 0 and hi[0] < ind.NEAR_PI_SIN < lo[0]
    for k in ("switch-", "switch+"):
        assert abs(sin_cos(lab[k])[0] - ind.NEAR_PI_SIN) < 1e-15


# ---- Jr^-1 -----------------------------------------------------------------------------------------------------------------------------

def jr_bound(a):
    """|I + ad/2 + ad^2/12 - ad^4/720 - Jr^-1|_2 <= 2 |ad|^6 / 30240: the first omitted Bernoulli term, ad^6 / 30240, times a geometric
    tail (the ratio of consecutive terms tends to |ad|^2 / (2 pi)^2 <= 0.065 at |ad| <= 1.6; the first ratios are below 0.07), which
    is below 1.2, rounded up to 2"""
    return 2.0 * a ** 6 / 30240.0


def rounding_floor(J_norm):
    """what double arithmetic adds to any 6 x 6 product chain of this file: each entry is a 6-term sum of products taken at most three
    deep (gamma_6 each, 18 eps), rounded once more on its way into a sum, and an entry-wise bound costs sqrt(6) in the 2-norm: 64 eps
    times the norm of the result.  Below |ad| ~ 0.02 it exceeds jr_bound (at |r| = 1e-6 that is 1e-40, less than one rounding of 1.0)"""
    return 64.0 * EPS * J_norm


def test_jr_inv_against_the_exact_inverse(program):
    worst = 0.0
    for r, J in zip(jr_cases(), program["jr"]):
        exact = ind.f64_exact(ind.jr_inv(r), J.reshape(6, 6))
        a = ind.ad_norm(r)
        err = np.linalg.norm(exact, 2)
        bound = jr_bound(a) + rounding_floor(1.0 + a)
        if jr_bound(a) > rounding_floor(1.0 + a):
            worst = max(worst, err / jr_bound(a))
        print("|r| %.1e |ad| %.3e: error %.3e, truncation bound %.3e" % (np.linalg.norm(r), a, err, jr_bound(a)))
        assert err <= bound
    print("worst error / truncation bound where the bound is above the rounding floor: %.3f" % worst)
    assert worst > 0.2, "the bound is meant to be tight: the first omitted term alone is half of it"


# ---- edge_linearise and edge_jacobians -------------------------------------------------------------------------------------------------

def _n2(A):
    return float(np.linalg.norm(np.atleast_2d(A), 2))


def edge_bounds(c):
    """The Jr^-1 bound propagated through one edge.  With a = |ad(r)|_2, rho = 3 LOG_TOLERANCE max(1, |t_E|) >= |r_code - r|_2 (Log's
    tolerance on six components), eps-terms from rounding_floor:
      J_j = Jr^-1(r):          bj = jr_bound(a) + 2 rho + floor      (the truncated series is 1-Lipschitz in ad for |ad| <= 2.2:
                                                                     1/2 + |ad|/6 + |ad|^3/180 < 1, and |ad(dr)|_2 <= 2 |dr|_2)
      J_i = -J_j Ad:           bi = (bj + floor) |Ad|_2
      w (robust, s > delta):   relative error eta = |Omega r| rho / s^2  (d(s^2) = 2 r^T Omega dr, w = delta / s)
      H_ac = J_a^T W J_c:      |W| (|J_a| bc + |J_c| ba + ba bc) + (eta + floor) |W| |J_a| |J_c|
      b_a = J_a^T W r:         ba |W r| + |J_a| |W| rho + (eta + floor) |J_a| |W| |r|"""
    r, Ji, Jj = ind.f64(c["r"]), ind.f64(c["Ji"]), ind.f64(c["Jj"])
    a = ind.ad_norm(r)
    rho = 3.0 * ind.LOG_TOLERANCE * max(1.0, c["tE"])
    nj, ni = _n2(Jj), _n2(Ji)
    Ad = -np.linalg.solve(Jj, Ji)
    bj = jr_bound(a) + 2.0 * rho + rounding_floor(nj)
    bi = (bj + rounding_floor(nj)) * _n2(Ad)
    w = 1.0 if not (c["robust"] and c["s"] > c["delta"]) else c["delta"] / c["s"]
    W = w * c["info"]
    eta = (_n2(c["info"] @ r) * rho / c["s"] ** 2 if c["robust"] else 0.0) + rounding_floor(1.0)
    nW = _n2(W)
    H = lambda na, nc, ba, bc: nW * (na * bc + nc * ba + ba * bc) + eta * nW * na * nc
    b = lambda na, ba: ba * _n2(W @ r) + na * nW * rho + eta * na * nW * _n2(r)
    return dict(r=rho, Ji=bi, Jj=bj, Hii=H(ni, ni, bi, bi), Hij=H(ni, nj, bi, bj), Hjj=H(nj, nj, bj, bj), bi=b(ni, bi), bj=b(nj, bj))


def _edge_output(row):
    return dict(r=row[:6], Hii=row[6:42].reshape(6, 6), Hij=row[42:78].reshape(6, 6), Hjj=row[78:114].reshape(6, 6), bi=row[114:120],
                bj=row[120:126], r2=row[126:132], Ji=row[132:168].reshape(6, 6), Jj=row[168:204].reshape(6, 6))


def test_edge_linearise_and_jacobians_against_differenced_jacobians(program):
    worst = {}
    for c, row in zip(edge_cases(), program["edge"]):
        out = _edge_output(row)
        bound = edge_bounds(c)
        ref = dict(zip(("Hii", "Hij", "Hjj", "bi", "bj"), c["blocks"]), r=c["r"], Ji=c["Ji"], Jj=c["Jj"])
        assert out["r"].tobytes() == out["r2"].tobytes()
        for key in ("r", "Ji", "Jj", "Hii", "Hij", "Hjj", "bi", "bj"):
            err = _n2(ind.f64_exact(ref[key], out[key]))
            ratio = err / bound[key]
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert err <= bound[key], (c["norm"], c["kind"], c["where"], key, err, bound[key])
        # the Huber weight took the branch the case was built for: against the code's own plain block of the same poses and Omega
        if c["where"] == "plain":
            plain = out["Hjj"]
        else:
            scale = np.abs(out["Hjj"]).max() / np.abs(plain).max()
            assert scale == pytest.approx(1.0 - 1e-6 if c["where"] == "above" else 1.0, abs=1e-9), (c["norm"], c["kind"], c["where"])
    print("worst error / bound: " + ", ".join("%s %.3f" % kv for kv in worst.items()))


def test_h_ij_is_not_its_transpose(program):
    """H_ij = J_i^T W J_j, rows of node i and columns of node j: on the anisotropic Omega at |r| = 0.5 the block is far from symmetric, the
    code's block matches the reference's and its transpose does not"""
    k = [k for k, c in enumerate(edge_cases()) if c["norm"] == 0.5 and c["kind"] == "aniso" and c["where"] == "plain"][0]
    c, out = edge_cases()[k], _edge_output(program["edge"][k])
    ref = ind.f64(c["blocks"][1])
    tol = edge_bounds(c)["Hij"]
    assert _n2(ref - ref.T) > 0.1 * _n2(ref)
    assert _n2(out["Hij"] - ref) <= tol
    assert _n2(out["Hij"].T - ref) > 1e3 * tol
    assert _n2(out["Hii"] - out["Hii"].T) <= 1e-12 * _n2(out["Hii"]) and _n2(out["Hjj"] - out["Hjj"].T) <= 1e-12 * _n2(out["Hjj"])


# ---- whole graphs ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ring(24)", "ring_aniso(24)", "two_fixed", "outlier_plain", "outlier", "star"])
def test_true_optimality(name):
    """the gradient of the TRUE cost (exact Log, differenced Jacobians) at the restatement's solution is at most 1e-6 of its value at the
    start: the truncation of Jr^-1 in the solver's own gradient does not move the solution beyond the suite's optimality bound"""
    g = pg.cases()[name]
    R, t, _ = pg.solved(name)
    delta = pg.DEFAULTS["huber_delta"]
    g0, g1 = ind.gradient(g, g["R0"], g["t0"], delta), ind.gradient(g, R, t, delta)
    own = pg.gradient(g, R, t) / pg.gradient(g, g["R0"], g["t0"])
    print("%s: true gradient %.3e -> %.3e (%.1e); by the solver's own Jacobians %.1e" % (name, g0, g1, g1 / g0, own))
    assert g0 > 0 and g1 <= 1e-6 * g0


@pytest.mark.parametrize("name", ["pair", "ring(24)", "two_fixed"])
def test_marginals_against_the_independent_dense_inverse(name):
    """dvo_graph_marginals_host at the solved poses against the inverse of the dense H assembled from the differenced Jacobians"""
    from rgbd_odometry_amd import capi
    g = pg.cases()[name]
    R, t, _ = pg.solved(name)
    D = ind.dense_covariance(g, R, t, pg.DEFAULTS["huber_delta"])
    edges = pg.c_edges(g)
    worst = 0.0
    for q in mr.queries(g):
        cov, rep = capi.pose_graph_marginals_host(pg.poses12(R, t), g["fixed"], edges, q, capi.DvoGraphParams.default(cg_tol=mr.CG_TOL))
        d = mr.distance(cov, mr.joint(D, q))
        print("%s, nodes %s: %.3e" % (name, q, d))
        assert rep["status"] == pg.CONVERGED
        worst = max(worst, d)
    assert worst <= mr.TOLERANCE


# ---- the graph that starts at a half turn, and the probe's host constant -----------------------------------------------------------------

def test_cost0_of_the_host_definition_on_the_probe_graphs():
    """dvo_graph_solve_host with max_iterations = 0 on the graphs of the device's cost0 probe: cost0 against the reference's r^T Omega r.
    This is where COST0_HOST_AGAINST_REFERENCE_MEASURED comes from; the host is held to ten times it, the device
    (tests/test_gpu_pose_graph_pins.py) to a hundred times"""
    from rgbd_odometry_amd import capi
    p = capi.DvoGraphParams.default(max_iterations=0)
    worst = {}
    for g in ind.probe_graphs():
        P0 = pg.poses12(g["R0"], g["t0"])
        P, rep = capi.pose_graph_solve_host(P0, g["fixed"], pg.c_edges(g), p)
        assert rep["status"] == pg.MAX_ITERATIONS and rep["iterations"] == 0 and rep["cost"] == rep["cost0"] and P.tobytes() == P0.tobytes()
        worst[g["label"]] = max(worst.get(g["label"], 0.0), ind.cost_error(rep["cost0"], g))
    for label, e in worst.items():
        print("theta %-12s cost0 %.3e" % (label, e))
    print("worst %.3e (COST0_HOST_AGAINST_REFERENCE_MEASURED %.3e)" % (max(worst.values()), ind.COST0_HOST_AGAINST_REFERENCE_MEASURED))
    assert max(worst.values()) <= 10.0 * ind.COST0_HOST_AGAINST_REFERENCE_MEASURED


def test_half_turn_start_on_the_host():
    """ring_half_turn: ring_clean(24) with one free node turned by pi - 1e-10 at the start.  On top of ring_clean's own start error of
    0.05 that leaves the node's two edges with residuals of pi - 0.021 and pi - 0.056, inside Log's symmetric-part branch, worth about
    pi^2 / sigma_r^2 each.  cost0 is the true cost and the solver moves.

    It does NOT reach the truth from there: the cost falls from 2.185e5 to 4.146e4 in the 50 default iterations (status
    MAX_ITERATIONS), and with more it converges after 91 to a local minimum of the true cost, 4.1456e4, 2.45 rad from the truth -- a node
    turned by half a turn can unwind either way, and Levenberg-Marquardt settles between.  So the distance to the truth is printed, not
    asserted; what is asserted is the start cost, that the cost falls, and that host and restatement walk the same path"""
    g = pg.ring_half_turn()
    R, t, rep = pg.host_solved_graph(g)
    want = float(ind.graph_cost(g, g["R0"], g["t0"], pg.DEFAULTS["huber_delta"]))
    print("ring_half_turn: cost0 %.6e (reference %.6e, relative %.2e), cost %.3e, %d iterations, status %d, to the truth %.3e" % (
        rep["cost0"], want, abs(rep["cost0"] - want) / want, rep["cost"], rep["iterations"], rep["status"], pg.pose_distance(*g["truth"], R, t)))
    assert abs(rep["cost0"] - want) <= ind.COST0_TOLERANCE * want
    assert rep["status"] != pg.NUMERIC and rep["cost"] < 0.25 * rep["cost0"]
    Rr, tr, ref = pg.solve(g)
    assert (rep["iterations"], rep["accepted"], rep["cg_iterations"], rep["status"]) == (ref["iterations"], ref["accepted"], ref["cg_iterations"], ref["status"])
    assert pg.pose_distance(Rr, tr, R, t) <= 1e-7


def test_a_start_cost_that_is_not_finite_on_the_host():
    """pair_overflow: a valid graph whose start cost overflows.  DVO_GRAPH_NUMERIC, no iteration, the poses as they came"""
    g = pg.pair_overflow()
    R, t, rep = pg.host_solved_graph(g)
    assert rep["status"] == pg.NUMERIC and rep["iterations"] == 0 and rep["accepted"] == 0 and rep["cg_iterations"] == 0
    assert rep["cost0"] == float("inf") and len(rep["cost_trace"]) == 1
    assert pg.poses12(R, t).tobytes() == pg.poses12(g["R0"], g["t0"]).tobytes()


@pytest.mark.parametrize("name", ["ring(65)", "outlier", "pair"])
def test_zero_tolerances_never_stop_the_loop(name):
    """step_tol = cost_tol = 0: a tolerance of 0 is off, so the host definition and the restatement run to the cap of 12 iterations (a
    rejection at lambda_max needs 16 rejections from lambda0), also where trials of exactly equal cost occur (`pair` is solved exactly
    after one step and every later trial repeats its cost); the trace has iterations + 1 entries and the two walk the same path"""
    g = pg.cases()[name]
    changes = dict(step_tol=0.0, cost_tol=0.0, max_iterations=12)
    R, t, rep = pg.host_solved_graph(g, **changes)
    Rr, tr, ref = pg.solve(g, **changes)
    print("%s: status %d, %d iterations, %d accepted, lambda %.1e" % (name, rep["status"], rep["iterations"], rep["accepted"], rep["lambda_"]))
    assert rep["status"] == pg.MAX_ITERATIONS and rep["iterations"] == 12 and len(rep["cost_trace"]) == 13
    assert (rep["iterations"], rep["accepted"], rep["cg_iterations"], rep["status"]) == (ref["iterations"], ref["accepted"], ref["cg_iterations"], ref["status"])
    assert rep["cost_trace"].tobytes() == ref["cost_trace"].tobytes()
    assert pg.pose_distance(Rr, tr, R, t) <= 1e-7
