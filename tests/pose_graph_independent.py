"""Pose graphs (include/dvo_amd.h, "pose graphs"): an independent reference for the per-edge mathematics, in mpmath at 100 digits.

Nothing here is taken from rgbd_odometry_amd/csrc/dvo_pose_graph.h or from its numpy restatement (tests/pose_graph_reference.py):
Exp and Log are the textbook closed forms (Rodrigues; V and V^-1 of SE(3)), checked in tests/test_pose_graph_pins_cpu.py against
mp.expm of the 4 x 4 twist; Jr^-1 is the Bernoulli series summed to convergence; the Jacobians of the edge residual are central
differences of the mp residual itself.  Only graphs (pose_graph_reference.case) and layout conversions are shared with the restatement.

Conventions, as the public header states them: a pose maps node-frame points to the world, an edge measures Z ~ T_i^-1 T_j, the tangent
order is [translation, rotation], perturbations act on the right (T <- T Exp(x)), r = Log(Z^-1 T_i^-1 T_j), s^2 = r^T Omega r,
rho = s^2 or Huber's 2 delta s - delta^2 beyond delta on edges flagged robust.

Inputs: a matrix handed to the code under test is float64, and the reference evaluates that very float64 matrix, its rotation part
projected to the nearest rotation (the polar factor) at full precision: the reference is not charged for the rounding of its input.

Every function runs at DPS digits whatever the caller's mpmath precision is, and returns mpf numbers (lists and nested lists of them);
f64() converts to numpy."""
import functools

import mpmath as mp
import numpy as np

DPS = 100
#: step of the central differences: truncation ~ H_DIFF^2 = 1e-60, rounding ~ 1e-100 / H_DIFF = 1e-70, both below 1e-25
H_DIFF = mp.mpf(10) ** -30

#: the worst absolute error of dvo_pg::se3_log against se3_log() below over the sweep of tests/test_pose_graph_pins_cpu.py restricted to
#: theta <= pi - 1e-2, errors in v relative to max(1, |t|); measured on the CPU at commit 8dfe3cb, the last one that took the rotation
#: vector from the antisymmetric part alone (profiles/pose_graph_pins/README.md)
LOG_HOST_AGAINST_REFERENCE_MEASURED = 3.69e-15
#: what the tests assert for Log on the whole sweep, pi included: the factor covers the translation scale 30 and V^-1 near pi
LOG_TOLERANCE = 10.0 * LOG_HOST_AGAINST_REFERENCE_MEASURED
#: the worst error (cost_error below) of the host definition's cost0 against edge_cost() on the probe graphs of
#: tests/test_gpu_pose_graph_pins.py (probe_graphs), measured on the CPU at the commit that moved Log near pi to the symmetric part, the
#: child of 8dfe3cb (on 8dfe3cb itself: 1.0 from pi - 1e-9 on, the whole rotational cost missing)
COST0_HOST_AGAINST_REFERENCE_MEASURED = 3.73e-15
#: what the device is held to on the same graphs: its sin / cos / atan2 are the device library's and its sums run in lane order; the
#: factor is the one pose_graph_marginals_reference.TOLERANCE uses from host to device
COST0_TOLERANCE = 100.0 * COST0_HOST_AGAINST_REFERENCE_MEASURED


def _prec(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return run


# ---- small dense algebra on nested lists of mpf ----------------------------------------------------------------------------------

def _m(a):
    """numpy (or nested list) -> nested lists of mpf, exactly"""
    a = np.asarray(a, dtype=object) if not isinstance(a, np.ndarray) else a
    if a.ndim == 1:
        return [mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in a]
    return [[mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in row] for row in a]


def f64(a):
    return np.array([[float(x) for x in row] for row in a]) if isinstance(a[0], (list, tuple)) else np.array([float(x) for x in a])


def f64_exact(ref, code):
    """code - ref for float64 `code` against mpf `ref`, subtracted at full precision and then rounded"""
    with mp.workdps(DPS):
        code = np.asarray(code, dtype=np.float64)
        if code.ndim == 1:
            return np.array([float(mp.mpf(float(code[i])) - ref[i]) for i in range(len(code))])
        return np.array([[float(mp.mpf(float(code[i, j])) - ref[i][j]) for j in range(code.shape[1])] for i in range(code.shape[0])])


def _mm(A, B):
    if len(B) == 3:
        return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(len(B[0]))] for i in range(len(A))]
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _mv(A, x):
    if len(x) == 3:
        return [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(len(A))]
    return [mp.fsum(A[i][k] * x[k] for k in range(len(x))) for i in range(len(A))]


def _tr(A):
    return [[A[j][i] for j in range(len(A))] for i in range(len(A[0]))]


def _eye(n):
    return [[mp.mpf(1 if i == j else 0) for j in range(n)] for i in range(n)]


def _hat(w):
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def _lin(terms, n):
    """sum of c * A over (c, A), n x n"""
    return [[mp.fsum(c * A[i][j] for c, A in terms) for j in range(n)] for i in range(n)]


def _norm(x):
    return mp.sqrt(mp.fsum(v * v for v in x))


@_prec
def project_rotation(R):
    """the rotation nearest to a float64 3 x 3 matrix (its polar factor), by Newton's iteration X <- (X + X^-T) / 2"""
    X = _m(R)
    for _ in range(60):
        C = [[X[(i + 1) % 3][(j + 1) % 3] * X[(i + 2) % 3][(j + 2) % 3] - X[(i + 1) % 3][(j + 2) % 3] * X[(i + 2) % 3][(j + 1) % 3]
              for j in range(3)] for i in range(3)]                       # cofactors: X^-T = C / det
        det = mp.fsum(X[0][j] * C[0][j] for j in range(3))
        Xn = [[(X[i][j] + C[i][j] / det) / 2 for j in range(3)] for i in range(3)]
        d = max(abs(Xn[i][j] - X[i][j]) for i in range(3) for j in range(3))
        X = Xn
        if d < mp.mpf(10) ** -(DPS - 10):
            break
    return X


@_prec
def pose(R, t):
    """(R, t) in float64 -> the reference's pose: (projected R, exact t)"""
    return project_rotation(R), _m(np.asarray(t, dtype=np.float64))


# ---- Exp and Log -------------------------------------------------------------------------------------------------------------------

def _abc(th):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3"""
    if th == 0:
        return mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    return mp.sin(th) / th, 2 * mp.sin(th / 2) ** 2 / th ** 2, (th - mp.sin(th)) / th ** 3


@_prec
def se3_exp(d):
    """Exp of d = [v, w]: R = I + A W + B W^2 (Rodrigues), t = V v with V = I + B W + C W^2"""
    d = _m(d)
    v, w = d[:3], d[3:]
    A, B, C = _abc(_norm(w))
    W = _hat(w)
    W2 = _mm(W, W)
    I = _eye(3)
    return _lin([(1, I), (A, W), (B, W2)], 3), _mv(_lin([(1, I), (B, W), (C, W2)], 3), v)


def _so3_log(R):
    """the rotation vector of a rotation matrix on the closed ball |w| <= pi"""
    sv = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]          # sin(th) a
    s, c = _norm(sv), (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    th = mp.atan2(s, c)
    if s > mp.mpf(10) ** -(DPS // 3):
        return [th * x / s for x in sv]
    if c > 0:                                                              # th below 1e-33: w = sin(th) a to every digit kept
        return sv
    # within 1e-33 of a half turn: (R + R^T) / 2 = c I + (1 - c) a a^T; the column of the largest a_k^2, the sign of sin(th) a
    S = [[(R[i][j] + R[j][i]) / 2 - (c if i == j else 0) for j in range(3)] for i in range(3)]
    k = max(range(3), key=lambda q: S[q][q])
    a = [S[i][k] for i in range(3)]
    n = _norm(a)
    a = [x / n for x in a]
    if mp.fsum(a[i] * sv[i] for i in range(3)) < 0:
        a = [-x for x in a]
    return [th * x for x in a]


def _v_inv(w):
    """V^-1 = I - W / 2 + D W^2, D = (1 - (th / 2) cot(th / 2)) / th^2"""
    th = _norm(w)
    D = mp.mpf(1) / 12 if th == 0 else (1 - (th / 2) * mp.cot(th / 2)) / th ** 2
    W = _hat(w)
    return _lin([(1, _eye(3)), (-mp.mpf(1) / 2, W), (D, _mm(W, W))], 3)


@_prec
def se3_log(R, t, flip=False):
    """Log of (R, t), mp inputs (see pose()): r = [V^-1 t, w], valid on the whole closed ball theta <= pi.

    At theta = pi both signs of the axis are correct (w and -w are the same rotation) and they give different v: which one a float64
    input lands on is decided by its rounding.  flip=True returns the other representative, [V(-w)^-1 t, -w]; a comparison at a half
    turn accepts either, or goes through Exp(Log(.))"""
    w = _so3_log(R)
    if flip:
        w = [-x for x in w]
    return _mv(_v_inv(w), t) + w


# ---- the edge ------------------------------------------------------------------------------------------------------------------------

def _rel(Ra, ta, Rb, tb):
    """T_a^-1 T_b"""
    Rat = _tr(Ra)
    return _mm(Rat, Rb), _mv(Rat, [tb[k] - ta[k] for k in range(3)])


def _compose(Ra, ta, Rb, tb):
    x = _mv(Ra, tb)
    return _mm(Ra, Rb), [x[k] + ta[k] for k in range(3)]


@_prec
def compose(*poses):
    """T_1 T_2 ... of mp poses (R, t)"""
    R, t = poses[0]
    for Rb, tb in poses[1:]:
        R, t = _compose(R, t, Rb, tb)
    return R, t


@_prec
def edge_residual(Ti, Tj, Z, flip=False):
    """r = Log(Z^-1 T_i^-1 T_j) of mp poses"""
    return se3_log(*_rel(*Z, *_rel(*Ti, *Tj)), flip=flip)


@_prec
def weight_and_rho(r, info, robust, delta):
    """(s^2, Huber weight, rho) of a residual under Omega"""
    s2 = mp.fsum(r[a] * info[a][b] * r[b] for a in range(6) for b in range(6))
    s = mp.sqrt(s2)
    if robust and delta > 0 and s > delta:
        return s2, delta / s, 2 * delta * s - delta * delta
    return s2, mp.mpf(1), s2


@_prec
def edge_cost(Ti, Tj, Z, info, robust=False, delta=0.0, flip=False):
    return weight_and_rho(edge_residual(Ti, Tj, Z, flip=flip), _m(info), robust, mp.mpf(float(delta)))[2]


_STEPS = []


def _steps():
    """Exp(+h e_k), Exp(-h e_k) for k = 0 .. 5, once"""
    if not _STEPS:
        for k in range(6):
            x = [mp.mpf(0)] * 6
            x[k] = H_DIFF
            _STEPS.append((se3_exp(x), se3_exp([-v for v in x])))
    return _STEPS


@_prec
def edge_jacobians(Ti, Tj, Z):
    """r, J_i, J_j (6 x 6): the derivatives of r under T_i Exp(x) and T_j Exp(x) at x = 0, by central differences of the mp residual.
    Z^-1 (T_i X)^-1 T_j = Z^-1 X^-1 (T_i^-1 T_j) and Z^-1 T_i^-1 (T_j X) = (Z^-1 T_i^-1 T_j) X, with Exp(x)^-1 = Exp(-x): group
    algebra only, so that the unperturbed products are formed once"""
    Tij = _rel(*Ti, *Tj)
    E = _rel(*Z, *Tij)
    r = se3_log(*E)
    Zi = _rel(*Z, _eye(3), [mp.mpf(0)] * 3)
    Ji, Jj = [], []
    for plus, minus in _steps():
        a, b = se3_log(*_compose(*E, *plus)), se3_log(*_compose(*E, *minus))
        Jj.append([(a[q] - b[q]) / (2 * H_DIFF) for q in range(6)])
        a, b = se3_log(*_compose(*Zi, *_compose(*minus, *Tij))), se3_log(*_compose(*Zi, *_compose(*plus, *Tij)))
        Ji.append([(a[q] - b[q]) / (2 * H_DIFF) for q in range(6)])
    return r, _tr(Ji), _tr(Jj)


@_prec
def edge_blocks(r, Ji, Jj, info, robust=False, delta=0.0):
    """the Gauss-Newton blocks of one edge: H_ii, H_ij, H_jj = J_a^T (w Omega) J_c and b_i, b_j = J_a^T (w Omega) r"""
    info = _m(info)
    _, w, _ = weight_and_rho(r, info, robust, mp.mpf(float(delta)))
    W = [[w * x for x in row] for row in info]
    Ai, Aj = _mm(_tr(Ji), W), _mm(_tr(Jj), W)
    return _mm(Ai, Ji), _mm(Ai, Jj), _mm(Aj, Jj), _mv(Ai, r), _mv(Aj, r)


@_prec
def jr_inv(r):
    """the exact Jr^-1(r) = sum_n B_n (-ad)^n / n! (Bernoulli numbers, B_1 = -1/2), ad(r) = [[w^, v^], [0, w^]], summed until a term is
    below 1e-90; converges for |w| < 2 pi"""
    ad = _ad(r)
    J, P, n = _eye(6), _eye(6), 0
    while True:
        n += 1
        P = [[-x / n for x in row] for row in _mm(P, ad)]                    # (-ad)^n / n!
        b = mp.bernoulli(n)
        if b == 0:
            continue
        term = max(abs(b * x) for row in P for x in row)
        J = _lin([(1, J), (b, P)], 6)
        if term < mp.mpf(10) ** -90 or n > 2000:
            break
    return J


def _ad(r):
    r = _m(r)
    V, W = _hat(r[:3]), _hat(r[3:])
    return [W[i] + V[i] for i in range(3)] + [[mp.mpf(0)] * 3 + W[i] for i in range(3)]


def ad_norm(r):
    """|ad(r)|_2 in float64 (it only enters bounds)"""
    with mp.workdps(DPS):
        return float(np.linalg.norm(f64(_ad(r)), 2))


# ---- whole graphs ----------------------------------------------------------------------------------------------------------------------

@_prec
def graph_poses(R, t):
    return [pose(R[n], t[n]) for n in range(len(R))]


@_prec
def graph_cost(g, R, t, delta):
    """the total cost of a graph of pose_graph_reference at the float64 poses (R, t)"""
    T = graph_poses(R, t)
    return mp.fsum(edge_cost(T[g["i"][e]], T[g["j"][e]], pose(g["R"][e], g["t"][e]), g["info"][e], bool(g["flags"][e] & 1), delta)
                   for e in range(len(g["i"])))


@_prec
def graph_system(g, R, t, delta, hessian=True):
    """the dense Gauss-Newton matrix H (6n x 6n, over ALL nodes; None unless asked for) and the half gradient b = sum J^T w Omega r (6n)
    of the true cost at the float64 poses, from the differenced Jacobians, in float64 (accumulated in mp)"""
    n = g["n"]
    T = graph_poses(R, t)
    z = mp.mpf(0)
    H = [[z] * (6 * n) for _ in range(6 * n)] if hessian else None
    b = [z] * (6 * n)
    for e in range(len(g["i"])):
        i, j = int(g["i"][e]), int(g["j"][e])
        r, Ji, Jj = edge_jacobians(T[i], T[j], pose(g["R"][e], g["t"][e]))
        Hii, Hij, Hjj, bi, bj = edge_blocks(r, Ji, Jj, g["info"][e], bool(g["flags"][e] & 1), delta)
        for a in range(6):
            b[6 * i + a] += bi[a]
            b[6 * j + a] += bj[a]
            for c in range(6 if hessian else 0):
                H[6 * i + a][6 * i + c] += Hii[a][c]
                H[6 * i + a][6 * j + c] += Hij[a][c]
                H[6 * j + c][6 * i + a] += Hij[a][c]
                H[6 * j + a][6 * j + c] += Hjj[a][c]
    return f64(H) if hessian else None, f64(b)


def gradient(g, R, t, delta):
    """|sum J^T w Omega r| over the free nodes, infinity norm: half the gradient of the true cost"""
    _, b = graph_system(g, R, t, delta, hessian=False)
    free = np.repeat(g["fixed"] == 0, 6)
    return float(np.abs(b[free]).max())


def dense_covariance(g, R, t, delta):
    """H^-1 over the free nodes, embedded in (6n, 6n) with zero rows and columns at fixed nodes.  The inverse is numpy's, refined by one
    Newton step X <- X + X (I - H X) in extended precision"""
    n = g["n"]
    H, _ = graph_system(g, R, t, delta)
    free = np.repeat(g["fixed"] == 0, 6)
    Hf = H[np.ix_(free, free)].astype(np.longdouble)
    X = np.linalg.inv(Hf.astype(np.float64)).astype(np.longdouble)
    X = X + X @ (np.eye(len(Hf), dtype=np.longdouble) - Hf @ X)
    C = np.zeros((6 * n, 6 * n))
    C[np.ix_(free, free)] = X.astype(np.float64)
    return C


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------

#: sin(theta) below which, with cos(theta) < 0, dvo_pg::se3_log takes the axis from the symmetric part (kNearPi of dvo_pose_graph.h)
NEAR_PI_SIN = 0.1
AXES = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.3, -0.5, 0.81), (0.0, 0.0, -1.0)]
TRANSLATIONS = [(0.0, 0.0, 0.0), (0.1, 0.2, 0.3), (30.0, -20.0, 10.0)]


def angles():
    """(label, theta as mpf): the sweep's rotation angles, with the doubles on either side of theta^2 = 1e-4 and of the switch of Log"""
    with mp.workdps(DPS):
        out = [("0", mp.mpf(0))] + [(s, mp.mpf(s)) for s in ("1e-12", "1e-8", "1e-3")]
        small = float(np.sqrt(1e-4))
        out += [("small-", mp.mpf(float(np.nextafter(small, 0.0)))), ("small+", mp.mpf(float(np.nextafter(small, 1.0))))]
        out += [(s, mp.mpf(s)) for s in ("0.1", "1", "2", "3")]
        sw = float(mp.pi - mp.asin(mp.mpf(NEAR_PI_SIN)))
        out += [("switch-1e-6", mp.mpf(sw - 1e-6)), ("switch-", mp.mpf(float(np.nextafter(sw, 0.0)))), ("switch+", mp.mpf(float(np.nextafter(sw, 4.0)))),
                ("switch+1e-6", mp.mpf(sw + 1e-6))]
        out += [("pi-" + s, mp.pi - mp.mpf(s)) for s in ("1e-2", "1e-4", "1e-6", "1e-8", "1e-9", "1e-10", "1e-12")]
        out.append(("pi", +mp.pi))
        return out


_SWEEP = []


def sweep():
    """every (angle, axis, translation) of the sweep, built once: dicts with label, theta (mpf), axis and translation indices, the
    float64 (R, t) handed to the code, and its reference Log r (mpf) -- r_flip too where theta is pi"""
    if _SWEEP:
        return _SWEEP
    with mp.workdps(DPS):
        for ka, (label, th) in enumerate(angles()):
            for kx, ax in enumerate(AXES):
                a = [mp.mpf(x) for x in ax]
                n = _norm(a)
                w = [th * x / n for x in a]
                R64 = f64(se3_exp([0, 0, 0] + w)[0])
                for kt, tr in enumerate(TRANSLATIONS):
                    t64 = np.array(tr)
                    T = pose(R64, t64)
                    _SWEEP.append(dict(label=label, theta=th, ka=ka, kx=kx, kt=kt, R=R64, t=t64, r=se3_log(*T),
                                       r_flip=se3_log(*T, flip=True) if label == "pi" else None))
    return _SWEEP


def log_error(r_code, item):
    """the tests' measure of a Log against the reference: max(|dv| / max(1, |t|), |dw|), infinity norms; at theta = pi the smaller of the
    two over the representatives"""
    scale = max(1.0, float(np.linalg.norm(item["t"])))
    best = None
    for ref in (item["r"], item["r_flip"]):
        if ref is None:
            continue
        with mp.workdps(DPS):
            d = [abs(mp.mpf(float(r_code[k])) - ref[k]) for k in range(6)]
            e = float(max(max(d[:3]) / scale, max(d[3:])))
        best = e if best is None else min(best, e)
    return best


ANISO = None


def aniso_information():
    """an SPD Omega with a condition number of 1e4, no two eigenvalues equal and no axis aligned: a fixed rotation of
    diag(1, 10^0.8, ..., 10^4); transposed or permuted blocks show under it"""
    global ANISO
    if ANISO is None:
        Q, _ = np.linalg.qr(np.random.default_rng(41).normal(size=(6, 6)))
        A = Q @ np.diag(10.0 ** np.linspace(0.0, 4.0, 6)) @ Q.T
        ANISO = 0.5 * (A + A.T)
    return ANISO


_PROBE = []
PROBE_T0 = np.array([0.3, -0.2, 0.5, 0.4, -0.7, 0.2])          # node 0 of every probe graph: Exp of this
PROBE_Z = np.array([-0.5, 0.8, 0.1, -0.3, 0.2, 0.9])           # the measurement of every probe graph: Exp of this


def probe_graphs():
    """the cost0 probe: a third of the sweep (one translation per angle and axis, in turn) as `pair`-shaped graphs -- two nodes, node 0
    fixed, one plain edge -- with T_1 = T_0 Z X rounded to float64, so that the residual is the sweep's X up to that rounding; each once
    with Omega = I and once with aniso_information().  At most 512 graphs.  Dicts of pose_graph_reference's graph form with `cost`
    (mpf) and `cost_flip` (at theta = pi) from the reference"""
    import pose_graph_reference as pg
    if _PROBE:
        return _PROBE
    with mp.workdps(DPS):
        T0m, Zm = se3_exp(PROBE_T0), se3_exp(PROBE_Z)
        R0, t0, ZR, Zt = f64(T0m[0]), f64(T0m[1]), f64(Zm[0]), f64(Zm[1])
        T0, Z = pose(R0, t0), pose(ZR, Zt)
        for item in sweep():
            if (item["ka"] + item["kx"] + item["kt"]) % 3:
                continue
            T1m = compose(T0, Z, pose(item["R"], item["t"]))
            R1, t1 = f64(T1m[0]), f64(T1m[1])
            T1 = pose(R1, t1)
            for kind, info in (("I", np.eye(6)), ("aniso", aniso_information())):
                g = pg._graph("probe %s %d %d %s" % (item["label"], item["kx"], item["kt"], kind), np.stack([R0, R1]), np.stack([t0, t1]),
                              [1, 0], [0], [1], ZR, Zt, info[None], [0], None)
                g["cost"] = edge_cost(T0, T1, Z, info)
                g["cost_flip"] = edge_cost(T0, T1, Z, info, flip=True) if item["label"] == "pi" else None
                g["label"] = item["label"]
                _PROBE.append(g)
    assert len(_PROBE) <= 512
    return _PROBE


def cost_error(cost, g):
    """the error of a float64 cost0 against the reference's (the nearer representative at theta = pi), relative to the cost -- or to
    |Omega|_2, the cost of a unit residual, where that is larger: the poses are float64, so r carries an absolute error of about
    eps max(1, |t|) however small it is, and a cost below that scale has no relative accuracy to speak of (at theta = 0 and t = 0 the
    cost is the square of that error)"""
    best = None
    with mp.workdps(DPS):
        floor = mp.mpf(float(np.linalg.norm(g["info"][0], 2)))
        for ref in (g["cost"], g["cost_flip"]):
            if ref is None:
                continue
            e = float(abs(mp.mpf(float(cost)) - ref) / max(ref, floor))
            best = e if best is None else min(best, e)
    return best
