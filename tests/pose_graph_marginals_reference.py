"""Marginal covariances of pose graphs (include/dvo_amd.h, "pose graphs", MARGINAL COVARIANCES): the dense reference the tests compare
dvo_graph_marginals_host and dvo_graph_marginals with, a numpy restatement of dvo_graph_edge_chi2, and the queries the tests run.

The reference is not a restatement of the definition's CG: it builds the dense undamped Gauss-Newton matrix H over the free nodes from
pose_graph_reference.linearise (scattering Hii, Hij, Hij^T, Hjj), inverts it with np.linalg.inv and picks the joint blocks, with zero
rows and columns for fixed nodes."""
import numpy as np

import pose_graph_reference as pg

#: the worst max|cov - dense| / max|dense joint block| of dvo_graph_marginals_host (cg_tol = 1e-12) over the cases and queries of
#: tests/test_pose_graph_marginals_cpu.py, measured on the CPU (profiles/pose_graph_marginals/README.md); `star` sets it
HOST_AGAINST_DENSE_MEASURED = 4.42e-13
#: what the tests assert, for the host definition against the dense inverse and for the device against the host definition: the margin
#: covers the difference between the definition's sum order and any other order, and nothing else
TOLERANCE = 100.0 * HOST_AGAINST_DENSE_MEASURED

CG_TOL = 1e-12


def dense_hessian(g, R, t, delta=pg.DEFAULTS["huber_delta"]):
    """the undamped Gauss-Newton matrix over ALL nodes, (6n, 6n)"""
    n = g["n"]
    H = np.zeros((6 * n, 6 * n))
    if len(g["i"]) == 0:
        return H
    Hii, Hij, Hjj, _, _ = pg.linearise(g, R, t, delta)
    for e, (i, j) in enumerate(zip(g["i"], g["j"])):
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        H[si, si] += Hii[e]
        H[si, sj] += Hij[e]
        H[sj, si] += Hij[e].T
        H[sj, sj] += Hjj[e]
    return H


_DENSE = {}


def dense_covariance(g, R, t, key=None, delta=pg.DEFAULTS["huber_delta"]):
    """H^-1 over the free nodes, embedded in (6n, 6n) with zero rows and columns at fixed nodes; cached under `key`"""
    if key is not None and key in _DENSE:
        return _DENSE[key]
    n = g["n"]
    free = np.repeat(g["fixed"] == 0, 6)
    C = np.zeros((6 * n, 6 * n))
    if free.any():
        H = dense_hessian(g, R, t, delta)
        C[np.ix_(free, free)] = np.linalg.inv(H[np.ix_(free, free)])
    if key is not None:
        _DENSE[key] = C
    return C


def joint(C, nodes):
    """the joint covariance of the listed nodes out of the full matrix"""
    idx = np.concatenate([np.arange(6 * c, 6 * c + 6) for c in nodes])
    return C[np.ix_(idx, idx)]


def distance(cov, dense):
    """the tests' measure: max|cov - dense| / max|dense joint block| (0 for a block that is all zero and matched exactly)"""
    scale = np.abs(dense).max()
    d = np.abs(cov - dense).max()
    return d / scale if scale > 0.0 else d


def edge_jacobians(g, e, R, t):
    """r (6,), J_i, J_j (6, 6) of edge e at the poses, as pose_graph_reference.linearise forms them"""
    one = pg._graph("edge", R, t, g["fixed"], [g["i"][e]], [g["j"][e]], g["R"][e:e + 1], g["t"][e:e + 1], g["info"][e:e + 1], [0], None)
    r, Rij, tij = pg.residuals(one, R, t)
    Jj = pg.jr_inv(r)
    Rt = Rij.transpose(0, 2, 1)
    tt = -np.stack([pg._seq([Rij[:, k, a] * tij[:, k] for k in range(3)]) for a in range(3)], axis=1)
    Ad = np.zeros((1, 6, 6))
    Ad[:, :3, :3] = Rt
    Ad[:, 3:, 3:] = Rt
    Ad[:, 0, 3:] = tt[:, 1, None] * Rt[:, 2, :] - tt[:, 2, None] * Rt[:, 1, :]
    Ad[:, 1, 3:] = tt[:, 2, None] * Rt[:, 0, :] - tt[:, 0, None] * Rt[:, 2, :]
    Ad[:, 2, 3:] = tt[:, 0, None] * Rt[:, 1, :] - tt[:, 1, None] * Rt[:, 0, :]
    Ji = -pg._mul6(Jj, Ad)
    return r[0], Ji[0], Jj[0]


def edge_chi2(g, e, R, t, cov):
    """the restatement of dvo_graph_edge_chi2 for edge e of g at the poses: (r, S, chi2); cov (12, 12) or None"""
    r, Ji, Jj = edge_jacobians(g, e, R, t)
    S = np.linalg.inv(g["info"][e])
    if cov is not None:
        J = np.concatenate([Ji, Jj], axis=1)
        S = J @ cov @ J.T + S
    return r, S, float(r @ np.linalg.solve(S, r))


def queries(g):
    """the node lists a case is asked for: m = 1, 2 and 3, with the first free node, the last node and two neighbours; a case with a
    second fixed node lists it"""
    n = g["n"]
    first = int(np.nonzero(g["fixed"] == 0)[0][0]) if (g["fixed"] == 0).any() else 0
    last = n - 1
    if n == 2:
        return [[first], [0, 1], [1, 0]]
    second = int(np.nonzero(g["fixed"] == 0)[0][1])                      # the next free node: the first one's neighbour on a ring
    if n > 500:                                                          # the long columns: one query of each size, fewer columns
        return [[last], [first, second, last]]
    out = [[first], [last], [first, second], [last, first], [first, second, last]]
    extra = [int(k) for k in np.nonzero(g["fixed"])[0] if k != 0]
    if extra:
        out += [[extra[0]], [first, extra[0]], [extra[0] - 1, extra[0], last]]
    return out
