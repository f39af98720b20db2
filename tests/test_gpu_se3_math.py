"""The double-precision helpers of the pose update (dvo_device_math.h: se3_exp_q, se3_log_q, quat_of_matrix, rotationize and the
hand-written reciprocal / square root / sin / cos / atan under them) on every case of tests/golden/se3_golden.npz, against the
50-digit values the fixture carries -- not against the oracle, whose closed forms cancel in 1e-10 <= theta < 0.1.

Bound: 4 x the oracle's own largest error on ITS well-conditioned cases (the fixture's base_* values, never below 2^-52), on EVERY
case.  The device's primitives are within ~1 ulp where libm is correctly rounded, over chains of the same length, and its series
have no cancellation; a wrong branch, sign, threshold side or permutation shows at 1e-11 or more.  Normalisation as in the
generator: R, omega absolute; t over |upsilon|; upsilon over |t|; the polar factor over sigma1/(sigma2+sigma3).  Beyond pi - 1e-5
the logarithm is judged as a group element: exp (in extended precision, here) of what the device returned against the input.

The measured maxima per quantity and band are printed before anything is asserted.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se3_golden.npz")
FACTOR = 4.0


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def ctx():
    from rgbd_odometry_amd import DvoContext
    with DvoContext(1) as c:
        yield c


def _report(rows):
    """rows: (quantity, band, measured maximum, baseline); prints them all, then returns the ones over FACTOR x baseline"""
    bad = []
    for q, band, worst, base in rows:
        print("se3-math  %-22s %-26s max %.3e   baseline %.3e   factor %.2f" % (q, band, worst, base, worst / base))
        if not worst <= FACTOR * base:
            bad.append((q, band, worst, base))
    return bad


def _exp_extended(psi):
    """(R, t) of psi in the platform's extended precision (x87: 64-bit significand), closed forms; theta ~ pi only"""
    L = np.longdouble
    assert np.finfo(L).eps < 1e-18, "no extended precision on this platform"
    u, w = np.asarray(psi[:3], L), np.asarray(psi[3:], L)
    th = np.sqrt(w @ w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], L)
    W2 = W @ W
    I = np.eye(3, dtype=L)
    R = I + (np.sin(th) / th) * W + ((1 - np.cos(th)) / (th * th)) * W2
    V = I + ((1 - np.cos(th)) / (th * th)) * W + ((th - np.sin(th)) / (th * th * th)) * W2
    return R, V @ u


def test_se3_exp_on_every_fixture_case(gold, ctx):
    th, mags = gold["exp_theta"], gold["mags"]
    n = len(th)
    eR, et = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        for k, mag in enumerate(mags):
            psi = np.concatenate([mag * gold["exp_udir"][i], gold["exp_omega"][i]])
            R, t = ctx.se3_exp(psi)
            eR[i, k] = np.abs(R - gold["exp_R"][i]).max()
            et[i, k] = np.abs(t - gold["exp_t"][i, k]).max() / np.linalg.norm(psi[:3])
    bands = (("theta < 1e-10", th < 1e-10), ("1e-10 <= theta < 1e-4", (th >= 1e-10) & (th < 1e-4)),
             ("1e-4 <= theta < 0.01", (th >= 1e-4) & (th < 0.01)), ("0.01 <= theta < 0.1", (th >= 0.01) & (th < 0.1)),
             ("0.1 <= theta <= pi", (th >= 0.1) & (th < 3.1416)), ("pi < theta < 4 pi", th >= 3.1416))
    assert sum(int(m.sum()) for _, m in bands) == n
    rows = []
    for name, m in bands:
        rows.append(("exp R", name, eR[m].max(), float(gold["base_exp_R"])))
        rows.append(("exp t/|upsilon|", name, et[m].max(), float(gold["base_exp_t"])))
    bad = _report(rows)
    assert not bad, bad
    assert np.all(eR <= FACTOR * gold["base_exp_R"]) and np.all(et <= FACTOR * gold["base_exp_t"])


def test_se3_log_on_every_fixture_case(gold, ctx):
    th, mags = gold["log_theta"], gold["mags"]
    rt = gold["log_round_trip"].astype(bool)
    n = len(th)
    ew, ev = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        R = gold["log_R"][i]
        for k, mag in enumerate(mags):
            t = mag * gold["log_tdir"][i]
            psi = ctx.se3_log(R, t)
            assert np.all(np.isfinite(psi)), (i, k, psi)
            if rt[i]:
                Rb, tb = _exp_extended(psi)
                ew[i, k] = float(np.abs(Rb - R).max())
                ev[i, k] = float(np.abs(tb - t).max()) / np.linalg.norm(t)
            else:
                ew[i, k] = np.abs(psi[3:] - gold["log_omega"][i]).max()
                ev[i, k] = np.abs(psi[:3] - gold["log_upsilon"][i, k]).max() / np.linalg.norm(t)
    trace = np.trace(gold["log_R"], axis1=1, axis2=2)
    bands = (("theta < 0.1 (series)", ~rt & (th < 0.1)), ("theta >= 0.1, trace > 0", ~rt & (th >= 0.1) & (trace > 0)),
             ("trace <= 0", ~rt & (trace <= 0)))
    assert sum(int(m.sum()) for _, m in bands) + int(rt.sum()) == n
    rows = []
    for name, m in bands:
        rows.append(("log omega", name, ew[m].max(), float(gold["base_log_omega"])))
        rows.append(("log upsilon/|t|", name, ev[m].max(), float(gold["base_log_upsilon"])))
    rows.append(("exp(log) R", "theta > pi - 1e-5", ew[rt].max(), float(gold["base_log_round_trip_R"])))
    rows.append(("exp(log) t/|t|", "theta > pi - 1e-5", ev[rt].max(), float(gold["base_log_round_trip_t"])))
    bad = _report(rows)
    assert not bad, bad


def test_rotationize_on_every_fixture_case(gold, ctx):
    kinds = gold["rot_kind"]
    err = np.zeros(len(kinds))
    for i, A in enumerate(gold["rot_in"]):
        got = ctx.rotationize(A)
        if kinds[i] == 1:                       # singular: left as it is, bit for bit
            assert got.tobytes(order="C") == np.ascontiguousarray(gold["rot_out"][i]).tobytes(), (i, got)
        elif kinds[i] == 2:                     # a NaN inside: the call returns, and says so in its output
            assert np.isnan(got).any(), (i, got)
        else:
            err[i] = np.abs(got - gold["rot_out"][i]).max() / gold["rot_cond"][i]
    reg = kinds == 0
    cond = gold["rot_cond"]
    rows = [("polar factor / cond", name, err[reg & m].max(), float(gold["base_polar"]))
            for name, m in (("cond <= 1", cond <= 1), ("cond > 1", cond > 1))]
    bad = _report(rows)
    assert not bad, bad
