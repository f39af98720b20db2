"""tests/golden/se3_golden.npz (50-digit values of exp, log and the polar factor at the branch thresholds of the device's update
math) against the CPU oracle: the fixture is pinned to the oracle, the baselines it carries are the oracle's, and -- where mpmath
imports -- the generator reproduces the committed file bit for bit.  No GPU.

The committed expected values are the 50-digit ones ROUNDED to double, the recorded errors were taken against the unrounded ones:
an error measured here may exceed its record by that rounding, at most 2^-53 of the largest expected entry (in the quantity's
normalisation), and by nothing else -- the difference of two doubles this close is exact.
"""
import os
import sys

import numpy as np
import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "se3_golden.npz")
PI = float.fromhex("0x1.921fb54442d18p+1")


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLDEN) < 100 * 1000
    return dict(np.load(GOLDEN))


def _rounding(want, scale=1.0):
    return 2.0 ** -53 * np.abs(want).max() / scale * (1 + 1e-6)


def oracle_errors(gold, oracle):
    """the oracle's normalised error on every case against the committed doubles, with the rounding allowance of each:
    dict name -> (error array, allowance array), shaped like the fixture's *_oracle_err_* arrays"""
    mags = gold["mags"]
    n = len(gold["exp_theta"])
    eR, aR, et, at = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        for k, mag in enumerate(mags):
            psi = np.concatenate([mag * gold["exp_udir"][i], gold["exp_omega"][i]])
            R, t = oracle.se3_exp(psi)
            nu = np.linalg.norm(psi[:3])
            et[i, k], at[i, k] = np.abs(t - gold["exp_t"][i, k]).max() / nu, _rounding(gold["exp_t"][i, k], nu)
            if k == 0:
                eR[i], aR[i] = np.abs(np.asarray(R) - gold["exp_R"][i]).max(), _rounding(gold["exp_R"][i])
    m = len(gold["log_theta"])
    ew, aw, ev, av = np.zeros(m), np.zeros(m), np.zeros((m, 3)), np.zeros((m, 3))
    for i in range(m):
        if gold["log_round_trip"][i]:
            continue                      # judged as group elements: needs exp in 50 digits (the regeneration test covers them)
        for k, mag in enumerate(mags):
            t = mag * gold["log_tdir"][i]
            psi = oracle.se3_log(gold["log_R"][i], t)
            nt = np.linalg.norm(t)
            ev[i, k], av[i, k] = np.abs(psi[:3] - gold["log_upsilon"][i, k]).max() / nt, _rounding(gold["log_upsilon"][i, k], nt)
            if k == 0:
                ew[i], aw[i] = np.abs(psi[3:] - gold["log_omega"][i]).max(), _rounding(gold["log_omega"][i])
    r = len(gold["rot_kind"])
    ep, ap = np.full(r, np.nan), np.zeros(r)
    for i in range(r):
        if gold["rot_kind"][i] == 0:
            c = gold["rot_cond"][i]
            ep[i], ap[i] = np.abs(oracle.rotationize(gold["rot_in"][i]) - gold["rot_out"][i]).max() / c, _rounding(gold["rot_out"][i], c)
    return dict(exp_R=(eR, aR), exp_t=(et, at), log_omega=(ew, aw), log_upsilon=(ev, av), polar=(ep, ap))


@pytest.fixture(scope="module")
def errors(gold, oracle):
    return oracle_errors(gold, oracle)


def test_oracle_is_within_its_recorded_error_on_every_case(gold, errors):
    rt = gold["log_round_trip"].astype(bool)
    for name, rec, keep in (("exp_R", gold["exp_oracle_err_R"], None), ("exp_t", gold["exp_oracle_err_t"], None),
                            ("log_omega", gold["log_oracle_err_omega"], ~rt), ("log_upsilon", gold["log_oracle_err_upsilon"], ~rt),
                            ("polar", gold["rot_oracle_err"], gold["rot_kind"] == 0)):
        err, allow = errors[name]
        keep = np.ones(len(err), bool) if keep is None else keep
        over = err[keep] - (rec[keep] + allow[keep])
        assert np.all(over <= 0), (name, np.argwhere(over > 0)[:5], over.max())
    assert np.isnan(gold["rot_oracle_err"][gold["rot_kind"] != 0]).all()


def test_oracle_is_within_the_baseline_on_the_well_conditioned_cases(gold, errors):
    """what gives the baselines their meaning: on the cases where its closed forms do not cancel, the oracle alone stays within
    1 x baseline of the 50-digit value -- and outside them it does not (so the device is not being judged by the oracle)"""
    th = gold["exp_theta"]
    well = (th >= 0.1) | (th < 1e-10)
    rt = gold["log_round_trip"].astype(bool)
    for name, base, keep in (("exp_R", "base_exp_R", np.ones(len(th), bool)), ("exp_t", "base_exp_t", well),
                             ("log_omega", "base_log_omega", ~rt), ("log_upsilon", "base_log_upsilon", ~rt),
                             ("polar", "base_polar", gold["rot_kind"] == 0)):
        err, allow = errors[name]
        b = float(gold[base])
        assert b >= 2.0 ** -52
        assert np.all(err[keep] <= b + allow[keep]), (name, b, err[keep].max())
    for name in ("base_log_round_trip_R", "base_log_round_trip_t"):
        assert float(gold[name]) >= 2.0 ** -52
    et = errors["exp_t"][0]
    assert et[~well].max() > 1e4 * float(gold["base_exp_t"])           # ~1e-8 at theta = 1e-8
    assert et[np.isclose(th, 1e-8)].max() > 1e-9


def test_fixture_reaches_every_branch(gold):
    """the cases exist for branches; a fixture that no longer reaches one must not pass quietly"""
    th = gold["exp_theta"]
    for lo, hi in ((0.0, 1e-10), (1e-10, 1e-2), (1e-2, 4 * PI)):        # se3_exp_q: small angle, series, closed forms
        assert np.count_nonzero((th >= lo) & (th < hi)) >= 16
    for edge in (1e-10, 1e-2):                                          # both sides of each threshold, never the value itself
        rel = th[th > 0] / edge - 1
        assert np.any((rel > 1e-4) & (rel < 2e-2)) and np.any((rel < -1e-4) & (rel > -2e-2)) and not np.any(np.abs(rel) < 1e-4)
    assert th.max() > 4 * PI - 2e-3 and np.any(np.abs(th - PI) < 1e-9) and np.any(th == 0)
    lt = gold["log_theta"]
    for edge in (0.1, 2 * PI / 3):
        assert np.any((lt > edge) & (lt < edge * 1.002)) and np.any((lt < edge) & (lt > edge * 0.998))
    seen = set()
    for R in gold["log_R"]:                                             # quat_of_matrix, trace <= 0: (largest diagonal, sign of w)
        if np.trace(R) <= 0:
            i = int(np.argmax(np.diag(R)))
            j, k = (i + 1) % 3, (i + 2) % 3
            seen.add((i, bool(R[k, j] - R[j, k] > 0)))
    assert seen == {(i, s) for i in range(3) for s in (False, True)}
    assert np.count_nonzero(np.trace(gold["log_R"], axis1=1, axis2=2) > 0) > 100
    assert gold["log_round_trip"].sum() >= 8 and np.all(lt[gold["log_round_trip"].astype(bool)] > PI - 1e-5)
    kinds = gold["rot_kind"]
    assert (kinds == 1).sum() == 2 and (kinds == 2).sum() == 1 and np.isnan(gold["rot_in"][kinds == 2]).any()
    reg = kinds == 0
    dets = np.linalg.det(gold["rot_in"][reg])
    assert np.any(dets < 0) and np.all(np.sign(np.linalg.det(gold["rot_out"][reg])) == np.sign(dets))
    assert gold["rot_cond"][reg].max() > 500 and gold["rot_cond"][reg].min() <= 0.5 + 1e-6


def test_generator_reproduces_the_committed_fixture():
    pytest.importorskip("mpmath")
    sys.path.insert(0, GOLDEN_DIR)
    try:
        import make_se3_golden
    finally:
        sys.path.remove(GOLDEN_DIR)
    fresh = make_se3_golden.build()
    kept = np.load(GOLDEN)
    assert sorted(fresh) == sorted(kept.files)
    for k in kept.files:
        a, b = np.asarray(fresh[k]), kept[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
