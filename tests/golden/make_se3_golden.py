#!/usr/bin/env python3
"""Generates tests/golden/se3_golden.npz: the SE(3) helpers of the pose update (exp, log, rotationize) at their branch thresholds,
with expected values from tests/se3_reference.py (mpmath, 50 digits) rounded to double, and the CPU oracle's error on each case.

The oracle cannot judge the device here: its closed forms cancel in 1e-10 <= theta < 0.1 (its translation is off by ~1e-8 |upsilon|
at theta = 1e-8), the very range the tracker lives in.  So the fixture carries the 50-digit values, and the oracle's error against
them only sets the scale: per quantity, its largest normalised error over its WELL-CONDITIONED cases (never below 2^-52) is the
baseline; the GPU test allows the device 4 x baseline on every case.

Normalisation: R and omega absolute; t of exp over |upsilon|; upsilon of log over |t|; the polar factor over sigma1/(sigma2+sigma3).
Rotations beyond pi - 1e-5 are compared as group elements (exp of the logarithm against the input): the sign of theta is open there.

    python tests/golden/make_se3_golden.py          # rewrites se3_golden.npz (needs mpmath)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20260607
PI = float.fromhex("0x1.921fb54442d18p+1")
MAGS = (1e-3, 1.0, 1e3)                     # |upsilon| of exp, |t| of log
FLOOR = 2.0 ** -52
# the exp thresholds of the device compare theta^2, Sophus compares theta: 1e-3 relative on either side of 1e-10, never the value itself
THETAS_EXP = ([0.0, 1e-12, 0.99e-10, 1.01e-10] + [10.0 ** -k for k in range(9, 2, -1)] +
              [3e-3, 0.00999, 0.01001, 0.05, 0.5, PI / 2 - 1e-3, PI / 2 + 1e-3, 2.0, PI - 1e-6, PI, PI + 1e-6,
               2 * PI - 1e-3, 2 * PI + 1e-3, 3 * PI, 4 * PI - 1e-3])
THETAS_LOG = sorted([th for th in THETAS_EXP if th <= PI] + [0.0999, 0.1001, 2 * PI / 3 - 1e-3, 2 * PI / 3 + 1e-3])
THETAS_LOG_FAR = (2.2, 2.6, 3.0, 3.14)      # trace <= 0: each diagonal entry the largest in turn, both signs of w
AXES_DOMINANT = [(1.0, 0.11, -0.07), (-1.0, 0.05, 0.13), (0.09, 1.0, 0.12), (-0.14, -1.0, 0.06), (0.08, -0.1, 1.0), (0.12, 0.07, -1.0)]
AXES_GENERIC = [(0.6, -0.5, 0.62), (-0.45, 0.7, 0.55)]
ROUND_TRIP_FROM = PI - 1e-5

ROT_REGULAR, ROT_AS_IS, ROT_NAN = 0, 1, 2


def _unit(a):
    a = np.asarray(a, np.float64)
    return a / np.linalg.norm(a)


def _f(x):
    return float(x)


def build():
    import oracle_lib
    import se3_reference as ref
    oracle = oracle_lib.load()
    rng = np.random.default_rng(SEED)
    axes = [_unit(a) for a in AXES_DOMINANT + AXES_GENERIC]
    out = {"mags": np.array(MAGS)}

    def arr(x):
        return np.array(ref.to_double(x), np.float64)

    # ---- exp ------------------------------------------------------------------------------------------------------------------
    om, ud, R_, t_, th_, eR, et = [], [], [], [], [], [], []
    for th in THETAS_EXP:
        for ax in axes:
            omega = th * ax
            u = _unit(rng.standard_normal(3))
            Rm, _ = ref.exp(np.concatenate([u, omega]))
            om.append(omega); ud.append(u); th_.append(th); R_.append(arr(Rm))
            ts, es = [], []
            for k, mag in enumerate(MAGS):
                psi = np.concatenate([mag * u, omega])
                _, tm = ref.exp(psi)
                Ro, to = oracle.se3_exp(psi)
                if k == 0:
                    eR.append(_f(ref.max_abs_diff(np.asarray(Ro).tolist(), Rm)))
                ts.append(arr(tm))
                es.append(_f(ref.max_abs_diff(to.tolist(), tm) / ref.norm(ref.vec(psi[:3]))))
            t_.append(ts); et.append(es)
    out.update(exp_omega=np.array(om), exp_udir=np.array(ud), exp_theta=np.array(th_), exp_R=np.array(R_), exp_t=np.array(t_),
               exp_oracle_err_R=np.array(eR), exp_oracle_err_t=np.array(et))
    well = (out["exp_theta"] >= 0.1) | (out["exp_theta"] < 1e-10)
    out["base_exp_R"] = np.array(max(FLOOR, out["exp_oracle_err_R"].max()))
    out["base_exp_t"] = np.array(max(FLOOR, out["exp_oracle_err_t"][well].max()))

    # ---- log ------------------------------------------------------------------------------------------------------------------
    rots = [(th, ax) for th in THETAS_LOG for ax in axes] + [(th, _unit(a)) for th in THETAS_LOG_FAR for a in AXES_DOMINANT]
    Rin, td, w_, v_, th_, rt, ew, ev = [], [], [], [], [], [], [], []
    for th, ax in rots:
        R = arr(ref.so3_exp(th * ax))                 # the rotation in 50 digits, rounded to double: the input
        d = _unit(rng.standard_normal(3))
        round_trip = th > ROUND_TRIP_FROM
        Rin.append(R); td.append(d); th_.append(th); rt.append(round_trip)
        vs, es = [], []
        for k, mag in enumerate(MAGS):
            t = mag * d
            pm = ref.log(R, t)
            po = oracle.se3_log(R, t)
            if round_trip:
                Rb, tb = ref.exp(po)
                e_w = ref.max_abs_diff(R.tolist(), Rb)
                e_v = ref.max_abs_diff(t.tolist(), tb) / ref.norm(ref.vec(t))
            else:
                e_w = ref.max_abs_diff(po[3:].tolist(), pm[3:])
                e_v = ref.max_abs_diff(po[:3].tolist(), pm[:3]) / ref.norm(ref.vec(t))
            if k == 0:
                w_.append(arr(pm[3:])); ew.append(_f(e_w))
            vs.append(arr(pm[:3])); es.append(_f(e_v))
        v_.append(vs); ev.append(es)
    out.update(log_R=np.array(Rin), log_tdir=np.array(td), log_theta=np.array(th_), log_round_trip=np.array(rt, np.uint8),
               log_omega=np.array(w_), log_upsilon=np.array(v_), log_oracle_err_omega=np.array(ew), log_oracle_err_upsilon=np.array(ev))
    r = out["log_round_trip"].astype(bool)
    out["base_log_omega"] = np.array(max(FLOOR, out["log_oracle_err_omega"][~r].max()))
    out["base_log_upsilon"] = np.array(max(FLOOR, out["log_oracle_err_upsilon"][~r].max()))
    out["base_log_round_trip_R"] = np.array(max(FLOOR, out["log_oracle_err_omega"][r].max()))
    out["base_log_round_trip_t"] = np.array(max(FLOOR, out["log_oracle_err_upsilon"][r].max()))

    # ---- rotationize ----------------------------------------------------------------------------------------------------------
    def rot(th, ax):
        return arr(ref.so3_exp(th * _unit(ax)))

    base = [rot(0.0, (1, 0, 0)), rot(0.3, (0.6, -0.5, 0.62)), rot(2.5, (-0.14, -1.0, 0.06)), rot(PI, (0.12, 0.07, -1.0))]
    mats, kinds = [], []
    for R in base:
        mats.append(R)
    for noise in (1e-8, 1e-3):
        for R in base[1:]:
            mats.append(R + noise * rng.standard_normal((3, 3)))
    for scale in (1e-3, 1e3):
        for R in base[1:3]:
            mats.append(scale * R)
    for sv in ((1.0, 1.0, 1e-6), (1.0, 1e-3, 1e-6)):
        for a, b in ((1, 2), (3, 1)):
            mats.append(base[a] @ np.diag(sv) @ base[b].T)
    for R in base[1:3]:                                # reflections: det < 0, the polar factor has det -1
        mats.append(R @ np.diag([1.0, 1.0, -1.0]) + 1e-3 * rng.standard_normal((3, 3)))
    kinds += [ROT_REGULAR] * len(mats)
    mats += [np.diag([1.0, 1.0, 0.0]), np.zeros((3, 3))]        # singular: the device leaves the matrix as it is
    kinds += [ROT_AS_IS] * 2
    bad = base[1].copy()
    bad[1, 2] = np.nan
    mats.append(bad); kinds.append(ROT_NAN)
    want, cond, err = [], [], []
    for A, kind in zip(mats, kinds):
        if kind == ROT_REGULAR:
            P = ref.polar(A)
            s = ref.singular_values(A)
            c = s[0] / (s[1] + s[2])
            want.append(arr(P)); cond.append(_f(c))
            err.append(_f(ref.max_abs_diff(oracle.rotationize(A).tolist(), P) / c))
        else:
            want.append(A.copy()); cond.append(1.0); err.append(np.nan)     # the oracle's SVD answers these differently: not judged
    out.update(rot_in=np.array(mats), rot_out=np.array(want), rot_kind=np.array(kinds, np.uint8), rot_cond=np.array(cond),
               rot_oracle_err=np.array(err))
    out["base_polar"] = np.array(max(FLOOR, np.nanmax(out["rot_oracle_err"])))
    return out


if __name__ == "__main__":
    data = build()
    path = os.path.join(HERE, "se3_golden.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes,", len(data), "arrays")
    for k in sorted(data):
        if k.startswith("base_"):
            print("  %-24s %.3e" % (k, float(data[k])))
