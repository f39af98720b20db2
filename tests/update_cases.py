"""Named cases for the pose update's parameters and for the branches the default parameters never reach.  TEST INFRASTRUCTURE ONLY.

Under the default parameters every step of the suite's synthetic scenes is clamped at the trust radius (|psi| = 3e-3, theta ~ 1.4e-3):
the unclamped branch of pose_apply, termination after iteration 0, the general branch of se3_exp_q (theta >= 0.01), the general
branch of se3_log_q and the trace <= 0 branches of quat_of_matrix never run inside an alignment kernel, and a kernel that ignored one
of the parameters UpdConst carries would pass.  Every case here changes one thing, and says -- as an assertion on the ORACLE's trace
(run_iterations(..., params=p, trace=True)) -- which branch it exists for; assert_reaches_branch() runs in a CPU test and again at the
head of the GPU tests, so a case that stops covering its branch fails instead of passing.

Scene: SynthScene(320, 240, 4, 0), level 3 (40x30, 423 points) and level 2 (80x60, 910 points).

Start poses beyond 0.1 rad come in two forms.  "carried": the reference points go along, xyz' = float32(R0 xyz + t0), so the scene
stays in view (visible ratio ~0.97-0.99) -- but such a list is no enlistRefEdgePts list any more, and the engine gives it to the
one-point-per-lane kernels only.  "in place": the points stay where they are and the view turns away (visible ratio 0.25-0.8: points
behind the camera project too, and the energies still change every iteration); this form reaches the packed kernels.  The update sees
the same log(pose) branches either way.

Thresholds and counts were re-derived from the oracle's trace of this scene: with step_a = 1e-4 at level 3, |psi| runs
1.70e-3, 2.33e-3, 2.67e-3, 2.95e-3, 3e-3 (clamped), 3e-3 (clamped), 1.53e-3, 1.02e-3, 7.70e-4, 6.33e-4, 5.34e-4, 4.60e-4.
Three parameters change nothing while every step is clamped (the clamp removes the step's length, and lambda = 1 is 1e-4 of |g|):
reg_lambda, the step decay and step_b are therefore tried on top of step_a = 1e-4, the regulariser with lambda = 50, and each must
change the energies against that base.  enable_rotationize = 0 cannot change an energy from a start pose that is a rotation (the
oracle then skips a projection that moves the pose by ~1e-16, and the device carries a unit quaternion either way): its case asserts
exactly that, and checks that the flag reaches every kernel without harm.
"""
from __future__ import annotations

import numpy as np

import oracle_lib

SCENE = (320, 240, 4, 0)
ITERS = 12
UNCLAMPED = dict(step_a=1e-4)
STOP = 9e-4                      # between 1.02e-3 (iteration 7) and 7.70e-4 (iteration 8) of the step_a = 1e-4 trace at level 3
T_START = (0.2, -0.15, 0.17)     # ~0.3 m

_cache = {}


def scene(oracle):
    if "scene" not in _cache:
        from rgbd_odometry_amd import SynthScene
        sc = SynthScene(*SCENE)
        _cache["scene"] = (sc, oracle_lib.scene_levels(sc, oracle))
    return _cache["scene"]


def rotation(theta, axis):
    """Rodrigues, in double (start poses only: any matrix within rounding of a rotation will do)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    W = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(theta) * W + (1 - np.cos(theta)) * (W @ W)


class Case:
    def __init__(self, name, branch, check, overrides=None, level=3, iters=ITERS, start=None, carried=False, base=None):
        self.name, self.branch, self.check = name, branch, check
        self.overrides = dict(overrides or {})
        self.level, self.iters, self.carried, self.base = level, iters, carried, base
        self.R0, self.t0 = (np.eye(3), np.zeros(3)) if start is None else (rotation(*start), np.array(T_START))
        self.start = start

    @property
    def key(self):
        """the parameter set: one engine context serves every case with the same key"""
        return tuple(sorted(self.overrides.items()))

    def xyz(self, oracle, level=None):
        """the reference list of `level` as this case hands it to the engine and to the oracle"""
        L = scene(oracle)[1][self.level if level is None else level]
        if not self.carried:
            return L["xyz"]
        return (L["xyz"].astype(np.float64) @ self.R0.T + self.t0).astype(np.float32)

    def __repr__(self):
        return self.name


def params(oracle, overrides):
    p = oracle.default_params()
    for k, v in overrides.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def reference(oracle, case):
    """the oracle's traced run of the case, computed once and shared: callers do not modify it"""
    if case.name not in _cache:
        sc, lv = scene(oracle)
        L = lv[case.level]
        _cache[case.name] = oracle.run_iterations(case.level, case.iters, case.xyz(oracle), L["dt"], L["gx"], L["gy"], L["rows"], L["cols"],
                                                  sc.intrinsics, case.R0, case.t0, params=params(oracle, case.overrides), trace=True)
    return _cache[case.name]


def pyramid_reference(oracle, case, iters=(0, 0, ITERS, ITERS)):
    """the oracle's coarse-to-fine run over levels 3 -> 2 of the case's parameters and start pose"""
    key = (case.name, tuple(iters))
    if key not in _cache:
        sc, lv = scene(oracle)
        lv = [dict(L, xyz=case.xyz(oracle, l)) for l, L in enumerate(lv)]
        _cache[key] = oracle.align_pyramid(list(iters), lv, sc.intrinsics, case.R0, case.t0, params=params(oracle, case.overrides))
    return _cache[key]


# ---- what the oracle's trace must show ---------------------------------------------------------------------------------------------
def _steps(ref):
    """(|psi|, theta) of the steps that were applied (the iteration that terminates applies none)"""
    tr = [x for x in ref["trace"] if not x["broke"]]
    return np.array([np.linalg.norm(x["psi"]) for x in tr]), np.array([np.linalg.norm(x["psi"][3:]) for x in tr])


def _radius(case):
    return float(np.float32(case.overrides.get("trust_radius", 0.003)))


def _clamped(case, ref):
    n, _ = _steps(ref)
    return np.abs(n - _radius(case)) <= 1e-12 * _radius(case)


def _all_clamped(oracle, case, ref):
    assert ref["iters_run"] == case.iters and _clamped(case, ref).all()


def _unclamped(oracle, case, ref):
    c = _clamped(case, ref)
    n, _ = _steps(ref)
    assert ref["iters_run"] == case.iters
    assert (~c).sum() >= 6 and c.sum() >= 1, n
    assert np.all(n[~c] < _radius(case) * (1 - 1e-3))


def _terminates(oracle, case, ref):
    full, _ = _steps(reference(oracle, BY_NAME["unclamped"]))
    k = ref["iters_run"]
    assert 2 <= k < case.iters, k
    assert ref["trace"][k - 1]["broke"] and not any(x["broke"] for x in ref["trace"][:k - 1])
    stop = float(np.float32(case.overrides["psi_norm_stop"]))
    assert full[k - 2] > stop > full[k - 1] and full[k - 2] < _radius(case), (full, stop)     # between two consecutive unclamped steps
    assert np.all(ref["energy"][:k] > 0) and np.all(ref["energy"][k:] == 0)


def _theta_above(limit):
    def check(oracle, case, ref):
        _, th = _steps(ref)
        assert ref["iters_run"] == case.iters and np.all(th > limit), th
    return check


def _translation_only(oracle, case, ref):
    n, th = _steps(ref)
    assert ref["iters_run"] == case.iters and np.all(th == 0.0) and np.all(n >= 1e-7)
    assert len(set(ref["energy"].tolist())) > 2


def _changes_energies(oracle, case, ref):
    base = reference(oracle, BY_NAME[case.base])
    assert ref["iters_run"] == base["iters_run"] == case.iters
    assert not np.array_equal(ref["energy"], base["energy"]), (case.name, "changes nothing against", case.base)


def _rotationize_off(oracle, case, ref):
    base = reference(oracle, BY_NAME[case.base])
    assert np.array_equal(ref["energy"], base["energy"]) and ref["best_idx"] == base["best_idx"]
    assert np.abs(ref["R"] - base["R"]).max() < 1e-12 and np.abs(ref["t"] - base["t"]).max() < 1e-12


def quat_branch(R):
    """which branch of quat_of_matrix a matrix takes: -1 for trace > 0, else the index of its largest diagonal entry"""
    if np.trace(R) > 0:
        return -1
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > R[i, i] else i


def _log_general(oracle, case, ref):
    """every iteration takes log(pose) (the regulariser is on) of a pose this far from the identity"""
    assert params(oracle, case.overrides).enable_l2_reg == 1 and ref["iters_run"] == case.iters
    theta = case.start[0]
    for R in [case.R0] + [x["R"] for x in ref["trace"]]:
        w = 0.5 * np.sqrt(max(1 + np.trace(R), 0.0))
        tan2 = (1 - w * w) / (w * w)
        assert not (w > 0.5 and tan2 < 2.5e-3)                       # not the series branch of se3_log_q
        if theta < 1.0:
            assert w > 0.5 and quat_branch(R) == -1                  # general branch behind the first test, |x| <= 1 in d_atan
        else:
            assert np.trace(R) <= 0 and quat_branch(R) == quat_branch(case.R0) and tan2 > 1      # |x| > 1 in d_atan
    if case.carried:
        assert ref["visible_ratio"] >= 0.95, ref["visible_ratio"]
    else:                                                            # the view has turned away: still more than a wave of visible points
        assert ref["visible_ratio"] * len(case.xyz(oracle)) >= 64, ref["visible_ratio"]
    assert len(set(ref["energy"].tolist())) >= 2


CASES = [
    Case("defaults", "every step clamped at the trust radius: what the suite ran before", _all_clamped),
    Case("defaults-L2", "the same at level 2", _all_clamped, level=2),
    Case("unclamped", "pose_apply without the clamp (n2 <= tr2)", _unclamped, UNCLAMPED),
    Case("unclamped-stop", "termination after iteration 0 (s.stop), energies beyond it stay zero", _terminates,
         dict(UNCLAMPED, psi_norm_stop=STOP)),
    Case("radius-0.05", "se3_exp_q, closed forms (theta ~ 2.3e-2)", _theta_above(0.01), dict(trust_radius=0.05)),
    Case("radius-0.05-L2", "the same at level 2", _theta_above(0.01), dict(trust_radius=0.05), level=2),
    Case("radius-1.0", "se3_exp_q, closed forms (theta ~ 0.46)", _theta_above(0.3), dict(trust_radius=1.0)),
    Case("no-rotation", "se3_exp_q, small-angle branch: omega is exactly 0, V = R", _translation_only, dict(precond_rot=0.0)),
    Case("beta-0", "heavy ball off", _changes_energies, dict(beta=0.0), base="defaults"),
    Case("beta-0.9", "heavy ball 0.9", _changes_energies, dict(beta=0.9), base="defaults"),
    Case("lambda-50", "regulariser weight", _changes_energies, dict(UNCLAMPED, reg_lambda=50.0), base="unclamped"),
    Case("decay-2-1", "step decay from iteration 3 on, 1/(itr - 1)", _changes_energies,
         dict(UNCLAMPED, step_decay_after=2, step_decay_offset=1), base="unclamped"),
    Case("step-b-0.02", "step_b enters the step length", _changes_energies, dict(UNCLAMPED, step_b=0.02), base="unclamped"),
    Case("rotationize-off", "enable_rotationize = 0: no effect beyond 1e-12 from a rotation, in any kernel", _rotationize_off,
         dict(enable_rotationize=0), base="defaults"),
]
STARTS = [("0.5", (0.5, (0.3, -0.5, 0.8))), ("2.5x", (2.5, (1, 0, 0))), ("2.5y", (2.5, (0, 1, 0))), ("2.5z", (2.5, (0, 0, 1))),
          ("3.1", (3.1, (0.6, 0.8, 0)))]
# about a coordinate axis two of the quaternion's three vector components are zero, and a kernel that swapped them would pass (tried:
# it did); the same branches again about axes tilted away from x, y and z
TILTED = [("2.5x-tilted", (2.5, (1, 0.2, 0.3))), ("2.5y-tilted", (2.5, (0.2, 1, -0.25))), ("2.5z-tilted", (2.5, (-0.25, 0.2, 1)))]
for _n, _s in STARTS:
    _what = ("se3_log_q, general branch with w > 0.5" if _n == "0.5" else
             "quat_of_matrix, trace <= 0 (pose_state_load) and se3_log_q through d_atan with |x| > 1")
    CASES.append(Case("start-" + _n, _what + "; points in place", _log_general, start=_s))
    CASES.append(Case("start-" + _n + "-carried", _what + "; points carried along", _log_general, start=_s, carried=True))
for _n, _s in TILTED:
    CASES.append(Case("start-" + _n, "quat_of_matrix, trace <= 0, every component of the quaternion in play; points in place", _log_general,
                      start=_s))
CASES.append(Case("start-2.5z-L2", "the same at level 2; points in place", _log_general, start=STARTS[3][1], level=2))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def assert_reaches_branch(oracle, case):
    case.check(oracle, case, reference(oracle, case))


def assert_table(oracle):
    """properties of the table as a whole"""
    far = [BY_NAME["start-2.5" + a] for a in "xyz"]
    assert sorted(quat_branch(c.R0) for c in far) == [0, 1, 2]           # the largest diagonal entry differs between the three
    assert quat_branch(BY_NAME["start-3.1"].R0) >= 0 and quat_branch(BY_NAME["start-0.5"].R0) == -1
    tilted = [BY_NAME["start-" + n] for n, _ in TILTED]
    assert sorted(quat_branch(c.R0) for c in tilted) == [0, 1, 2]
    for c in tilted:                                                     # sin(1.25) * axis: no component near zero
        a = np.asarray(c.start[1], np.float64)
        assert np.all(np.abs(np.sin(1.25) * a / np.linalg.norm(a)) > 0.1)
    assert all(abs(np.linalg.norm(c.t0) - 0.3) < 0.01 for c in CASES if c.start)


def in_place():
    """the cases every path runs (lists the packed kernels accept)"""
    return [c for c in CASES if not c.carried]


def by_key(cases):
    """cases grouped by parameter set, in table order"""
    out = {}
    for c in cases:
        out.setdefault(c.key, []).append(c)
    return out


# ---- the 4-pair batch: one parameter set, four start poses -------------------------------------------------------------------------
# stop = 6e-4: from the identity the run ends after 11 iterations, from the other starts after 12 (no termination), 7 and 9
BATCH_OVERRIDES = dict(UNCLAMPED, psi_norm_stop=6e-4)
BATCH_STARTS = [np.zeros(6), np.array([-0.01, 0.016, 0.002, -0.017, -0.001, -0.012]),
                np.array([-0.006, -0.008, 0.007, 0.016, 0.003, -0.012]), np.array([-0.127, 0.061, -0.12, -0.032, -0.001, -0.045])]


def batch_references(oracle, level=3):
    """per pair (R0, t0, the oracle's run): at least one pair terminates early, at least one runs to the end"""
    if "batch" not in _cache:
        sc, lv = scene(oracle)
        L = lv[level]
        out = []
        for psi in BATCH_STARTS:
            R0, t0 = oracle.se3_exp(psi)
            R0 = np.array(R0)
            out.append((R0, t0, oracle.run_iterations(level, ITERS, L["xyz"], L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], sc.intrinsics,
                                                      R0, t0, params=params(oracle, BATCH_OVERRIDES), trace=True)))
        runs = [r["iters_run"] for _, _, r in out]
        assert any(2 <= k < ITERS for k in runs) and any(k == ITERS and not r["trace"][-1]["broke"] for (_, _, r), k in zip(out, runs)), runs
        _cache["batch"] = out
    return _cache["batch"]


# ---- the tracker: three ticks of one camera under a parameter set ------------------------------------------------------------------
#: the stream of tests/test_gpu_tracker_streams.py (240x320, three levels from full size, 8 iterations each), seed and motion of stream 0
TRACKER = dict(rows=240, cols=320, n_levels=3, first_shift=0, iters=[8, 8, 8], K=(262.5, 262.5, 159.75, 119.75), seeds=(300, 301),
               motions=((0.5, -1.0), (1.0, 0.5)), ticks=3)
TRACKER_SETS = {"unclamped-stop": dict(UNCLAMPED, psi_norm_stop=STOP), "radius-0.05": dict(trust_radius=0.05)}


def tracker_frames(stream):
    import frame_gen
    dy, dx = TRACKER["motions"][stream]
    return [frame_gen.camera_frame(TRACKER["seeds"][stream], TRACKER["rows"], TRACKER["cols"], shift=(int(round(dy * i)), int(round(dx * i))),
                                   holes=True) for i in range(TRACKER["ticks"])]


def tracker_runs(oracle, name):
    """the oracle's traced runs of stream 0: frames 1 and 2 against frame 0, coarse to fine, the pose carried on -- [(frame, level, run)]"""
    key = ("tracker", name)
    if key not in _cache:
        T = TRACKER
        Kf = tuple(np.float32(k) for k in T["K"])
        pyr = [oracle.build_pyramid(b, d, T["n_levels"], T["first_shift"]) for b, d in tracker_frames(0)]
        ref = [oracle.ref_level_from_grey(l, g, d, Kf) for l, (g, d) in enumerate(pyr[0])]
        p = params(oracle, TRACKER_SETS[name])
        R, t = np.eye(3), np.zeros(3)
        out = []
        for now in range(1, T["ticks"]):
            for l in range(T["n_levels"] - 1, -1, -1):
                g = pyr[now][l][0]
                dt, gx, gy, _ = oracle.now_level_from_grey(g)
                r = oracle.run_iterations(l, T["iters"][l], ref[l][0], dt, gx, gy, g.shape[0], g.shape[1], Kf, R, t, params=p, trace=True)
                R, t = r["R"], r["t"]
                out.append((now, l, r))
        _cache[key] = out
    return _cache[key]


def assert_tracker_reaches_branch(oracle, name):
    runs = tracker_runs(oracle, name)
    if name == "unclamped-stop":
        early = [r for _, _, r in runs if 2 <= r["iters_run"] < 8]
        assert early, [r["iters_run"] for _, _, r in runs]
        n = np.concatenate([_steps(r)[0] for _, _, r in runs])
        assert np.count_nonzero(n < 0.003 * (1 - 1e-3)) >= 3 and np.count_nonzero(n > 0.003 * (1 - 1e-9)) >= 3      # both sides of the clamp
    else:
        assert all(r["iters_run"] == 8 and np.all(_steps(r)[1] > 0.01) for _, _, r in runs)
