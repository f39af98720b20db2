"""The pose update's parameters and the branches the default parameters never reach (tests/update_cases.py), inside every alignment
kernel, against the CPU oracle run with the same parameters.

Each call form of the update builds and reads its UpdConst block in its own way: the packed fused kernel (solo at 512 and 256
threads, and as a team), the one-point-per-lane kernel, the host-driven dvo_iter_* calls, the wide / tiled step, a batch launch and
the tracker.  One context per path and parameter set, the cases looped inside it; the oracle's runs are computed once and shared.
Every case first asserts on the oracle's trace that it reaches its branch.

Comparison as in tests/test_gpu_parity.py: energies (including the zeros beyond an early termination), best index and visible ratio
equal, finalEpsilons / finalReprojections bit-equal where the path delivers them, the pose within ROT_TOL / TRANS_TOL.

Start poses beyond 0.1 rad with the points carried along are foreign lists to the engine (no enlistRefEdgePts list): they run on the
one-point-per-lane kernels only; the same start poses with the points in place run everywhere.
"""
import numpy as np
import pytest

import update_cases as uc
from oracle_lib import rot_angle
from test_gpu_parity import ROT_TOL, TRANS_TOL

pytestmark = pytest.mark.gpu

PYRAMID = [0, 0, uc.ITERS, uc.ITERS]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _context(oracle, overrides, n_pairs=1, **engine):
    """a context with the parameter set and the scene's four levels resident for every pair"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = uc.scene(oracle)
    ctx = DvoContext(n_pairs, **engine, **dict(overrides))
    ctx.set_intrinsics(*sc.intrinsics)
    for p in range(n_pairs):
        for l, L in enumerate(lv):
            ctx.set_ref_level(l, L["xyz"], pair=p)
            ctx.set_now_level(l, L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], pair=p)
    return ctx


def _set_points(ctx, oracle, case, state, levels):
    """the case's reference lists (carried lists differ from case to case; the scene's own are put back after them)"""
    want = case.name if case.carried else None
    if state.get("points") != want:
        for l in levels:
            ctx.set_ref_level(l, case.xyz(oracle, l))
        state["points"] = want


def _check(case, ref, got, what, final=True):
    assert _same(got["energy"], ref["energy"]), (case.name, what, got["energy"], ref["energy"])
    assert got["best_idx"] == ref["best_idx"] and got["visible_ratio"] == ref["visible_ratio"], (case.name, what)
    if final:
        assert _same(got["final_eps"], ref["final_eps"]) and _same(got["final_reproj"], ref["final_reproj"]), (case.name, what)
    assert rot_angle(ref["R"], got["R"]) <= ROT_TOL and np.linalg.norm(ref["t"] - got["t"]) <= TRANS_TOL, \
        (case.name, what, rot_angle(ref["R"], got["R"]), np.linalg.norm(ref["t"] - got["t"]))


def _run_fused(oracle, cases, shape_check, **engine):
    for key, group in uc.by_key(cases).items():
        with _context(oracle, key, **engine) as ctx:
            state = {}
            for case in group:
                uc.assert_reaches_branch(oracle, case)
                _set_points(ctx, oracle, case, state, [case.level])
                got = ctx.run_iterations(case.level, case.iters, case.R0, case.t0)
                shape_check(case, ctx.last_launch_shape())
                _check(case, uc.reference(oracle, case), got, engine)


@pytest.mark.parametrize("block", [512, 256])
def test_packed_kernel_one_workgroup(oracle, block):
    def shape(case, s):
        assert s[2] and s[0] == block and s[1] == 1, (case.name, s)
    uc.assert_table(oracle)
    _run_fused(oracle, uc.in_place(), shape, team_size=1, block_threads=block)


def test_packed_kernel_team(oracle):
    """a team of two workgroups shares the pair: both members must take the same branches, stop in the same iteration"""
    def shape(case, s):
        assert s[2] and s[1] > 1, (case.name, s)
    _run_fused(oracle, [uc.BY_NAME[n] for n in ("unclamped-stop", "radius-0.05", "start-2.5x-tilted")], shape, team_size=2)


def test_one_point_per_lane_kernel(oracle):
    def shape(case, s):
        assert not s[2], (case.name, s)
    _run_fused(oracle, uc.CASES, shape, engine_variant=1)


def test_host_driven_iterations(oracle):
    """dvo_iter_begin / _accumulate / _update / _end: the update of every iteration is a launch of its own, and the caller goes on
    calling after the level has terminated"""
    import torch
    from rgbd_odometry_amd.distributed import HipTiledEngine
    for key, group in uc.by_key(uc.CASES).items():
        with _context(oracle, key) as ctx:
            eng = HipTiledEngine(ctx)
            acc = eng.new_acc()
            state = {}
            for case in group:
                uc.assert_reaches_branch(oracle, case)
                _set_points(ctx, oracle, case, state, [case.level])
                n = eng.n_points(case.level)
                eng.iter_begin(case.level, case.iters, case.R0, case.t0)
                for itr in range(case.iters):
                    eng.iter_accumulate(case.level, 0, n, acc.data_ptr())
                    eng.iter_update(case.level, itr, n, acc.data_ptr())
                got = eng.iter_end(case.level)
                torch.cuda.synchronize()
                _check(case, uc.reference(oracle, case), got, "host-driven", final=False)


def test_wide_schedule_levels_3_to_2(oracle):
    """dvo_align_pyramid_wide over levels 3 -> 2: the state (and its UpdConst block) travels through HBM between the launches; in the
    termination case level 3 stops early and level 2 still runs"""
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    early = uc.pyramid_reference(oracle, uc.BY_NAME["unclamped-stop"], PYRAMID)
    assert 2 <= early["levels"][3]["iters_run"] < uc.ITERS and early["levels"][2]["iters_run"] >= 2
    cases = [c for c in uc.CASES if c.level == 3]
    for key, group in uc.by_key(cases).items():
        with _context(oracle, key) as ctx:
            state = {}
            for case in group:
                uc.assert_reaches_branch(oracle, case)
                _set_points(ctx, oracle, case, state, [2, 3])
                ref = uc.pyramid_reference(oracle, case, PYRAMID)
                R, t = ctx.align_pyramid_wide(PYRAMID, case.R0, case.t0, flags=DVO_FLAG_FINAL_OUTPUTS)
                for l in (3, 2):
                    rep = ref["levels"][l]
                    e, b, ratio = ctx.level_report(0, l, PYRAMID[l])
                    assert _same(e, rep["energy"]) and b == rep["best_idx"] and ratio == rep["visible_ratio"], (case.name, "wide", l, e, rep["energy"])
                fe, fr = ctx.final_outputs(0, ctx.n_points(2))
                assert _same(fe, ref["levels"][2]["final_eps"]) and _same(fr, ref["levels"][2]["final_reproj"]), (case.name, "wide")
                assert rot_angle(ref["R"], R) <= ROT_TOL and np.linalg.norm(ref["t"] - t) <= TRANS_TOL, (case.name, "wide")


def test_batch_of_four_start_poses(oracle):
    """one launch, one parameter set, four start poses: some pairs terminate early, one runs to the end; each its own oracle's report"""
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    refs = uc.batch_references(oracle)
    iters = [0, 0, 0, uc.ITERS]
    for engine in (dict(), dict(team_size=1, block_threads=256), dict(engine_variant=1)):
        with _context(oracle, uc.BATCH_OVERRIDES, n_pairs=4, **engine) as ctx:
            R, t = ctx.align_batch(iters, np.array([r[0] for r in refs]), np.array([r[1] for r in refs]), flags=DVO_FLAG_FINAL_OUTPUTS)
            for p, (_, _, ref) in enumerate(refs):
                e, b, ratio = ctx.level_report(p, 3, uc.ITERS)
                fe, fr = ctx.final_outputs(p, ctx.n_points(3, p))
                _check(uc.BY_NAME["unclamped-stop"], ref, dict(energy=e, best_idx=b, visible_ratio=ratio, final_eps=fe, final_reproj=fr,
                                                               R=R[p], t=t[p]), ("batch", engine, p))


@pytest.mark.parametrize("name", sorted(uc.TRACKER_SETS))
def test_tracker_three_ticks(oracle, name):
    """DvoTracker(max_streams=2, params=p): three ticks of two cameras == the single-stream sequence of engine calls under the same
    parameters (tests/test_gpu_tracker_streams.py), bit for bit"""
    import test_gpu_tracker_streams as ts
    T = uc.TRACKER
    assert (ts.ROWS, ts.COLS, ts.NL, ts.SHIFT, ts.ITERS, ts.K) == (T["rows"], T["cols"], T["n_levels"], T["first_shift"], T["iters"], T["K"])
    uc.assert_tracker_reaches_branch(oracle, name)
    ov = uc.TRACKER_SETS[name]
    seqs = [uc.tracker_frames(s) for s in range(2)]
    want = [ts.single_stream(q, params=ov) for q in seqs]
    with ts.make_tracker(2, params=ov) as tr:
        got = ts.run_tracker(tr, seqs, [[(s, n) for s in range(2)] for n in range(T["ticks"])])
    for s in range(2):
        ts.assert_same(got[s], want[s], "stream %d" % s)
    plain = ts.single_stream(seqs[0])
    assert not all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(plain, want[0])), "the parameters changed nothing"
