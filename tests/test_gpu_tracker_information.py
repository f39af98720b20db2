"""Pose information of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_information / dvo_tracker_get_information): with
every pose a step returns, H = sum w J J^T, g = J^T W eps, sum eps^2 and the visible count at that pose on the finest level that ran,
from one extra launch per step (dvo_tracker_info.hip) and no extra host synchronisation.

Expected values: the CPU oracle's accumulators (oracle_lib.accumulate) on the reference points and the now level the tracker's context
holds AFTER the step (dvo_get_ref_level / dvo_get_now_level of dvo_tracker_context), the stream's own intrinsics and the pose the step
returned.  H and g are double sums of exact products: only the order of the additions differs, hence the project's tolerance for
them (tests/test_gpu_parity.py::test_normal_matrix_of_every_iterate: rtol 1e-12, atol 1e-12 max|want|); sum_eps2 (the correctly
rounded exact sum), n_visible and level must be equal."""
import ctypes

import numpy as np
import pytest

import frame_gen
import frame_reference as fr

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 240, 320, 3, 0                 # the geometry of tests/test_gpu_tracker_streams.py
ITERS = [8, 8, 8]
K = (262.5, 262.5, 159.75, 119.75)
ENGINE = dict(block_threads=512, team_size=1)          # one launch shape in every arrangement (tests/test_gpu_tracker_streams.py)
MOTIONS = [(0.5, -1.0), (1.0, 0.5), (-0.5, 1.5), (1.5, -0.5), (0.0, 1.4)]
N_S, N_T = 5, 7                                        # key_frame_every = 5: tick 5 is the forced switch and its re-run
FIELDS = ("H", "g", "sum_eps2", "n_visible", "level")


def sequence(seed, n, motion):
    dy, dx = motion
    return [frame_gen.camera_frame(seed, ROWS, COLS, shift=(int(round(dy * i)), int(round(dx * i))), holes=True) for i in range(n)]


def make_tracker(n, iters=ITERS, adaptive=None, information=True, **engine):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in dict(ENGINE, **engine).items():
        setattr(p, k, v)
    a = adaptive or {}
    tr = DvoTracker(n, params=p, iters=iters, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, adaptive=adaptive is not None,
                    laplacian_b_thresh=a.get("laplacian_b", 3.0), visible_ratio_thresh=a.get("visible_ratio", 0.8),
                    min_points=a.get("min_points", 50))
    tr.set_intrinsics(*K)
    if information:
        tr.set_information(True)
    return tr


def level_dims(level, rows=ROWS, cols=COLS, shift=SHIFT):
    return fr.level_size(rows, shift + level), fr.level_size(cols, shift + level)


def resident(tr, stream, level, rows=ROWS, cols=COLS, shift=SHIFT):
    """reference points and now level of `stream` as the tracker's context holds them; rows, cols, shift: the tracker's geometry"""
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    n = ctypes.c_int()
    assert lib.dvo_get_ref_level(h, stream, level, None, 0, ctypes.byref(n)) == 0
    xyz = np.zeros(3 * n.value, np.float32)
    assert lib.dvo_get_ref_level(h, stream, level, capi._ptr(xyz), n.value, ctypes.byref(n)) == 0
    rows, cols = level_dims(level, rows, cols, shift)
    dt, gx, gy = (np.zeros(rows * cols, np.float32) for _ in range(3))
    assert lib.dvo_get_now_level(h, stream, level, capi._ptr(dt), capi._ptr(gx), capi._ptr(gy)) == 0
    return xyz.reshape(-1, 3), dt, gx, gy


def check_against_oracle(oracle, tr, stream, level, Ks, R, t, rec, what):
    xyz, dt, gx, gy = resident(tr, stream, level)
    rows, cols = level_dims(level)
    want = oracle.accumulate(level, xyz, 0, len(xyz), dt, gx, gy, rows, cols, Ks, R, t)
    H = np.zeros((6, 6)); k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = want[k]; k += 1
    g = want[21:27]
    print(what, "N", len(xyz), "visible", rec["n_visible"], int(want[28]), "sum_eps2", rec["sum_eps2"], want[27],
          "max rel dH %.3g" % (np.abs(rec["H"] - H).max() / np.abs(H).max()), "max rel dg %.3g" % (np.abs(rec["g"] - g).max() / np.abs(g).max()))
    assert rec["level"] == level, what
    assert rec["n_visible"] == int(want[28]) and rec["n_visible"] > 6, what
    assert rec["sum_eps2"] == want[27], (what, rec["sum_eps2"], want[27])
    np.testing.assert_allclose(rec["H"], H, rtol=1e-12, atol=1e-12 * np.abs(H).max(), err_msg=str(what))
    np.testing.assert_allclose(rec["g"], g, rtol=1e-12, atol=1e-12 * np.abs(g).max(), err_msg=str(what))


def assert_zero_record(rec, what):
    assert rec["level"] == -1 and rec["n_visible"] == 0 and rec["sum_eps2"] == 0.0, (what, rec)
    assert not rec["H"].any() and not rec["g"].any(), (what, rec)


def same_record(a, b):
    return all(np.array_equal(a[k], b[k]) for k in FIELDS)


def run(tr, seqs, schedule, oracle=None, level=0, Ks=None):
    """schedule: per tick [(stream, frame index)].  Per tick: dict(R, t, ev, stats, rec={stream: record}, sig={stream: signals});
    with an oracle every record is checked against it right after its step"""
    ticks = []
    for n, entry in enumerate(schedule):
        streams = [s for s, _ in entry]
        R, t, ev = tr.step(streams, [seqs[s][i][0] for s, i in entry], [seqs[s][i][1] for s, i in entry])
        out = dict(R=R, t=t, ev=ev.copy(), stats=tr.stats(), rec={}, sig={})
        for k, s in enumerate(streams):
            if tr.information_on:
                out["rec"][s] = tr.information(s)
                if ev[k] == 1:
                    assert_zero_record(out["rec"][s], (n, s))
                elif oracle is not None:
                    check_against_oracle(oracle, tr, s, level, (Ks or {}).get(s, K), R[k], t[k], out["rec"][s], ("tick", n, "stream", s, "event", int(ev[k])))
            if ev[k] != 1:
                out["sig"][s] = tr.signals(s)
        ticks.append(out)
    return ticks


def tracked(n, information=True, **kw):
    tr = make_tracker(n, information=information, **kw)
    tr.information_on = information
    return tr


FULL = [[(s, n) for s in range(N_S)] for n in range(N_T)]


@pytest.fixture(scope="module")
def seqs():
    return [sequence(900 + s, N_T, MOTIONS[s]) for s in range(N_S)]


@pytest.fixture(scope="module")
def on_run(seqs):
    """five streams, seven ticks, information on; nothing but the steps touches the context"""
    with tracked(N_S) as tr:
        return run(tr, seqs, FULL)


def test_parity_on_every_tick_and_stream(seqs, oracle, on_run):
    with tracked(N_S) as tr:
        ticks = run(tr, seqs, FULL, oracle=oracle)
    assert [x["ev"].tolist() for x in ticks] == [[1] * N_S] + [[0] * N_S] * 4 + [[5] * N_S] + [[0] * N_S]
    assert ticks[5]["stats"]["key_frames"] == N_S           # the records of tick 5 are the re-run's, against the new reference
    # reading the resident levels between the steps changed nothing
    for a, b in zip(ticks, on_run):
        assert all(same_record(a["rec"][s], b["rec"][s]) for s in range(N_S))


@pytest.mark.parametrize("iters,level", [([0, 0, 8], 2), ([0, 8, 8], 1)])
def test_coarse_finest_level(seqs, oracle, iters, level):
    """the record is taken on the finest level that RAN: 60 x 80 (a few hundred points, not a multiple of 64) or 120 x 160"""
    with tracked(2, iters=iters) as tr:
        ticks = run(tr, seqs, [[(0, n), (1, n)] for n in range(3)], oracle=oracle, level=level)
        n_pts = [len(resident(tr, s, level)[0]) for s in (0, 1)]
    assert all(r["level"] == level for x in ticks[1:] for r in x["rec"].values())
    if level == 2:
        assert all(64 < n < 2048 for n in n_pts) and any(n % 64 for n in n_pts), n_pts


def test_mixed_rig(seqs, oracle):
    """streams with their own intrinsics and undistortion in one handle -- the context DVO_FLAG_NORMAL_MATRIX refuses -- each against
    the oracle with ITS camera model"""
    Ks = {0: (250.0, 254.0, 161.0, 118.0), 1: (275.0, 271.5, 157.5, 121.25)}
    D = np.array((-0.08, 0.03, 0.001, -0.0005, 0.0))
    with tracked(3) as tr:
        for s, k in Ks.items():
            tr.set_stream_intrinsics(s, *k)
        tr.set_stream_undistort(1, np.array(Ks[1], np.float64), D)
        ticks = run(tr, seqs, [[(s, n) for s in range(3)] for n in range(N_T)], oracle=oracle, Ks=Ks)
    assert ticks[5]["ev"].tolist() == [5, 5, 5]


def test_record_depends_on_the_stream_alone(seqs, on_run):
    """bit for bit: stream 3 of the five-stream tracker, the same frames as the only stream of a one-stream tracker, and as stream 3 of
    steps that list [3, 1] only"""
    with tracked(1) as tr:
        alone = run(tr, [seqs[3]], [[(0, n)] for n in range(N_T)])
    with tracked(N_S) as tr:
        pair = run(tr, seqs, [[(3, n), (1, n)] for n in range(N_T)])
    for n in range(N_T):
        a, b, c = on_run[n]["rec"][3], alone[n]["rec"][0], pair[n]["rec"][3]
        assert same_record(a, b) and same_record(a, c), (n, a, b, c)
        assert on_run[n]["ev"][3] == alone[n]["ev"][0] == pair[n]["ev"][0]
    assert on_run[5]["ev"][3] == 5 and on_run[5]["rec"][3]["n_visible"] > 6


def test_nothing_else_moves(seqs, on_run):
    """information on against off: the same poses, events and signals, the same host synchronisations, one launch more per step (two
    on a step with key-frame switches)"""
    with tracked(N_S, information=False) as tr:
        off = run(tr, seqs, FULL)
    for n, (a, b) in enumerate(zip(on_run, off)):
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"], n
        assert a["stats"]["syncs"] == b["stats"]["syncs"], (n, a["stats"], b["stats"])
        extra = 0 if n == 0 else (2 if b["stats"]["key_frames"] else 1)      # tick 0: first frames only, nothing was aligned
        assert a["stats"]["launches"] == b["stats"]["launches"] + extra, (n, a["stats"], b["stats"])
        assert {k: v for k, v in a["stats"].items() if k != "launches"} == {k: v for k, v in b["stats"].items() if k != "launches"}, n
    assert [x["stats"]["key_frames"] for x in off] == [0, 0, 0, 0, 0, N_S, 0]
    assert [x["stats"]["syncs"] for x in off][1:5] == [1, 1, 1, 1]


def test_adaptive_mode(seqs, oracle):
    """the adaptive exits (finalEpsilons ride on the first alignment): parity holds, the signals are what they are without information"""
    adaptive = dict(laplacian_b=3.0, visible_ratio=0.97, min_points=50)
    sched = [[(s, n) for s in range(3)] for n in range(N_T)]
    with tracked(3, adaptive=adaptive) as tr:
        on = run(tr, seqs, sched, oracle=oracle)
    with tracked(3, adaptive=adaptive, information=False) as tr:
        off = run(tr, seqs, sched)
    print("adaptive events", [x["ev"].tolist() for x in on])
    for n, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"] and (n == 0 or len(a["sig"]) == 3), n
        assert a["stats"]["syncs"] == b["stats"]["syncs"], n


def test_sensor_formats(seqs):
    """mono8 images + 16-bit depth through dvo_tracker_step_fmt give the records of the BGR8 / float frames they stand for"""
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    streams = [0, 1, 2]
    with tracked(3) as new, tracked(3) as old:
        for n in range(N_T):
            grey = [fr.bgr2gray(seqs[s][n][0]) for s in streams]
            d16 = [np.clip(np.nan_to_num(np.rint(seqs[s][n][1] * 1000.0), nan=0.0), 0, 65535).astype(np.uint16) for s in streams]
            got = new.step(streams, grey, d16)
            want = old.step(streams, [np.repeat(g[..., None], 3, 2) for g in grey],
                            [np.where(d == 0, 1, d).astype(np.float32) for d in d16], flags=DVO_UPLOAD_DEPTH_RAW)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), n
            for s in streams:
                assert same_record(new.information(s), old.information(s)), (n, s)
            assert new.information(0)["level"] == (-1 if n == 0 else 0)
        assert want[2].tolist() == [0, 0, 0] and new.stats() == old.stats()


def test_contract(seqs):
    from rgbd_odometry_amd import DvoError
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE

    def refused(code, fn, *a):
        with pytest.raises(DvoError) as ei:
            fn(*a)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    with tracked(2, information=False) as tr:
        step = lambda n, streams=(0, 1): tr.step(list(streams), [seqs[s][n][0] for s in streams], [seqs[s][n][1] for s in streams])
        step(0)
        refused(DVO_ERR_STATE, tr.information, 0)                 # off
        tr.set_information(True)
        refused(DVO_ERR_STATE, tr.information, 0)                 # on, not stepped since
        refused(DVO_ERR_INVALID, tr.information, 2)
        refused(DVO_ERR_INVALID, tr.information, -1)
        step(1)
        rec = tr.information(0)
        assert rec["level"] == 0 and rec["n_visible"] > 6
        H = rec["H"]
        assert np.array_equal(H, H.T) and np.all(np.linalg.eigvalsh(H) > -1e-9 * np.abs(H).max())      # positive semi-definite
        C = tr.covariance(0)
        assert C is not None and np.all(np.isfinite(C)) and np.allclose(C, C.T, rtol=1e-9, atol=0) and np.all(np.diag(C) > 0)
        tr.reset_stream(1)
        refused(DVO_ERR_STATE, tr.information, 1)                 # reset: nothing until its next step
        assert tr.information(0)["n_visible"] == rec["n_visible"]
        step(2, streams=(1,))                                      # stream 1 starts over: the zero record, no covariance
        assert_zero_record(tr.information(1), "after reset")
        assert tr.covariance(1) is None
        tr.set_information(False)
        refused(DVO_ERR_STATE, tr.information, 0)
    for kw in (dict(interpolate_dt=1), dict(engine_variant=1)):
        with tracked(1, information=False, **kw) as tr:
            refused(DVO_ERR_INVALID, tr.set_information, True)
            refused(DVO_ERR_STATE, tr.information, 0)             # nothing changed: still off
            tr.set_information(False)
