"""Per-stream camera calibration of the multi-stream trackers (include/dvo_amd.h: dvo_tracker_set_stream_intrinsics / _undistort /
clear_stream_camera, dvo_photo_streams_set_stream_intrinsics).  A rig whose streams carry different intrinsics and distortion must give,
for every stream, exactly what the single-stream path gives on that stream's frames with that stream's calibration -- in one handle,
with the launch and synchronisation counts of a uniform rig."""
import signal
from contextlib import contextmanager

import numpy as np
import pytest

import frame_gen

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 240, 320, 3, 0
ITERS = [8, 8, 8]
K_WIDE = (262.5, 262.5, 159.75, 119.75)
# three camera models; two distortions, each shared by two streams (the streams without one take their frames as they are)
KS = [K_WIDE, (250.0, 254.0, 161.0, 118.0), (275.0, 271.5, 157.5, 121.25)]
DIST = [(-0.08, 0.03, 0.001, -0.0005, 0.0), (0.05, -0.02, -0.0008, 0.0012, 0.004)]
# stream -> (intrinsics index, distortion index or None)
RIG = [(0, None), (1, 0), (2, 1), (1, 0), (2, 1), (0, None)]
# one launch shape on both sides (see tests/test_gpu_tracker_streams.py)
ENGINE = dict(block_threads=512, team_size=1)
MOTIONS = [(0.5, -1.0), (1.0, 0.5), (-0.5, 1.5), (1.5, -0.5), (0.0, 1.4), (-1.0, -1.0)]


@contextmanager
def time_limit(seconds):
    def boom(*_):
        raise TimeoutError("test case exceeded %d s" % seconds)
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def sequence(seed, n, motion):
    dy, dx = motion
    return [frame_gen.camera_frame(seed, ROWS, COLS, shift=(int(round(dy * i)), int(round(dx * i))), holes=True) for i in range(n)]


def k4(K):
    return np.array(K, np.float64)


def single_stream(frames, K=K_WIDE, dist=None, every=5, engine=ENGINE):
    """the engine calls of dvo_amd::SolveDVO::processFirstFrame / processFrame for one camera with its own set_intrinsics and
    frames_set_undistort: [(R, t, event, None)] per frame"""
    from rgbd_odometry_amd import DvoContext
    out = []
    with DvoContext(1, **engine) as ctx:
        ctx.set_intrinsics(*K)
        if dist is not None:
            ctx.frames_set_undistort(ROWS, COLS, k4(K), np.array(dist, np.float64))
        cR, cT = np.eye(3), np.zeros(3)
        last_ref = 0
        ref_slot = now_slot = prev_slot = -1
        for n, (bgr, depth) in enumerate(frames):
            slot = next(x for x in range(4) if x not in (ref_slot, now_slot, prev_slot))      # SolveDVO::freeSlot
            ctx.frames_upload_cameras([bgr], [depth], n_levels=NL, first_shift=SHIFT, first_slot=slot)
            if n == 0:
                ref_slot = slot
                ctx.frames_as_ref(slot, 0, 1)
                cR, cT = np.eye(3), np.zeros(3)
                out.append((cR.copy(), cT.copy(), 1, None))
                continue
            if now_slot >= 0:
                prev_slot = now_slot
            now_slot = slot
            ctx.frames_as_now(slot, 0, 1)
            R, t = ctx.align_batch(ITERS, cR[None].copy(), cT[None].copy())
            cR, cT = R[0], t[0]
            event = 0
            if n - last_ref == every and last_ref != n - 1:
                last_ref = n - 1
                ref_slot = prev_slot
                ctx.frames_as_ref(prev_slot, 0, 1)
                R, t = ctx.align_batch(ITERS, np.eye(3)[None], np.zeros((1, 3)))
                cR, cT = R[0], t[0]
                event = 5
            out.append((cR.copy(), cT.copy(), event, None))
    return out


def make_tracker(n, engine=ENGINE):
    import ctypes
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in engine.items():
        setattr(p, k, v)
    tr = DvoTracker(n, params=p, iters=ITERS, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT)
    tr.set_intrinsics(*K_WIDE)
    return tr


def calibrate(tr, rig=RIG):
    for s, (ki, di) in enumerate(rig):
        tr.set_stream_intrinsics(s, *KS[ki])
        if di is not None:
            tr.set_stream_undistort(s, k4(KS[ki]), np.array(DIST[di], np.float64))


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for n, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (what, n, "event", g[2], w[2])
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (what, n, "pose", g[0], w[0], g[1], w[1])


def run_schedule(tr, seqs, schedule, resets=()):
    """schedule: per tick [(stream, frame index)]; resets: {tick: [streams]} reset before that tick.  Returns per stream the outputs
    and the per-tick stats"""
    got, stats = {s: [] for s in range(len(seqs))}, []
    for tick, entry in enumerate(schedule):
        for s in dict(resets).get(tick, []):
            tr.reset_stream(s)
        streams = [s for s, _ in entry]
        R, t, ev = tr.step(streams, [seqs[s][i][0] for s, i in entry], [seqs[s][i][1] for s, i in entry])
        stats.append(tr.stats())
        for k, s in enumerate(streams):
            got[s].append((R[k], t[k], int(ev[k]), None))
    return got, stats


def mixed_schedule(n_s, n_t):
    """stream 5 joins late (tick 3), stream 3 skips tick 4, stream 2 is reset before tick 7; returns the schedule, the resets and per
    stream the list of frames it received, split at its reset"""
    pos, schedule, parts = [0] * n_s, [], [[[]] for _ in range(n_s)]
    resets = {7: [2]}
    for tick in range(n_t):
        if tick in resets:
            for s in resets[tick]:
                parts[s].append([])
        live = [s for s in range(n_s) if not (s == 5 and tick < 3) and not (s == 3 and tick == 4)]
        entry = []
        for s in live:
            entry.append((s, pos[s]))
            parts[s][-1].append(pos[s])
            pos[s] += 1
        schedule.append(entry)
    return schedule, resets, parts


@pytest.mark.parametrize("interp", [0, 1])
def test_mixed_rig_bit_identical_to_single_stream(interp):
    """6 streams, 3 intrinsics, 2 distortions shared by two streams each; a key-frame switch, a late join, a skip and a reset"""
    with time_limit(900):
        engine = dict(ENGINE, interpolate_dt=interp)
        n_s, n_t = 6, 12
        seqs = [sequence(400 + s, n_t, MOTIONS[s]) for s in range(n_s)]
        schedule, resets, parts = mixed_schedule(n_s, n_t)
        with make_tracker(n_s, engine) as tr:
            calibrate(tr)
            got, _ = run_schedule(tr, seqs, schedule, resets)
        for s in range(n_s):
            ki, di = RIG[s]
            want = []
            for part in parts[s]:
                want += single_stream([seqs[s][i] for i in part], K=KS[ki], dist=None if di is None else DIST[di], engine=engine)
            assert_same(got[s], want, "stream %d" % s)
            assert any(w[2] == 5 for w in want), s                 # a key-frame switch ran on every stream
        assert got[2][7][2] == 1 and got[5][0][2] == 1


def test_per_stream_setters_with_handle_values_match_handle_wide():
    with time_limit(600):
        n_s, n_t = 4, 7
        seqs = [sequence(500 + s, n_t, MOTIONS[s]) for s in range(n_s)]
        sched = [[(s, n) for s in range(n_s)] for n in range(n_t)]
        D = np.array(DIST[0], np.float64)
        from rgbd_odometry_amd import capi
        with make_tracker(n_s) as tr:                     # the handle-wide map: dvo_frames_set_undistort on the tracker's context
            K = k4(K_WIDE)
            assert capi.load_library().dvo_frames_set_undistort(tr.context_handle(), ROWS, COLS, capi._ptr(K), capi._ptr(D)) == 0
            want, wst = run_schedule(tr, seqs, sched)
        with make_tracker(n_s) as tr:
            for s in range(n_s):
                tr.set_stream_intrinsics(s, *K_WIDE)
                tr.set_stream_undistort(s, k4(K_WIDE), D)
            got, gst = run_schedule(tr, seqs, sched)
        for s in range(n_s):
            assert_same(got[s], want[s], "stream %d" % s)
        assert gst == wst


def test_launch_counts_of_a_mixed_rig_equal_a_uniform_rig():
    with time_limit(600):
        n_s, n_t = 6, 7
        seqs = [sequence(600 + s, n_t, MOTIONS[s]) for s in range(n_s)]
        sched = [[(s, n) for s in range(n_s)] for n in range(n_t)]
        with make_tracker(n_s) as tr:
            _, uniform = run_schedule(tr, seqs, sched)
        with make_tracker(n_s) as tr:
            calibrate(tr)
            _, mixed = run_schedule(tr, seqs, sched)
        for u, m in zip(uniform, mixed):
            for k in ("launches", "syncs", "runs", "key_frames"):
                assert u[k] == m[k], (k, u, m)


def test_start_of_stream_rule():
    from rgbd_odometry_amd import DvoError
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    with time_limit(600):
        n_s, n_t = 2, 6
        seqs = [sequence(700 + s, n_t, MOTIONS[s]) for s in range(n_s)]
        with make_tracker(n_s) as tr:
            a, _ = run_schedule(tr, seqs, [[(s, n) for s in range(n_s)] for n in range(3)])
            for call in (lambda: tr.set_stream_intrinsics(1, *KS[1]), lambda: tr.set_stream_undistort(1, k4(KS[1]), np.array(DIST[0])),
                         lambda: tr.set_stream_undistort(1, None, None), lambda: tr.clear_stream_camera(1)):
                with pytest.raises(DvoError) as e:
                    call()
                assert e.value.code == DVO_ERR_STATE
            b, _ = run_schedule(tr, seqs, [[(s, n) for s in range(n_s)] for n in range(3, n_t)])
            tr.reset_stream(1)
            tr.set_stream_intrinsics(1, *KS[1])
            tr.set_stream_undistort(1, k4(KS[1]), np.array(DIST[0]))
            c, _ = run_schedule(tr, seqs, [[(1, n)] for n in range(n_t)])
        for s in range(n_s):
            assert_same(a[s] + b[s], single_stream(seqs[s]), "stream %d (refused calls change nothing)" % s)
        assert_same(c[1], single_stream(seqs[1], K=KS[1], dist=DIST[0]), "stream 1 after reset")


def test_refusals_change_nothing():
    from rgbd_odometry_amd import DvoError
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    with time_limit(600):
        n_s, n_t = 3, 6
        seqs = [sequence(800 + s, n_t, MOTIONS[s]) for s in range(n_s)]
        sched = [[(s, n) for s in range(n_s)] for n in range(n_t)]
        D = np.array(DIST[1], np.float64)
        with make_tracker(n_s) as tr:
            calibrate(tr, RIG[:n_s])
            bad = [lambda: tr.set_stream_intrinsics(n_s, *KS[1]), lambda: tr.set_stream_intrinsics(-1, *KS[1]),
                   lambda: tr.set_stream_intrinsics(0, 0.0, 250.0, 160.0, 120.0), lambda: tr.set_stream_intrinsics(1, 250.0, -1.0, 160.0, 120.0),
                   lambda: tr.set_stream_undistort(0, k4(KS[0]), None), lambda: tr.set_stream_undistort(0, None, D),
                   lambda: tr.set_stream_undistort(n_s, k4(KS[0]), D), lambda: tr.set_stream_undistort(2, (0.0, 250.0, 160.0, 120.0), D),
                   lambda: tr.clear_stream_camera(n_s)]
            for call in bad:
                with pytest.raises(DvoError) as e:
                    call()
                assert e.value.code == DVO_ERR_INVALID
            got, _ = run_schedule(tr, seqs, sched)
        for s in range(n_s):
            ki, di = RIG[s]
            assert_same(got[s], single_stream(seqs[s], K=KS[ki], dist=None if di is None else DIST[di]), "stream %d" % s)


def test_cleared_stream_follows_the_handle_again():
    with time_limit(600):
        n_s, n_t = 2, 6
        seqs = [sequence(850 + s, n_t, MOTIONS[s]) for s in range(n_s)]
        with make_tracker(n_s) as tr:
            calibrate(tr, RIG[:n_s])
            tr.clear_stream_camera(1)
            got, _ = run_schedule(tr, seqs, [[(s, n) for s in range(n_s)] for n in range(n_t)])
        assert_same(got[1], single_stream(seqs[1]), "stream 1")
        assert_same(got[0], single_stream(seqs[0], K=KS[RIG[0][0]]), "stream 0")


def test_wrong_k_guard():
    """the per-stream K reaches the kernels (the reference extraction, the packed kernel's compact-point expansion): a stream whose K
    differs from the handle's does not track like the handle's K"""
    with time_limit(600):
        n_t = 6
        seqs = [sequence(900, n_t, MOTIONS[1])] * 2
        with make_tracker(2) as tr:
            tr.set_stream_intrinsics(1, *KS[2])
            got, _ = run_schedule(tr, seqs, [[(0, n), (1, n)] for n in range(n_t)])
        assert_same(got[0], single_stream(seqs[0]), "stream 0")
        assert_same(got[1], single_stream(seqs[1], K=KS[2]), "stream 1")
        assert any(not np.array_equal(a[1], b[1]) for a, b in zip(got[0][1:], got[1][1:]))


# ---- photometric streams ------------------------------------------------------------------------------------------------------
K640 = (525.0, 525.0, 319.5, 239.5)
K640_B = (540.0, 531.5, 322.0, 236.5)
LEVELS = (3, 2)


def camera(seed, rows=480, cols=640, shift=(0, 0)):
    bgr, depth_m = frame_gen.camera_frame(seed, rows, cols, shift=shift)
    d = np.nan_to_num(np.round(depth_m * 1000.0), nan=0.0, posinf=65535, neginf=0)
    return bgr, np.clip(d, 1, 65535).astype(np.uint16)


def photo_sequence(seed, n, motion):
    dy, dx = motion
    return [camera(seed, shift=(int(round(dy * i)), int(round(dx * i)))) for i in range(n)]


def photo_single(frames, K, fixed, ref_every):
    """RGBDOdometry::processFrame's engine calls on a one-stream context configured with K"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    out = []
    with DvoContext(1) as ctx:
        ctx.photo_configure(K, fixed=fixed)
        T, n_frame = np.eye(4), 0
        for bgr, d16 in frames:
            up = lambda slot: ctx.frames_upload_cameras([bgr], [d16.astype(np.float32)], n_levels=4, first_shift=0, first_slot=slot,
                                                        flags=DVO_UPLOAD_DEPTH_RAW)
            ev = 0
            if n_frame % ref_every == 0:
                up(0)
                ctx.photo_set_ref(0, first_level=1)
                T, ev = np.eye(4), 1
            up(1)
            T, norms, upd = ctx.photo_align(1, T, levels=LEVELS)
            out.append((T.copy(), norms, list(upd), ev))
            n_frame += 1
    return out


@pytest.mark.parametrize("fixed", [False, True])
def test_photo_streams_two_camera_matrices(fixed):
    from rgbd_odometry_amd import DvoContext, DvoError, DvoPhotoStreams
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE, DVO_UPLOAD_DEPTH_RAW
    with time_limit(900):
        n_s, n_t = 4, 6
        cams = [K640, K640_B, K640_B, K640]
        seqs = [photo_sequence(70 + s, n_t, ((s % 3) - 1.0, 2.0 - (s % 5))) for s in range(n_s)]
        got = {s: [] for s in range(n_s)}
        with DvoPhotoStreams(n_s, K640, fixed=fixed, ref_every=3) as ps:
            for s in range(n_s):
                if cams[s] != K640:
                    ps.set_stream_intrinsics(s, *cams[s])
            for call in (lambda: ps.set_stream_intrinsics(n_s, *K640_B), lambda: ps.set_stream_intrinsics(0, 0.0, 1.0, 1.0, 1.0),
                         lambda: ps.set_stream_intrinsics(0, 1.0, -2.0, 1.0, 1.0)):
                with pytest.raises(DvoError) as e:
                    call()
                assert e.value.code == DVO_ERR_INVALID
            launches = []
            for t in range(n_t):
                res = ps.step(list(range(n_s)), [seqs[s][t][0] for s in range(n_s)], [seqs[s][t][1] for s in range(n_s)])
                launches.append(ps.stats())
                for s in range(n_s):
                    got[s].append((res["T"][s].copy(), res["norms"][s].copy(), [int(x) for x in res["updates"][s]], int(res["event"][s])))
                if t == 0:
                    with pytest.raises(DvoError) as e:
                        ps.set_stream_intrinsics(1, *K640)
                    assert e.value.code == DVO_ERR_STATE
            # the Jacobians of the current references (frame 3) equal the single path's under the stream's K
            for s in (0, 1):
                with DvoContext(1) as ctx:
                    ctx.frames_upload_cameras([seqs[s][3][0]], [seqs[s][3][1].astype(np.float32)], n_levels=4, first_shift=0,
                                              flags=DVO_UPLOAD_DEPTH_RAW)
                    ctx.photo_configure(cams[s], fixed=fixed)
                    ctx.photo_set_ref(0, first_level=1)
                    for l in (1, 2, 3):
                        want, have = ctx.photo_jacobian(l), ps.jacobian(s, l)
                        assert have["n"] == want["n"] > 100
                        for k in ("J", "sel_i", "sel_j", "A"):
                            assert np.array_equal(have[k], want[k]), (fixed, s, l, k)
        with DvoPhotoStreams(n_s, K640, fixed=fixed, ref_every=3) as ps:
            uniform = []
            for t in range(n_t):
                ps.step(list(range(n_s)), [seqs[s][t][0] for s in range(n_s)], [seqs[s][t][1] for s in range(n_s)])
                uniform.append(ps.stats())
        assert [(u["launches"], u["syncs"], u["runs"]) for u in uniform] == [(m["launches"], m["syncs"], m["runs"]) for m in launches]
        for s in range(n_s):
            want = photo_single(seqs[s], cams[s], fixed, 3)
            for n, ((T, norms, upd, ev), (wT, wn, wu, we)) in enumerate(zip(got[s], want)):
                assert ev == we and np.array_equal(T, wT) and np.array_equal(norms, wn) and upd == list(wu), (s, n)
        # wrong-K guard: streams 0 and 3 (handle K) and 1 and 2 (their own) see different frames; stream 1 against the handle's K
        other = photo_single(seqs[1], K640, fixed, 3)
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(got[1], other))
