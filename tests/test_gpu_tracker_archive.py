"""Key-frame archive and loop-closure alignment of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_archive,
dvo_tracker_score, dvo_tracker_match; kernels in dvo_tracker_archive.hip).

Geometry and helpers of tests/test_gpu_tracker_information.py: 240 x 320, 3 levels, 8 iterations each, one launch shape everywhere,
3 streams and 7 ticks (tick 5 is the forced key-frame switch).  Stream 0's last frame is generated with shift (0, 0) again: the
revisit a loop closure is made of.

Expected values.  Archive: dvo_get_ref_level of the tracker's context right after the step, bit for bit.  Score: the CPU oracle's
accumulators (oracle_lib.accumulate) on the ARCHIVED points and dvo_get_now_level of the stream; n_visible and sum_eps2 (the
correctly rounded exact sum) equal, H and g -- double sums of exact products whose order of addition differs -- within the project's
rule for them (rtol 1e-12, atol 1e-12 max|want|: tests/test_gpu_parity.py::test_normal_matrix_of_every_iterate).  Match: the pose a
tracker (identity guess) or a one-pair context (any guess) computes from the same two frames -- the same kernel, the same launch shape,
the same data, hence bit for bit."""
import ctypes

import numpy as np
import pytest

import frame_gen
import test_gpu_tracker_information as TI

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT, ITERS, K, ENGINE = TI.ROWS, TI.COLS, TI.NL, TI.SHIFT, TI.ITERS, TI.K, TI.ENGINE
N_S, N_T = 3, 7
FULL = [[(s, n) for s in range(N_S)] for n in range(N_T)]
MATCH_LAUNCHES, STORE_LAUNCHES = 3, 1                  # DVO_TRACKER_MATCH_LAUNCHES, DVO_TRACKER_ARCHIVE_LAUNCHES of the header
FIELDS = ("H", "g", "sum_eps2", "n_points", "n_visible")


@pytest.fixture(scope="module")
def seqs():
    out = [TI.sequence(900 + s, N_T, TI.MOTIONS[s]) for s in range(N_S)]
    out[0][N_T - 1] = frame_gen.camera_frame(900, ROWS, COLS, shift=(0, 0), holes=True)       # stream 0 comes back to where it started
    return out


def make(n, archive=(8, 4, None), information=True, every=5, **engine):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in dict(ENGINE, **engine).items():
        setattr(p, k, v)
    tr = DvoTracker(n, params=p, iters=ITERS, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, key_frame_every=every)
    tr.set_intrinsics(*K)
    if information:
        tr.set_information(True)
    if archive is not None:
        tr.set_archive(archive[0], archive[1], archive[2])
    return tr


def step(tr, seqs, entry):
    streams = [s for s, _ in entry]
    return tr.step(streams, [seqs[s][i][0] for s, i in entry], [seqs[s][i][1] for s, i in entry])


def ref_level(tr, stream, level):
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    n = ctypes.c_int()
    assert lib.dvo_get_ref_level(h, stream, level, None, 0, ctypes.byref(n)) == 0
    xyz = np.zeros((n.value, 3), np.float32)
    assert lib.dvo_get_ref_level(h, stream, level, capi._ptr(xyz), n.value, ctypes.byref(n)) == 0
    return xyz


def now_level(tr, stream, level):
    return TI.resident(tr, stream, level)[1:]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_record(a, b):
    return all(same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in FIELDS)


def check_record(oracle, xyz, now, level, R, t, rec, what):
    """rec against the oracle's accumulators of the points xyz and the now level (dt, gx, gy) at (R, t)"""
    rows, cols = TI.level_dims(level)
    want = oracle.accumulate(level, xyz, 0, len(xyz), now[0], now[1], now[2], rows, cols, K, R, t)
    H = np.zeros((6, 6)); k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = want[k]; k += 1
    g = want[21:27]
    print(what, "N", len(xyz), "visible", rec["n_visible"], int(want[28]), "sum_eps2", rec["sum_eps2"], want[27],
          "max rel dH %.3g" % (np.abs(rec["H"] - H).max() / np.abs(H).max()), "max rel dg %.3g" % (np.abs(rec["g"] - g).max() / np.abs(g).max()))
    assert rec["n_points"] == len(xyz), what
    assert rec["n_visible"] == int(want[28]) and rec["n_visible"] > 6, what
    assert rec["sum_eps2"] == want[27], (what, rec["sum_eps2"], want[27])
    np.testing.assert_allclose(rec["H"], H, rtol=1e-12, atol=1e-12 * np.abs(H).max(), err_msg=str(what))
    np.testing.assert_allclose(rec["g"], g, rtol=1e-12, atol=1e-12 * np.abs(g).max(), err_msg=str(what))


def refused(code, fn, *a, **kw):
    from rgbd_odometry_amd import DvoError
    with pytest.raises(DvoError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def run(tr, seqs, archive, probe=False):
    """the 7-tick run; archive: check every new key frame against the context; probe: score and match between the ticks"""
    ticks, ids = [], {}
    for n, entry in enumerate(FULL):
        R, t, ev = step(tr, seqs, entry)
        out = dict(R=R, t=t, ev=ev.copy(), stats=tr.stats(), rec={s: tr.information(s) for s in range(N_S)},
                   sig={s: tr.signals(s) for s in range(N_S) if ev[s] != 1})
        for s in range(N_S):
            if not archive or ev[s] == 0:
                continue
            kid = tr.key_frame_id(s)
            assert kid == len(ids), (n, s, kid)                 # ids count up by one per key frame
            ids[(n, s)] = kid
            info = tr.archive_info(kid)
            pts = [tr.archive_points(kid, l) for l in range(NL)]
            for l in range(NL):
                want = ref_level(tr, s, l)
                assert len(want) > 64 and same_bits(pts[l], want), (n, s, l, len(pts[l]), len(want))
            assert info == dict(stream=s, frame=0 if ev[s] == 1 else n - 1, n_points=[len(p) for p in pts]), (n, s, info)
        if probe and n >= 1:
            cand = [(0, tr.key_frame_id(1)), (2, tr.key_frame_id(0))]
            tr.score([c[0] for c in cand], [c[1] for c in cand], 0, R[:2], t[:2])
            st = tr.archive_stats()
            assert (st["last_launches"], st["last_syncs"]) == (1, 1), (n, st)
            tr.match([c[0] for c in cand], [c[1] for c in cand])
            st = tr.archive_stats()
            assert (st["last_launches"], st["last_syncs"]) == (MATCH_LAUNCHES, 1), (n, st)
        ticks.append(out)
    return ticks, ids


@pytest.fixture(scope="module")
def closed(seqs):
    """the 7-tick run with the archive on, left open for the tests that score and match against it"""
    tr = make(N_S)
    ticks, ids = run(tr, seqs, archive=True)
    yield tr, ticks, ids
    tr.close()


def test_archive_holds_every_key_frame(closed):
    """run() compared every new key frame with dvo_get_ref_level of the context, level by level, and its archive_info"""
    tr, ticks, ids = closed
    assert [x["ev"].tolist() for x in ticks] == [[1] * N_S] + [[0] * N_S] * 4 + [[5] * N_S] + [[0] * N_S]
    assert sorted(ids) == [(0, s) for s in range(N_S)] + [(5, s) for s in range(N_S)]
    st = tr.archive_stats()
    assert (st["archived"], st["refused"], st["evicted"]) == (2 * N_S, 0, 0)
    # the first key frames are still there, untouched by the later ones
    for s in range(N_S):
        assert tr.archive_info(ids[(0, s)])["stream"] == s and tr.archive_info(ids[(0, s)])["frame"] == 0
        assert tr.key_frame_id(s) == ids[(5, s)]


def test_ring_evicts_the_oldest(seqs):
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    # one stream, a key frame on ticks 0, 2, 3, 4 (key_frame_every = 2), two slots
    with make(1, archive=(2, 1, None), every=2) as tr:
        ids = []
        for n in range(5):
            _, _, ev = step(tr, seqs, [(0, n)])
            if ev[0]:
                ids.append(tr.key_frame_id(0))
                assert same_bits(tr.archive_points(ids[-1], 0), ref_level(tr, 0, 0)), n
        assert ids == list(range(len(ids))) and len(ids) >= 3, ids
        for kid in ids[:-2]:
            refused(DVO_ERR_STATE, tr.archive_info, kid)
            refused(DVO_ERR_STATE, tr.archive_points, kid, 0)
            refused(DVO_ERR_STATE, tr.score, [0], [kid], 0, np.eye(3)[None], np.zeros((1, 3)))
        for kid in ids[-2:]:
            assert tr.archive_info(kid)["stream"] == 0
        refused(DVO_ERR_STATE, tr.archive_info, ids[-1] + 1)       # never given
        refused(DVO_ERR_STATE, tr.archive_info, -1)
        st = tr.archive_stats()
        assert (st["archived"], st["evicted"], st["refused"]) == (len(ids), len(ids) - 2, 0)
    # three new key frames in ONE tick, two slots: the first is evicted at once, the other two are whole
    with make(N_S, archive=(2, 1, None)) as tr:
        step(tr, seqs, FULL[0])
        assert [tr.key_frame_id(s) for s in range(N_S)] == [-1, 1, 2]
        refused(DVO_ERR_STATE, tr.archive_info, 0)
        for s in (1, 2):
            for l in range(NL):
                assert same_bits(tr.archive_points(s, l), ref_level(tr, s, l)), (s, l)
        assert tr.archive_stats()["evicted"] == 1


def test_small_slots_refuse_and_count(seqs):
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    with make(N_S, archive=(8, 2, [16, 16, 16])) as tr:
        for n in range(N_T):
            step(tr, seqs, FULL[n])
            assert [tr.key_frame_id(s) for s in range(N_S)] == [-1] * N_S, n
        st = tr.archive_stats()
        assert (st["archived"], st["refused"], st["evicted"]) == (0, 2 * N_S, 0)
        refused(DVO_ERR_STATE, tr.archive_info, 0)
        refused(DVO_ERR_STATE, tr.score, [0], [0], 0, np.eye(3)[None], np.zeros((1, 3)))


def loop_candidates(closed):
    """stream 0's last frame (shift (0, 0) again) against its key frames of tick 0 and of tick 5"""
    tr, ticks, ids = closed
    return tr, [0, 0], [ids[(0, 0)], ids[(5, 0)]], ticks[-1]["R"][0], ticks[-1]["t"][0]


def test_score_the_loop_closure_against_the_oracle(closed, oracle):
    tr, streams, keys, R_step, t_step = loop_candidates(closed)
    for level in (0, 2):
        now = now_level(tr, 0, level)
        for name, R, t in (("identity", np.eye(3), np.zeros(3)), ("step pose", R_step, t_step)):
            recs = tr.score(streams, keys, level, np.stack([R, R]), np.stack([t, t]))
            for kid, rec in zip(keys, recs):
                check_record(oracle, tr.archive_points(kid, level), now, level, R, t, rec, ("level", level, name, "key", kid))
    # the revisit: at the identity the frame is the first key frame's own view (residuals of rounding only), while the key frame of tick 5
    # saw the scene (2, -4) pixels away: the mean squared residual tells the two apart
    a, b = tr.score(streams, keys, 0, np.stack([np.eye(3)] * 2), np.zeros((2, 3)))
    assert a["sum_eps2"] / a["n_visible"] < b["sum_eps2"] / b["n_visible"], (a["sum_eps2"], a["n_visible"], b["sum_eps2"], b["n_visible"])


def test_score_record_depends_on_its_candidate_alone(closed):
    tr, ticks, ids = closed
    cand = [(0, ids[(0, 0)]), (0, ids[(5, 0)]), (0, ids[(5, 1)])]          # the last one: another stream's key frame, same camera model
    poses = [(np.eye(3), np.zeros(3)), (ticks[-1]["R"][0], ticks[-1]["t"][0]), (ticks[-1]["R"][1], ticks[-1]["t"][1])]
    for level in (0, 2):
        alone = [tr.score([s], [k], level, R[None], t[None])[0] for (s, k), (R, t) in zip(cand, poses)]
        order = [2, 0, 1]
        both = tr.score([cand[i][0] for i in order], [cand[i][1] for i in order], level, np.stack([poses[i][0] for i in order]),
                        np.stack([poses[i][1] for i in order]))
        for j, i in enumerate(order):
            assert same_record(alone[i], both[j]), (level, i, alone[i], both[j])
        assert all(r["n_visible"] > 6 for r in alone)


@pytest.mark.parametrize("tick", [0, 5])
def test_match_from_the_identity_is_a_trackers_second_step(closed, seqs, tick):
    """key frame of event 1 (frame 0) and of the tick-5 switch (frame 4 = frame n - 1), each against stream 0's last frame"""
    tr, ticks, ids = closed
    key_frame = seqs[0][0 if tick == 0 else 4]
    with make(1, archive=None, information=False, every=1000) as solo:
        solo.step([0], [key_frame[0]], [key_frame[1]])
        R, t, ev = solo.step([0], [seqs[0][N_T - 1][0]], [seqs[0][N_T - 1][1]])
    assert ev[0] == 0
    Rm, tm, recs = tr.match([0], [ids[(tick, 0)]])
    print("tick", tick, "t", tm[0], "visible", recs[0]["n_visible"], "of", recs[0]["n_points"])
    assert same_bits(Rm[0], R[0]) and same_bits(tm[0], t[0]), (Rm[0], R[0], tm[0], t[0])
    assert recs[0]["n_visible"] > 6


def rodrigues(w):
    th = np.linalg.norm(w)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def test_match_from_a_guess_is_a_one_pair_alignment(closed, seqs, oracle):
    """arranged as tests/test_gpu_tracker_streams.py::single_stream: key frame -> reference, now frame -> now, dvo_set_poses +
    dvo_align_batch from the same guess; two candidates in one call, against stream 0's and stream 1's current frames"""
    from rgbd_odometry_amd import DvoContext
    tr, ticks, ids = closed
    cand = [(0, ids[(0, 0)], seqs[0][0]), (1, ids[(5, 1)], seqs[1][4])]
    R0 = np.stack([rodrigues((0.004, -0.003, 0.002)), rodrigues((-0.002, 0.005, 0.001))])
    t0 = np.array([[0.004, -0.002, 0.003], [-0.003, 0.001, 0.002]])
    before = [(tr.information(s), tr.signals(s), tr.key_frame_id(s)) for s in range(N_S)]
    Rm, tm, recs = tr.match([c[0] for c in cand], [c[1] for c in cand], R0, t0)
    for i, (s, kid, key_frame) in enumerate(cand):
        with DvoContext(1, **ENGINE) as ctx:
            ctx.set_intrinsics(*K)
            ctx.frames_upload_cameras([key_frame[0]], [key_frame[1]], n_levels=NL, first_shift=SHIFT, first_slot=0)
            ctx.frames_as_ref(0, 0, 1)
            ctx.frames_upload_cameras([seqs[s][N_T - 1][0]], [seqs[s][N_T - 1][1]], n_levels=NL, first_shift=SHIFT, first_slot=1)
            ctx.frames_as_now(1, 0, 1)
            R, t = ctx.align_batch(ITERS, R0[i][None].copy(), t0[i][None].copy())
        assert same_bits(Rm[i], R[0]) and same_bits(tm[i], t[0]), (i, Rm[i], R[0], tm[i], t[0])
        check_record(oracle, tr.archive_points(kid, 0), now_level(tr, s, 0), 0, Rm[i], tm[i], recs[i], ("match", i))
    after = [(tr.information(s), tr.signals(s), tr.key_frame_id(s)) for s in range(N_S)]
    for a, b in zip(before, after):
        assert TI.same_record(a[0], b[0]) and a[1:] == b[1:]


def test_nothing_else_moves(seqs):
    """archive off against on with score and match between the ticks: the same poses, events, signals and information records, the same
    synchronisations per step; the launches of a step with new key frames grow by the store's (first frames and switches never share a
    tick here), others by nothing"""
    with make(N_S, archive=None) as tr:
        off, _ = run(tr, seqs, archive=False)
    with make(N_S) as tr:
        on, _ = run(tr, seqs, archive=True, probe=True)
    for n, (a, b) in enumerate(zip(on, off)):
        assert same_bits(a["R"], b["R"]) and same_bits(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"], n
        assert all(TI.same_record(a["rec"][s], b["rec"][s]) for s in range(N_S)), n
        assert a["stats"]["syncs"] == b["stats"]["syncs"], (n, a["stats"], b["stats"])
        extra = STORE_LAUNCHES if n in (0, 5) else 0
        assert a["stats"]["launches"] == b["stats"]["launches"] + extra, (n, a["stats"], b["stats"])
        assert {k: v for k, v in a["stats"].items() if k != "launches"} == {k: v for k, v in b["stats"].items() if k != "launches"}, n
    assert [x["stats"]["key_frames"] for x in off] == [0, 0, 0, 0, 0, N_S, 0]


def test_contract(seqs):
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE
    eye, zero = np.eye(3)[None], np.zeros((1, 3))
    with make(4, archive=None) as tr:
        refused(DVO_ERR_STATE, tr.key_frame_id, 0)                              # off by default
        refused(DVO_ERR_STATE, tr.score, [0], [0], 0, eye, zero)
        refused(DVO_ERR_INVALID, tr.set_archive, -1, 2)
        refused(DVO_ERR_INVALID, tr.set_archive, 4, 0)
        refused(DVO_ERR_INVALID, tr.set_archive, 4, 2, [0, -5, 0])
        refused(DVO_ERR_STATE, tr.key_frame_id, 0)                              # nothing changed: still off
        tr.set_stream_intrinsics(1, 250.0, 254.0, 161.0, 118.0)                 # stream 1: another camera model
        tr.set_archive(4, 2)
        refused(DVO_ERR_STATE, tr.key_frame_id, 0)                              # never stepped
        for n in range(2):
            step(tr, seqs, [(s, n) for s in range(3)])                          # stream 3 stays at its start
        ids = [tr.key_frame_id(s) for s in range(3)]
        assert ids == [0, 1, 2]

        def state():
            return (tr.archive_stats(), tr.stats(), [tr.key_frame_id(s) for s in range(3)], [tr.information(s) for s in range(3)],
                    [tr.signals(s) for s in range(3)])

        ok = tr.score([2, 0], [ids[0], ids[2]], 0, np.stack([np.eye(3)] * 2), np.zeros((2, 3)))       # another stream's key frame, same model
        assert all(r["n_visible"] > 6 for r in ok)
        tr.match([2], [ids[0]])
        before = state()
        for call in (lambda s, k: tr.score(s, k, 0, np.tile(np.eye(3), (len(s), 1, 1)), np.zeros((len(s), 3))), lambda s, k: tr.match(s, k)):
            refused(DVO_ERR_INVALID, call, [], [])                              # n outside [1, max_matches]
            refused(DVO_ERR_INVALID, call, [0, 0, 0], [ids[0]] * 3)
            refused(DVO_ERR_INVALID, call, [4], [ids[0]])                       # stream outside [0, max_streams)
            refused(DVO_ERR_INVALID, call, [-1], [ids[0]])
            refused(DVO_ERR_INVALID, call, [1], [ids[0]])                       # key frame enlisted under another camera model
            refused(DVO_ERR_INVALID, call, [0], [ids[1]])
            refused(DVO_ERR_STATE, call, [3], [ids[0]])                         # never stepped: no now frame
            refused(DVO_ERR_STATE, call, [0], [7])                              # unknown id
            refused(DVO_ERR_STATE, call, [0], [-1])
        refused(DVO_ERR_INVALID, tr.score, [0], [ids[0]], NL, eye, zero)        # level outside the tracker's
        refused(DVO_ERR_INVALID, tr.score, [0], [ids[0]], -1, eye, zero)
        refused(DVO_ERR_INVALID, tr.key_frame_id, 4)
        refused(DVO_ERR_INVALID, tr.archive_points, ids[0], NL)
        after = state()
        assert before[:3] == after[:3] and before[4] == after[4]
        assert all(TI.same_record(a, b) for a, b in zip(before[3], after[3]))
        own = tr.match([1], [ids[1]])                                           # stream 1 against its own key frame, under its model
        assert own[2][0]["n_visible"] > 6
        tr.set_archive(0)                                                       # off again: the ids are gone, tracking goes on
        refused(DVO_ERR_STATE, tr.archive_info, ids[0])
        step(tr, seqs, [(s, 2) for s in range(3)])
    for kw in (dict(interpolate_dt=1), dict(engine_variant=1), dict(debug_alias_mod=1)):
        with make(1, archive=None, information=False, **kw) as tr:
            refused(DVO_ERR_INVALID, tr.set_archive, 4, 2)
            refused(DVO_ERR_STATE, tr.key_frame_id, 0)                          # nothing changed: still off
            assert tr.archive_stats() == dict(archived=0, refused=0, evicted=0, last_launches=0, last_syncs=0), kw
