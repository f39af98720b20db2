"""Depth verification of loop-closure candidates of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_verify; kernel in
dvo_tracker_verify.hip).

Geometry and helpers of tests/test_gpu_tracker_archive.py: 240 x 320, 3 levels, 8 iterations each, 3 streams and the 7-tick schedule;
stream 0's last frame is its tick-0 frame again.  A record is seven integers, each with one value whatever the order of the reduction:
EVERY comparison below is equality of all seven with the numpy restatement (tests/verify_reference.py) on the ARCHIVED points
(dvo_tracker_archive_get_points) and the depth image of the oracle's pyramid of the frame that was fed.  That every class of point
occurs in these inputs is asserted, on the reference alone, by tests/test_tracker_verify_cpu.py."""
import ctypes

import numpy as np
import pytest

import test_gpu_tracker_archive as TA
import test_gpu_tracker_information as TI
import test_gpu_tracker_views as TV
import frame_reference as fr
import verify_reference as vr
from test_gpu_tracker_archive import seqs  # noqa: F401  (the fixture: the frames of the 7-tick run)

pytestmark = pytest.mark.gpu

NL, SHIFT, K, N_S, N_T = TA.NL, TA.SHIFT, TA.K, TA.N_S, TA.N_T
MAX_MATCHES = 16
EYE, ZERO = np.eye(3), np.zeros(3)
SIDEWAYS = (EYE, np.array([50.0, 0.0, 0.0]))           # 50 m to the side: every point projects far outside the image


class Planes:
    """depth image (rows, cols float32 mm) of a level of the oracle's pyramid of a fed frame, computed once per frame"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, frame, level, nl=NL, shift=SHIFT):
        key = (id(frame[0]), nl, shift)
        if key not in self.cache:
            self.cache[key] = (frame, self.oracle.build_pyramid(frame[0], frame[1], n_levels=nl, first_shift=shift))
        return np.asarray(self.cache[key][1][level][1]).astype(np.float32)


@pytest.fixture(scope="module")
def planes(oracle):
    return Planes(oracle)


@pytest.fixture(scope="module")
def closed(seqs):  # noqa: F811
    """the 7-tick run with the archive on (16 candidates per call), left open for the tests that verify against it"""
    tr = TA.make(N_S, archive=(8, MAX_MATCHES, None))
    ticks, ids = TA.run(tr, seqs, archive=True)
    yield tr, ticks, ids
    tr.close()


def batches(items, n=MAX_MATCHES):
    return [items[i:i + n] for i in range(0, len(items), n)]


def verify_all(tr, cands, level, poses, **tol):
    """cands: [(stream, key id)], poses: [(R, t)] -> records, in calls of at most MAX_MATCHES candidates"""
    out = []
    for idx in batches(list(range(len(cands)))):
        out += tr.verify([cands[i][0] for i in idx], [cands[i][1] for i in idx], level, np.stack([poses[i][0] for i in idx]),
                         np.stack([poses[i][1] for i in idx]), **tol)
    return out


def check(oracle, got, xyz, plane, level, Ks, R, t, what, **tol):
    want = vr.verify(oracle, level, xyz, plane, Ks, R, t, **tol)
    print(what, "device", got, "" if got == want else "REFERENCE %s" % want)
    assert got == want, (what, got, want)
    return want


def test_parity_on_every_stream_key_frame_level_and_pose(closed, seqs, oracle, planes):  # noqa: F811
    tr, ticks, ids = closed
    cands = [(s, kid) for s in range(N_S) for kid in sorted(ids.values())]
    assert len(cands) == N_S * 2 * N_S
    matched = []
    for b in batches(cands):
        Rm, tm, _ = tr.match([c[0] for c in b], [c[1] for c in b])
        matched += list(zip(Rm, tm))
    kinds = dict(identity=[(EYE, ZERO)] * len(cands), matched=matched, perturbed=[vr.perturbed(R, t) for R, t in matched])
    seen = dict.fromkeys(("n_agree", "n_front", "n_behind", "no measurement", "invisible"), 0)
    for level in range(NL):
        pts = {kid: tr.archive_points(kid, level) for kid in sorted(ids.values())}
        for kind, poses in kinds.items():
            recs = verify_all(tr, cands, level, poses)
            st = tr.archive_stats()
            assert (st["last_launches"], st["last_syncs"]) == (1, 1), st
            for (s, kid), (R, t), rec in zip(cands, poses, recs):
                w = check(oracle, rec, pts[kid], planes(seqs[s][N_T - 1], level), level, K, R, t, ("level", level, kind, "stream", s, "key", kid))
                assert w["n_points"] == len(pts[kid]) > 64
                for k, v in (("n_agree", w["n_agree"]), ("n_front", w["n_front"]), ("n_behind", w["n_behind"]),
                             ("no measurement", w["n_visible"] - w["n_depth"]), ("invisible", w["n_points"] - w["n_visible"])):
                    seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    # the revisit: stream 0's last frame against its own tick-0 key frame agrees at the matched pose, and the verdict says so; at the
    # perturbed pose the same candidate does not pass
    from rgbd_odometry_amd.capi import depth_verdict
    i = cands.index((0, ids[(0, 0)]))
    rev = tr.verify([0], [ids[(0, 0)]], 0, matched[i][0][None], matched[i][1][None])[0]
    assert rev["n_agree"] > rev["n_depth"] / 2 and depth_verdict(rev, 0.8, 0.05, 64), rev
    bad = tr.verify([0], [ids[(0, 0)]], 0, kinds["perturbed"][i][0][None], kinds["perturbed"][i][1][None])[0]
    assert not depth_verdict(bad, 0.8, 0.05, 64), bad


def test_boundary_residual_agrees(closed, seqs, oracle, planes):  # noqa: F811
    """tol_rel = 0 and tol_mm = the median |r| of the candidate's own residuals: the point(s) with |r| == tol agree"""
    tr, ticks, ids = closed
    for s, key, level, pose in ((0, (5, 0), 0, vr.perturbed(EYE, ZERO)), (1, (0, 2), 0, (EYE, ZERO)), (2, (5, 1), 2, vr.perturbed(EYE, ZERO)),
                                (0, (0, 0), 1, vr.perturbed(ticks[-1]["R"][0], ticks[-1]["t"][0]))):
        kid = ids[key]
        xyz, plane = tr.archive_points(kid, level), planes(seqs[s][N_T - 1], level)
        vis, has, r, _ = vr.residuals(oracle, level, xyz, plane, K, *pose)
        a = np.sort(np.abs(r[has]))
        tol = float(a[len(a) // 2])                            # one of the residuals themselves, a float32
        at = int((has & (np.abs(r) == np.float32(tol))).sum())
        assert at >= 1 and np.float32(tol) == tol
        got = tr.verify([s], [kid], level, pose[0][None], pose[1][None], tol_mm=tol, tol_rel=0.0)[0]
        want = check(oracle, got, xyz, plane, level, K, *pose, ("boundary", s, key, level, "tol", tol, "points at it", at), tol_mm=tol, tol_rel=0.0)
        assert want["n_agree"] == int((has & (np.abs(r) <= np.float32(tol))).sum()) >= len(a) // 2 + 1
        assert want["n_front"] + want["n_behind"] > 0


def test_depth_domain_on_the_device(seqs, oracle):  # noqa: F811
    """one tick fed with DVO_UPLOAD_DEPTH_RAW float depth (sensor units: millimetres, stored as they are) carrying patches of 0, 0.5,
    1.0, 70000, +inf and NaN: none of them is a measurement"""
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    bgr, depth_m = seqs[0][1]
    raw = fr.depth_m_to_mm16(depth_m).astype(np.float32)
    rows, cols = raw.shape
    values = (0.0, 0.5, 1.0, 70000.0, np.inf, np.nan)
    for k, v in enumerate(values):                               # six bands across the whole height, 30 columns each
        raw[:, 20 + 50 * k:50 + 50 * k] = v
    with TA.make(1, archive=(4, 2, None)) as tr:
        TA.step(tr, seqs, [(0, 0)])
        kid = tr.key_frame_id(0)
        tr.step([0], [bgr], [raw], flags=DVO_UPLOAD_DEPTH_RAW)
        for level in range(NL):
            plane = fr.resize_nn(raw, level)
            for v in values:
                assert (np.isnan(plane) if np.isnan(v) else plane == np.float32(v)).sum() >= plane.shape[0] * (30 >> level) // 2, (level, v)
            xyz = tr.archive_points(kid, level)
            for name, pose in (("identity", (EYE, ZERO)), ("perturbed", vr.perturbed(EYE, ZERO))):
                got = tr.verify([0], [kid], level, pose[0][None], pose[1][None])[0]
                want = check(oracle, got, xyz, plane, level, K, *pose, ("raw depth", level, name))
                assert want["n_visible"] - want["n_depth"] > want["n_visible"] // 8 and want["n_depth"] > 0, want
            # max_depth_mm is inclusive, min_depth_mm exclusive: with (0.25, 70000] the bands of 0.5, 1.0 and 70000 ARE measurements
            got = tr.verify([0], [kid], level, EYE[None], ZERO[None], min_depth_mm=0.25, max_depth_mm=70000.0)[0]
            wide = check(oracle, got, xyz, plane, level, K, EYE, ZERO, ("raw depth, wide domain", level), min_depth_mm=0.25, max_depth_mm=70000.0)
            assert wide["n_depth"] > vr.verify(oracle, level, xyz, plane, K, EYE, ZERO)["n_depth"]


def test_odd_geometry_and_nothing_visible(oracle, planes):
    """250 x 322 frames at full resolution (the views test's geometry: rows and cols no multiples of any tile), and a pose that leaves
    no point visible"""
    geom = dict(rows=250, cols=322, nl=2, shift=0)
    s = TV.sequence(77, 3, (1.0, -1.5), 250, 322)
    with TV.tracked(1, iters=[8, 8], views=False, geom=geom) as tr:
        tr.set_archive(4, 4)
        for n in range(3):
            tr.step([0], [s[n][0]], [s[n][1]])
        kid = tr.key_frame_id(0)
        for level in range(2):
            xyz, plane = tr.archive_points(kid, level), planes(s[2], level, 2, 0)
            assert plane.shape == TV.level_dims(geom, level)
            poses = [(EYE, ZERO), vr.perturbed(EYE, ZERO), SIDEWAYS]
            recs = tr.verify([0] * 3, [kid] * 3, level, np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]))
            for name, pose, rec in zip(("identity", "perturbed", "sideways"), poses, recs):
                check(oracle, rec, xyz, plane, level, K, *pose, ("odd geometry", level, name))
            assert recs[0]["n_agree"] > 64
            assert recs[2] == dict(n_points=len(xyz), n_visible=0, n_depth=0, n_agree=0, n_front=0, n_behind=0, sum_abs_q4=0), recs[2]


def test_list_longer_than_one_trip(oracle, planes):
    """480 x 640 at full resolution: a list of several trips of the walk (2048 points each) with a ragged last one"""
    frames = vr.long_list_frames()
    geom = dict(rows=vr.LONG_ROWS, cols=vr.LONG_COLS, nl=1, shift=0)
    with TV.tracked(1, iters=[4], views=False, geom=geom) as tr:
        tr.set_intrinsics(*vr.LONG_K)
        tr.set_archive(2, 2)
        for f in frames:
            tr.step([0], [f[0]], [f[1]])
        kid = tr.key_frame_id(0)
        xyz, plane = tr.archive_points(kid, 0), planes(frames[1], 0, 1, 0)
        assert len(xyz) > 2 * 2048 and len(xyz) % 2048
        for name, pose in (("identity", (EYE, ZERO)), ("perturbed", vr.perturbed(EYE, ZERO))):
            got = tr.verify([0], [kid], 0, pose[0][None], pose[1][None])[0]
            want = check(oracle, got, xyz, plane, 0, vr.LONG_K, *pose, ("long list", name))
            assert want["n_depth"] > 2048


def test_mixed_rig(seqs, oracle, planes):  # noqa: F811
    """stream 1 has intrinsics of its own: its key frames verify under ITS model, a pair across the two models is refused"""
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    K1 = (250.0, 254.0, 161.0, 118.0)
    with TA.make(2, archive=(4, 2, None)) as tr:
        tr.set_stream_intrinsics(1, *K1)
        for n in range(2):
            TA.step(tr, seqs, [(0, n), (1, n)])
        ids = [tr.key_frame_id(s) for s in range(2)]
        pose = vr.perturbed(EYE, ZERO)
        recs = tr.verify([0, 1], ids, 0, np.stack([EYE, pose[0]]), np.stack([ZERO, pose[1]]))
        check(oracle, recs[0], tr.archive_points(ids[0], 0), planes(seqs[0][1], 0), 0, K, EYE, ZERO, "shared model")
        w = check(oracle, recs[1], tr.archive_points(ids[1], 0), planes(seqs[1][1], 0), 0, K1, *pose, "own model")
        assert w != vr.verify(oracle, 0, tr.archive_points(ids[1], 0), planes(seqs[1][1], 0), K, *pose)       # the model matters
        TA.refused(DVO_ERR_INVALID, tr.verify, [1], [ids[0]], 0, EYE[None], ZERO[None])
        TA.refused(DVO_ERR_INVALID, tr.verify, [0], [ids[1]], 0, EYE[None], ZERO[None])


def test_record_depends_on_its_candidate_alone(closed):
    tr, ticks, ids = closed
    R6, t6 = ticks[-1]["R"], ticks[-1]["t"]
    cand = [(0, ids[(0, 0)], EYE, ZERO), (0, ids[(5, 0)], R6[0], t6[0]), (1, ids[(5, 2)], *vr.perturbed(R6[1], t6[1])),
            (2, ids[(0, 1)], *vr.perturbed(EYE, ZERO))]
    for level in (0, 2):
        def call(idx):
            return tr.verify([cand[i][0] for i in idx], [cand[i][1] for i in idx], level, np.stack([cand[i][2] for i in idx]),
                             np.stack([cand[i][3] for i in idx]))
        alone = [call([i])[0] for i in range(len(cand))]
        assert all(r["n_depth"] > 64 for r in alone) and len({tuple(r.values()) for r in alone}) == len(cand)
        order = [2, 0, 3, 1]
        assert call(order) == [alone[i] for i in order], level
        full = [i % len(cand) for i in range(MAX_MATCHES)]      # a batch of max_matches
        assert call(full) == [alone[i] for i in full], level


def test_nothing_else_moves(seqs):  # noqa: F811
    """the 7-tick schedule with verify calls between the ticks and without: the same poses, events, signals, information records and
    stats() of every step, bit for bit; a verify call is one launch and one synchronisation"""
    def run(probe):
        with TA.make(N_S, archive=(8, MAX_MATCHES, None)) as tr:
            tr.set_places(NL - 1)
            out = []
            for n, entry in enumerate(TA.FULL):
                R, t, ev = TA.step(tr, seqs, entry)
                out.append(dict(R=R, t=t, ev=ev.copy(), stats=tr.stats(), rec=[tr.information(s) for s in range(N_S)],
                                sig=[tr.signals(s) for s in range(N_S) if ev[s] != 1], keys=[tr.key_frame_id(s) for s in range(N_S)],
                                places=tr.places(list(range(N_S)), 2), archive=tr.archive_stats()))
                if probe:
                    cand = [(s, tr.key_frame_id((s + n) % N_S)) for s in range(N_S)]
                    for level in range(NL):
                        recs = tr.verify([c[0] for c in cand], [c[1] for c in cand], level, R, t)
                        st = tr.archive_stats()
                        assert (st["last_launches"], st["last_syncs"]) == (1, 1), (n, st)
                        assert all(r["n_points"] > 64 for r in recs)
                    assert tr.stats() == out[-1]["stats"]
            return out
    with_verify, without = run(True), run(False)
    for n, (a, b) in enumerate(zip(with_verify, without)):
        assert TA.same_bits(a["R"], b["R"]) and TA.same_bits(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"] and a["stats"] == b["stats"] and a["keys"] == b["keys"] and a["places"] == b["places"], n
        assert all(TI.same_record(x, y) for x, y in zip(a["rec"], b["rec"])), n
        assert a["archive"] == b["archive"], n                    # ... last_launches / last_syncs of the query included


def test_contract(seqs):  # noqa: F811
    from rgbd_odometry_amd import capi
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE
    eye, zero = EYE[None], ZERO[None]
    with TA.make(4, archive=None) as tr:
        TA.refused(DVO_ERR_STATE, tr.verify, [0], [0], 0, eye, zero)                # archive off
        tr.set_stream_intrinsics(1, 250.0, 254.0, 161.0, 118.0)
        tr.set_archive(4, 2)
        TA.refused(DVO_ERR_STATE, tr.verify, [0], [0], 0, eye, zero)                # never stepped
        TA.step(tr, seqs, [(s, 0) for s in range(3)])                               # stream 3 stays at its start
        ids = [tr.key_frame_id(s) for s in range(3)]
        assert ids == [0, 1, 2]

        def state():
            return (tr.archive_stats(), tr.stats(), [tr.key_frame_id(s) for s in range(3)], [tr.archive_points(k, 0).tobytes() for k in ids])

        def call(s, k, level=0, **tol):
            return tr.verify(s, k, level, np.tile(EYE, (len(s), 1, 1)), np.zeros((len(s), 3)), **tol)

        ok = call([2, 0], [ids[0], ids[2]])                                         # another stream's key frame, same model
        assert all(r["n_depth"] > 64 for r in ok)
        before = state()
        TA.refused(DVO_ERR_INVALID, call, [], [])                                   # n outside [1, max_matches]
        TA.refused(DVO_ERR_INVALID, call, [0, 0, 0], [ids[0]] * 3)
        TA.refused(DVO_ERR_INVALID, call, [4], [ids[0]])                            # stream outside range
        TA.refused(DVO_ERR_INVALID, call, [-1], [ids[0]])
        TA.refused(DVO_ERR_INVALID, call, [0], [ids[0]], NL)                        # level outside the tracker's
        TA.refused(DVO_ERR_INVALID, call, [0], [ids[0]], -1)
        TA.refused(DVO_ERR_INVALID, call, [1], [ids[0]])                            # camera models differ
        TA.refused(DVO_ERR_INVALID, call, [0], [ids[1]])
        for bad in (dict(tol_mm=-1.0), dict(tol_rel=-0.5), dict(min_depth_mm=5.0, max_depth_mm=5.0), dict(min_depth_mm=9.0, max_depth_mm=2.0),
                    dict(tol_mm=np.nan), dict(tol_rel=np.nan), dict(min_depth_mm=np.nan), dict(max_depth_mm=np.nan)):
            TA.refused(DVO_ERR_INVALID, call, [0], [ids[0]], **bad)
        TA.refused(DVO_ERR_STATE, call, [3], [ids[0]])                              # never stepped
        TA.refused(DVO_ERR_STATE, call, [0], [7])                                   # unknown id
        TA.refused(DVO_ERR_STATE, call, [0], [-1])                                  # what a refused key frame's id is
        # NULL arguments, on the C function itself
        lib, h = capi.load_library(), tr._h
        S, I = (ctypes.c_int * 1)(0), (ctypes.c_longlong * 1)(ids[0])
        Rc, tc = np.ascontiguousarray(EYE), np.zeros(3)
        rec = (capi.DvoTrackerVerifyRecord * 1)()
        P = capi._ptr
        assert lib.dvo_tracker_verify(h, 1, S, I, 0, P(Rc), P(tc), None, rec) == 0 and rec[0].n_depth > 64      # vp = NULL: the defaults
        for args in ((None, I, 0, P(Rc), P(tc), None, rec), (S, None, 0, P(Rc), P(tc), None, rec), (S, I, 0, None, P(tc), None, rec),
                     (S, I, 0, P(Rc), None, None, rec), (S, I, 0, P(Rc), P(tc), None, None)):
            assert lib.dvo_tracker_verify(h, 1, *args) == DVO_ERR_INVALID, args
        assert lib.dvo_tracker_verify(None, 1, S, I, 0, P(Rc), P(tc), None, rec) == DVO_ERR_INVALID
        after = state()
        assert before == after
        # a current frame stored without a depth plane: stream 0's frame went to slot 0 (bank 0) -- put a colour-only frame there
        B = (ctypes.c_void_p * 1)(seqs[0][0][0].ctypes.data)
        assert lib.dvo_frames_upload_cameras(tr.context_handle(), 0, 1, B, None, TA.ROWS, TA.COLS, NL, SHIFT, -1, 0) == 0
        TA.refused(DVO_ERR_STATE, call, [0], [ids[0]])
        assert call([2], [ids[0]])[0] == ok[0]                                      # the other streams' frames are what they were
        tr.set_archive(0)                                                           # off again
        TA.refused(DVO_ERR_STATE, call, [2], [ids[0]])
    # evicted and refused ids
    with TA.make(1, archive=(2, 1, None), every=2) as tr:
        got = []
        for n in range(5):
            _, _, ev = TA.step(tr, seqs, [(0, n)])
            if ev[0]:
                got.append(tr.key_frame_id(0))
        assert len(got) >= 3
        TA.refused(DVO_ERR_STATE, tr.verify, [0], [got[0]], 0, eye, zero)           # evicted
        assert tr.verify([0], [got[-1]], 0, eye, zero)[0]["n_points"] > 64
    with TA.make(1, archive=(4, 1, [16, 16, 16])) as tr:
        TA.step(tr, seqs, [(0, 0)])
        assert tr.key_frame_id(0) == -1 and tr.archive_stats()["refused"] == 1
        TA.refused(DVO_ERR_STATE, tr.verify, [0], [0], 0, eye, zero)                # refused: the id was never given
