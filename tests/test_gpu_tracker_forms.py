"""Pose information, score and match of the multi-stream tracker (dvo_tracker_info.h, dvo_tracker_archive.hip, dvo_tracker_match of
dvo_capi_tracker.cpp) on every form a now level takes, away from the world the other tracker tests stand on (240 x 320 natural
frames, complete compact forms, poses at convergence):

the wide world (tests/tracker_forms.py) -- 50 x 1282 frames whose level 0 takes a PARTIAL compact form with real 16-byte texels (the
texel branch of info_accumulate, the texel copy of archive_load_kernel) and whose level 1 (25 x 641) takes a COMPLETE one, both with
an incomplete last tile row and column group; the same in a tracker that keeps 16-byte texels everywhere (engine_variant = 4);

a pose sweep from the identity to a pose where nothing is visible, with reprojections on all four borders of the level;

match guesses far from the answer, where the alignment itself reads the pixels a partial form leaves to the texels;

reference lists shorter than one wave (the square: 92, 44 and 20 points);

and all of it again on sparse texel slabs (DVO_TEX_SLAB=sparse in a child process).

Expected values: the CPU oracle's accumulators (oracle_lib.accumulate) on the resident or archived points and dvo_get_now_level of
the stream at the pose in question -- n_visible, n_points, level and sum_eps2 equal, H and g within rtol 1e-12 and atol 1e-12
max|want| (tests/test_gpu_parity.py::test_normal_matrix_of_every_iterate), an all-zero record exactly zero.  A match: bit for bit
the pose of a one-pair context fed the same two camera frames, and within the project's bounds of the oracle's alignment from the
same data (rotation 1e-5, translation 1e-4: tests/test_gpu_capacity.py)."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import test_gpu_tracker_archive as TA
import test_gpu_tracker_information as TI
import test_gpu_tracker_views as TV
import tracker_forms as F
from oracle_lib import rot_angle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = TI.ENGINE
EVEN = dict(rows=TI.ROWS, cols=TI.COLS, nl=TI.NL, shift=TI.SHIFT)
GUESS_R = np.stack([TA.rodrigues((0.004, -0.003, 0.002)), TA.rodrigues((-0.002, 0.005, 0.001))])      # of TA's match from a guess
GUESS_T = np.array([[0.004, -0.002, 0.003], [-0.003, 0.001, 0.002]])
# measured on an MI355X: the tests of this file take 3 s in the parent; the child as a whole (interpreter, imports, the same tests)
# 5.7 s.  About three times that
CHILD_TIMEOUT = 20


def make_tracker(n, geom, K, iters, every=5, archive=(4, 2, None), **engine):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in dict(ENGINE, **engine).items():
        setattr(p, k, v)
    tr = DvoTracker(n, params=p, iters=iters, rows=geom["rows"], cols=geom["cols"], n_levels=geom["nl"], first_shift=geom["shift"],
                    key_frame_every=every)
    tr.set_intrinsics(*K)
    tr.set_information(True)
    tr.set_archive(*archive)
    tr.geom, tr.K, tr.iters = geom, K, list(iters)
    tr.last_level = min(l for l in range(geom["nl"]) if iters[l] > 0)
    return tr


def now_level(tr, stream, level):
    g = tr.geom
    return TI.resident(tr, stream, level, g["rows"], g["cols"], g["shift"])[1:]


def check_record(oracle, tr, xyz, now, level, R, t, rec, what):
    """rec (an information or a score record) against the oracle's accumulators of the points xyz and the now level (dt, gx, gy) at
    (R, t), at any visible count; returns the visible count"""
    rows, cols = F.level_dims(tr.geom, level)
    want = oracle.accumulate(level, xyz, 0, len(xyz), now[0], now[1], now[2], rows, cols, tr.K, R, t)
    H = np.zeros((6, 6)); k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = want[k]; k += 1
    g = want[21:27]
    rel = lambda got, w: np.abs(got - w).max() / np.abs(w).max() if np.abs(w).max() > 0 else np.abs(got).max()
    print(what, "N", len(xyz), "visible", rec["n_visible"], int(want[28]), "sum_eps2", rec["sum_eps2"], want[27],
          "max rel dH %.3g" % rel(rec["H"], H), "max rel dg %.3g" % rel(rec["g"], g))
    if "level" in rec:
        assert rec["level"] == level, what
    if "n_points" in rec:
        assert rec["n_points"] == len(xyz), what
    assert rec["n_visible"] == int(want[28]), (what, rec["n_visible"], int(want[28]))
    assert rec["sum_eps2"] == want[27], (what, rec["sum_eps2"], want[27])
    np.testing.assert_allclose(rec["H"], H, rtol=1e-12, atol=1e-12 * np.abs(H).max(), err_msg=str(what))
    np.testing.assert_allclose(rec["g"], g, rtol=1e-12, atol=1e-12 * np.abs(g).max(), err_msg=str(what))
    if not want.any():
        assert rec["n_visible"] == 0 and rec["sum_eps2"] == 0.0 and not rec["H"].any() and not rec["g"].any(), (what, rec)
    return rec["n_visible"]


def same_record(a, b):
    return a.keys() == b.keys() and all(TA.same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def state(tr, n_streams):
    return [(tr.information(s), tr.signals(s), tr.key_frame_id(s)) for s in range(n_streams)]


def track(tr, seqs, oracle):
    """every stream's sequence, one frame per tick; every record after a stream's first frame against the oracle at the pose its step
    returned.  Returns (ticks, ids): ticks[n] = dict(R, t, ev, rec={stream: record}), ids[(tick, stream)] = id of the key frame made"""
    g, ticks, ids = tr.geom, [], {}
    streams = list(range(len(seqs)))
    for n in range(len(seqs[0])):
        R, t, ev = tr.step(streams, [seqs[s][n][0] for s in streams], [seqs[s][n][1] for s in streams])
        out = dict(R=R, t=t, ev=ev.copy(), rec={})
        for s in streams:
            rec = out["rec"][s] = tr.information(s)
            if ev[s] == 1:
                TI.assert_zero_record(rec, (n, s))
            else:
                xyz, dt, gx, gy = TI.resident(tr, s, tr.last_level, g["rows"], g["cols"], g["shift"])
                check_record(oracle, tr, xyz, (dt, gx, gy), tr.last_level, R[s], t[s], rec, ("tick", n, "stream", s, "event", int(ev[s])))
            if ev[s] != 0:
                ids[(n, s)] = tr.key_frame_id(s)
                assert ids[(n, s)] >= 0, (n, s)
        ticks.append(out)
    return ticks, ids


def forms(tr, n_streams):
    """[level][stream] = (palette size or refusal code, partial, texel mode of the last alignment)"""
    return [[TV.now_form(tr, s, l) for s in range(n_streams)] for l in range(tr.geom["nl"])]


def assert_wide_forms(tr, texel):
    f = forms(tr, 2)
    print("now forms per level and stream", f, "texel-resident" if texel else "default")
    for l in range(2):
        if texel:                                                    # as test_both_resident_forms of the views
            assert tr.iters[l] == 0 or all(x[0] <= 0 and not x[1] and x[2] != 2 for x in f[l]), f
        else:
            assert all(x[0] > 0 and x[1] == (l == 0) for x in f[l]), f      # level 0: partial; level 1: complete


def score_sweep(tr, oracle, stream, kids, level, seed):
    """every pose of the sweep for every candidate (stream, kid): alone against the oracle, then all of them again in calls of two in
    shuffled order, bit for bit.  Returns the records alone, {(kid, pose name): record}"""
    rows, cols = F.level_dims(tr.geom, level)
    now = now_level(tr, stream, level)
    items, alone, seen = [], {}, []
    for kid in kids:
        xyz = tr.archive_points(kid, level)
        poses, report = F.sweep(oracle, level, xyz, now, rows, cols, tr.K)
        a, b, c = F.conditions(poses, report, len(xyz))
        assert a and b and c, ("the sweep's conditions", level, kid, a, b, c, report)
        for name, R, t in poses:
            rec = tr.score([stream], [kid], level, R[None], t[None])[0]
            nv = check_record(oracle, tr, xyz, now, level, R, t, rec, ("level", level, "key", kid, name))
            assert nv == report[name]["visible"]
            alone[(kid, name)] = rec
            items.append((kid, name, R, t))
            seen.append(nv)
        print("level", level, "key", kid, "N", len(xyz), "visible over the sweep", seen[-len(poses):])
    order = np.random.default_rng(seed).permutation(len(items))
    order = np.append(order, order[:len(order) % 2])                 # an odd count: the first one once more
    for j in range(0, len(order), 2):
        pair = [items[order[j]], items[order[j + 1]]]
        both = tr.score([stream, stream], [p[0] for p in pair], level, np.stack([p[2] for p in pair]), np.stack([p[3] for p in pair]))
        for p, rec in zip(pair, both):
            assert same_record(alone[(p[0], p[1])], rec), (level, p[0], p[1], alone[(p[0], p[1])], rec)
    assert min(seen) == 0 and max(seen) > 6
    return alone


def check_match(tr, oracle, n_streams, cands, R0, t0):
    """cands: [(stream, key id, the key frame's camera frame, the stream's current camera frame)], matched in ONE call from (R0, t0)"""
    from rgbd_odometry_amd import DvoContext
    g, nl = tr.geom, tr.geom["nl"]
    before = state(tr, n_streams)
    Rm, tm, recs = tr.match([c[0] for c in cands], [c[1] for c in cands], R0, t0)
    for i, (s, kid, key_frame, now_frame) in enumerate(cands):
        with DvoContext(1, **ENGINE) as ctx:
            ctx.set_intrinsics(*tr.K)
            ctx.frames_upload_cameras([key_frame[0]], [key_frame[1]], n_levels=nl, first_shift=g["shift"], first_slot=0)
            ctx.frames_as_ref(0, 0, 1)
            ctx.frames_upload_cameras([now_frame[0]], [now_frame[1]], n_levels=nl, first_shift=g["shift"], first_slot=1)
            ctx.frames_as_now(1, 0, 1)
            R, t = ctx.align_batch(tr.iters, R0[i][None].copy(), t0[i][None].copy())
        levels = []
        for l in range(nl):
            rows, cols = F.level_dims(g, l)
            dt, gx, gy = now_level(tr, s, l)
            levels.append(dict(xyz=tr.archive_points(kid, l), dt=dt, gx=gx, gy=gy, rows=rows, cols=cols))
        ref = oracle.align_pyramid(tr.iters, levels, tr.K, R0[i], t0[i])
        dR, dt_ = rot_angle(ref["R"], Rm[i]), np.linalg.norm(ref["t"] - tm[i])
        print("match", i, "stream", s, "key", kid, "t", tm[i], "against the oracle: rotation %.3g translation %.3g" % (dR, dt_))
        assert TA.same_bits(Rm[i], R[0]) and TA.same_bits(tm[i], t[0]), (i, Rm[i], R[0], tm[i], t[0])
        L = levels[tr.last_level]
        check_record(oracle, tr, L["xyz"], (L["dt"], L["gx"], L["gy"]), tr.last_level, Rm[i], tm[i], recs[i], ("match", i))
        assert dR <= 1e-5 and dt_ <= 1e-4, (i, dR, dt_)
    for a, b in zip(before, state(tr, n_streams)):
        assert TI.same_record(a[0], b[0]) and a[1:] == b[1:]
    return Rm, tm, recs


# ---- the wide world ----
@pytest.fixture(scope="module")
def wide_seqs():
    return F.wide_sequences()


def wide_run(seqs, oracle, iters, texel):
    tr = make_tracker(2, F.WIDE, F.WIDE_K, iters, every=2, **(dict(engine_variant=4) if texel else {}))
    ticks, ids = track(tr, seqs, oracle)
    assert [x["ev"].tolist() for x in ticks] == [[1, 1], [0, 0], [5, 5]]
    assert sorted(ids) == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert_wide_forms(tr, texel)
    return tr, ticks, ids


@pytest.fixture(scope="module")
def wide(wide_seqs, oracle):
    """the default tracker and the texel-resident one after the three ticks at iters = [8, 8], left open for score and match"""
    a, b = wide_run(wide_seqs, oracle, [8, 8], False), wide_run(wide_seqs, oracle, [8, 8], True)
    yield a, b
    a[0].close(); b[0].close()


def assert_same_ticks(a, b):
    for n, (x, y) in enumerate(zip(a, b)):
        assert TA.same_bits(x["R"], y["R"]) and TA.same_bits(x["t"], y["t"]) and np.array_equal(x["ev"], y["ev"]), n
        assert all(same_record(x["rec"][s], y["rec"][s]) for s in x["rec"]), (n, x["rec"], y["rec"])


def test_wide_information_on_the_partial_level(wide):
    """level 0, 50 x 1282: track() held every record against the oracle, in both trackers -- the texel branch of info_accumulate for a
    partial form and for a context without compact forms"""
    (tr, ticks, ids), (tx, tticks, tids) = wide
    assert all(r["level"] == 0 for x in ticks[1:] for r in x["rec"].values())
    n = [len(TI.resident(tr, s, 0, 50, 1282, 0)[0]) for s in (0, 1)]
    assert all(64 < k < 512 for k in n), n
    assert ids == tids
    assert_same_ticks(ticks, tticks)


def test_wide_information_on_the_complete_level(wide_seqs, oracle):
    """iters = [0, 8]: the record is taken on level 1, 25 x 641, the compact branch with an incomplete last tile row and column group"""
    runs = []
    for texel in (False, True):
        tr, ticks, ids = wide_run(wide_seqs, oracle, [0, 8], texel)
        with tr:
            assert all(r["level"] == 1 for x in ticks[1:] for r in x["rec"].values())
            assert all(64 < len(TI.resident(tr, s, 1, 50, 1282, 0)[0]) < 512 for s in (0, 1))
        runs.append(ticks)
    assert_same_ticks(*runs)


@pytest.mark.parametrize("level", [0, 1])
def test_wide_score_over_the_pose_sweep(wide, oracle, level):
    """stream 0's current frame against its own first key frame and against stream 1's current key frame"""
    (tr, _, ids), (tx, _, _) = wide
    kids = [ids[(0, 0)], ids[(2, 1)]]
    a = score_sweep(tr, oracle, 0, kids, level, seed=level)
    b = score_sweep(tx, oracle, 0, kids, level, seed=level + 7)
    assert a.keys() == b.keys() and all(same_record(a[k], b[k]) for k in a)


@pytest.mark.parametrize("start", ["identity", "guess"])
def test_wide_match(wide, wide_seqs, oracle, start):
    """two candidates in one call: stream 0 against its own first key frame, stream 1 against stream 0's current key frame; both the
    partial level 0 and the complete level 1 travel through archive_load_kernel"""
    (tr, _, ids), (tx, _, _) = wide
    cands = [(0, ids[(0, 0)], wide_seqs[0][0], wide_seqs[0][2]), (1, ids[(2, 0)], wide_seqs[0][1], wide_seqs[1][2])]
    R0, t0 = (np.stack([np.eye(3)] * 2), np.zeros((2, 3))) if start == "identity" else (GUESS_R, GUESS_T)
    a = check_match(tr, oracle, 2, cands, R0, t0)
    b = check_match(tx, oracle, 2, cands, R0, t0)
    assert TA.same_bits(a[0], b[0]) and TA.same_bits(a[1], b[1]) and all(same_record(x, y) for x, y in zip(a[2], b[2]))


def test_wide_match_reads_unranked_pixels(wide_seqs, oracle):
    """iters = [8, 0]: level 0 alone, from guesses that put the points on the flat wall, where the partial form holds no rank and the
    alignment kernel falls back to the level's 16-byte texels -- the texels archive_load_kernel copied, found through the palette's NaN
    entry it copied (it once left that entry behind: no fall-back, a pose 5e-3 rad and 2e-2 m off the oracle's)"""
    R0, t0 = F.far_guesses()
    out = []
    for texel in (False, True):
        tr, _, ids = wide_run(wide_seqs, oracle, [8, 0], texel)
        with tr:
            cands = [(0, ids[(0, 0)], wide_seqs[0][0], wide_seqs[0][2]), (1, ids[(2, 0)], wide_seqs[0][1], wide_seqs[1][2])]
            hits = [F.unranked_hits(oracle, 0, tr.archive_points(kid, 0), now_level(tr, s, 0), 50, 1282, F.WIDE_K, R, t)
                    for (s, kid, _, _), R, t in zip(cands, R0, t0)]
            print("points on unranked pixels at the guesses", hits)
            assert all(h >= 32 for h in hits), hits
            out.append(check_match(tr, oracle, 2, cands, R0, t0))
    a, b = out
    assert TA.same_bits(a[0], b[0]) and TA.same_bits(a[1], b[1]) and all(same_record(x, y) for x, y in zip(a[2], b[2]))


# ---- the pose sweep on complete forms at even geometry ----
@pytest.fixture(scope="module")
def even():
    """240 x 320: the 7-tick run of tests/test_gpu_tracker_archive.py, left open"""
    seqs = [TI.sequence(900 + s, TA.N_T, TI.MOTIONS[s]) for s in range(TA.N_S)]
    with TA.make(TA.N_S) as tr:
        _, ids = TA.run(tr, seqs, archive=True)
        tr.geom, tr.K = EVEN, TI.K
        yield tr, ids


@pytest.mark.parametrize("level", [0, 2])
def test_even_geometry_score_over_the_pose_sweep(even, oracle, level):
    """stream 0's last frame against its key frames of tick 0 and tick 5, on complete compact forms"""
    tr, ids = even
    f = [TV.now_form(tr, 0, l) for l in range(3)]
    print("now forms of stream 0 per level", f)
    assert all(x[0] > 0 and not x[1] for x in f), f
    score_sweep(tr, oracle, 0, [ids[(0, 0)], ids[(5, 0)]], level, seed=level)


# ---- short lists ----
@pytest.mark.parametrize("iters,level", [([0, 0, 8], 2), ([0, 8, 8], 1)])
def test_short_lists(oracle, iters, level):
    """the square: 92, 44 and 20 reference points -- at level 2 less than one wave, every lane's points u = 1..3 of the walk invalid"""
    seq = F.square_sequence()
    with make_tracker(1, F.SQUARE, F.SQUARE_K, iters) as tr:
        ticks, ids = track(tr, [seq], oracle)
        assert [x["ev"].tolist() for x in ticks] == [[1], [0], [0]] and tr.last_level == level
        assert all(x["rec"][0]["level"] == level for x in ticks[1:])
        kid = ids[(0, 0)]
        n = [len(tr.archive_points(kid, l)) for l in range(3)]
        print("square: points per level", n, "now forms", forms(tr, 1), "visible", [x["rec"][0]["n_visible"] for x in ticks[1:]])
        assert n == list(F.SQUARE_N) and 6 < n[2] < 64
        poses = [F.fixed_sweep()[0], F.ALL_INVISIBLE]
        for l in sorted({level, 2}):
            xyz, now = tr.archive_points(kid, l), now_level(tr, 0, l)
            alone = [tr.score([0], [kid], l, R[None], t[None])[0] for _, R, t in poses]
            seen = [check_record(oracle, tr, xyz, now, l, R, t, rec, ("square level", l, name)) for (name, R, t), rec in zip(poses, alone)]
            assert seen[0] > 6 and seen[1] == 0, seen
            both = tr.score([0, 0], [kid, kid], l, np.stack([poses[1][1], poses[0][1]]), np.stack([poses[1][2], poses[0][2]]))
            assert same_record(both[0], alone[1]) and same_record(both[1], alone[0])
        for R0, t0 in ((np.eye(3)[None], np.zeros((1, 3))), (GUESS_R[:1], GUESS_T[:1])):
            check_match(tr, oracle, 1, [(0, kid, seq[0], seq[2])], R0, t0)


# ---- sparse texel slabs ----
def test_this_file_on_sparse_texel_slabs():
    """every test above again with DVO_TEX_SLAB=sparse (the tracker's, the match context's and the one-pair contexts' texel slabs
    sparse): match maps the destination's texels for real forms and for forms the host has not looked at (map_texels, the `unknown`
    bit), and the load kernel copies only what is backed -- in a child process, because the policy is read once per process"""
    env = dict(os.environ, DVO_TEX_SLAB="sparse")
    me = "tests/test_gpu_tracker_forms.py"
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", me, "--deselect", me + "::test_this_file_on_sparse_texel_slabs",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print("the child took %.1f s: %s" % (time.time() - t0, r.stdout.strip().splitlines()[-1:] or r.stderr[-300:]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
