"""Multi-stream tracker on the GPU (include/dvo_amd.h, "many camera streams"): every stream's trajectory -- relative poses, key-frame
events and reasons, the adaptive signals -- must be bit-identical to the single-stream path (the sequence of engine calls
dvo_amd::SolveDVO::processFirstFrame / processFrame makes, on a one-pair context) run on that stream's frames alone."""
import os
import signal
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import frame_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tracker_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 240, 320, 3, 0
ITERS = [8, 8, 8]
K = (262.5, 262.5, 159.75, 119.75)
# One launch shape on both sides: the poses come from double sums whose order follows the workgroup size and team size, which the
# engine otherwise picks from the batch size (float32 per-point quantities and energies are identical under any shape).  camera_frame
# keeps a 16-pixel margin: |motion| * (frames - 1) <= 16 keeps every frame at the full size.
ENGINE = dict(block_threads=512, team_size=1)


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


def single_stream(frames, adaptive=None, every=5, params=None):
    """the engine calls of dvo_amd::SolveDVO::processFirstFrame / processFrame for one camera: [(R, t, event, signals)] per frame;
    params: dvo_params fields other than the defaults (the update's parameters, tests/test_gpu_update_params.py)"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    last = min(l for l in range(NL) if ITERS[l] > 0)
    out = []
    with DvoContext(1, **ENGINE, **(params or {})) as ctx:
        ctx.set_intrinsics(*K)
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
            R, t = ctx.align_batch(ITERS, cR[None].copy(), cT[None].copy(), flags=DVO_FLAG_FINAL_OUTPUTS if adaptive else 0)
            cR, cT = R[0], t[0]
            sig, reason, signals = False, 0, None
            if adaptive:
                _, _, ratio = ctx.level_report(0, last, ITERS[last])
                eps, _ = ctx.final_outputs(0, ctx.n_points(last, 0))
                b, ratio, npts = T.laplacian_b(eps), np.float32(ratio), len(eps)
                signals = (b, ratio, npts)
                if b > np.float32(adaptive["laplacian_b"]):
                    sig, reason = True, 2
                if ratio < np.float32(adaptive["visible_ratio"]):
                    sig, reason = True, 3
                if npts < adaptive["min_points"]:
                    sig, reason = True, 4
            if n - last_ref == every:
                sig, reason = True, 5
            event = 0
            if sig and last_ref != n - 1:
                last_ref = n - 1
                ref_slot = prev_slot
                ctx.frames_as_ref(prev_slot, 0, 1)
                R, t = ctx.align_batch(ITERS, np.eye(3)[None], np.zeros((1, 3)))
                cR, cT = R[0], t[0]
                event = reason
            out.append((cR.copy(), cT.copy(), event, signals))
    return out


def make_tracker(n, adaptive=None, params=None, **kw):
    import ctypes
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in dict(ENGINE, **(params or {})).items():
        setattr(p, k, v)
    a = adaptive or {}
    tr = DvoTracker(n, params=p, iters=ITERS, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, adaptive=adaptive is not None,
                    laplacian_b_thresh=a.get("laplacian_b", 3.0), visible_ratio_thresh=a.get("visible_ratio", 0.8),
                    min_points=a.get("min_points", 50), **kw)
    tr.set_intrinsics(*K)
    return tr


def gop_lines(traj):
    """GOP chain + printPose lines of one stream (dvo_amd::SolveDVOStreams::compose == SolveDVO's GOP calls)"""
    g, lines = T.GOP(), []
    for n, (R, t, ev, _) in enumerate(traj):
        if ev == 1:
            g = T.GOP()
            g.push_key(n, 1, R, t)
            continue
        if ev >= 2:
            g.update_most_recent_to_key(ev)
        g.push_ordinary(n, R, t)
        lines.append(T.pose_line(g.elems[-1]["R"], g.elems[-1]["t"]))
    return g, lines


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for n, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (what, n, "event", g[2], w[2])
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (what, n, "pose", g[0], w[0], g[1], w[1])
        if w[3] is not None:
            assert g[3][0] == w[3][0] and g[3][1] == w[3][1] and g[3][2] == w[3][2], (what, n, "signals", g[3], w[3])


def run_tracker(tr, seqs, schedule, adaptive=False):
    """schedule: per tick the list of (stream, frame index into seqs[stream]) to step; returns per stream [(R, t, event, signals)]"""
    got = {s: [] for s in range(len(seqs))}
    for tick in schedule:
        streams = [s for s, _ in tick]
        R, t, ev = tr.step(streams, [seqs[s][i][0] for s, i in tick], [seqs[s][i][1] for s, i in tick])
        for k, s in enumerate(streams):
            sig = tr.signals(s) if (adaptive and ev[k] != 1) else None
            got[s].append((R[k], t[k], int(ev[k]), sig))
    return got


MOTIONS = [(0.5, -1.0), (1.0, 0.5), (-0.5, 1.5), (1.5, -0.5), (0.0, 1.4), (-1.0, -1.0)]


def test_default_policy_six_streams(oracle):
    with time_limit(600):
        seqs = [sequence(100 + s, 11, MOTIONS[s]) for s in range(6)]
        want = [single_stream(q) for q in seqs]
        with make_tracker(6) as tr:
            got = run_tracker(tr, seqs, [[(s, n) for s in range(6)] for n in range(11)])
        for s in range(6):
            assert_same(got[s], want[s], "stream %d" % s)
            assert [w[2] for w in want[s]] == [1, 0, 0, 0, 0, 5, 0, 0, 0, 5, 0]
            gg, gl = gop_lines(got[s])
            wg, wl = gop_lines(want[s])
            assert gl == wl and all(np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) for a, b in zip(gg.elems, wg.elems))
        # stream 0 against the oracle chain (the C oracle as the aligner, as tests/test_tracker.py does)
        pyr = [oracle.build_pyramid(b, d, NL, SHIFT) for b, d in seqs[0]]
        Kf = tuple(np.float32(k) for k in K)
        cache = {}

        def align(ref, now, R0, t0):
            if ("r", ref) not in cache:
                cache[("r", ref)] = [oracle.ref_level_from_grey(l, g, d, Kf) for l, (g, d) in enumerate(pyr[ref])]
            if ("n", now) not in cache:
                cache[("n", now)] = [oracle.now_level_from_grey(g) for g, _ in pyr[now]]
            lv = [dict(xyz=r[0], uv=r[1], dt=m[0], gx=m[1], gy=m[2], rows=g.shape[0], cols=g.shape[1])
                  for r, m, (g, _) in zip(cache[("r", ref)], cache[("n", now)], pyr[now])]
            r = oracle.align_pyramid(ITERS, lv, Kf, R0, t0)
            return np.array(r["R"]), np.array(r["t"])

        _, want_lines = T.track(11, align)
        G = np.array([[float(x) for x in ln.split()] for ln in gop_lines(got[0])[1]])
        W = np.array([[float(x) for x in ln.split()] for ln in want_lines])
        assert np.abs(G - W).max() <= 2e-5


def test_adaptive_exits():
    with time_limit(900):
        motions = [(0.5, -1.0), (1.5, 1.5), (-0.5, 1.5), (1.5, -1.5), (0.0, 1.5), (-1.0, -1.0)]
        seqs = [sequence(200 + s, 11, motions[s]) for s in range(6)]
        # thresholds placed among the values the sequences produce (a first pass that never switches for them)
        probe = [single_stream(q, adaptive=dict(laplacian_b=1e30, visible_ratio=-1.0, min_points=-1)) for q in seqs]
        sig = [w[3] for p in probe for w in p if w[3] is not None]
        b = np.array([x[0] for x in sig]); r = np.array([x[1] for x in sig]); npts = np.array([x[2] for x in sig])
        adaptive = dict(laplacian_b=float(np.percentile(b, 60)), visible_ratio=float(np.percentile(r, 15)),
                        min_points=int(np.percentile(npts, 25)))
        want = [single_stream(q, adaptive=adaptive) for q in seqs]
        with make_tracker(6, adaptive=adaptive) as tr:
            got = run_tracker(tr, seqs, [[(s, n) for s in range(6)] for n in range(11)], adaptive=True)
        for s in range(6):
            assert_same(got[s], want[s], "stream %d" % s)
        reasons = {w[2] for q in want for w in q}
        ticks = {tuple(n for n, w in enumerate(q) if w[2] >= 2) for q in want}
        print("adaptive thresholds", adaptive, "reasons", sorted(reasons), "switch ticks", ticks)
        assert {2, 3, 4} <= reasons, (adaptive, [[w[2] for w in q] for q in want])
        assert len(ticks) > 1                                # streams switch on different ticks


def test_subset_steps():
    with time_limit(600):
        seqs = [sequence(300 + s, 11, MOTIONS[s]) for s in range(6)]
        pos = [0] * 6
        schedule, received = [], [[] for _ in range(6)]
        for tick in range(10):
            if tick == 7:
                received[2].append("reset")
            # stream 3 skips ONE tick: from then on its frames sit in the other bank than its neighbours' (two upload runs per tick)
            live = [s for s in range(6) if not (s >= 4 and tick < 3) and not (s == 1 and tick in (5, 6)) and not (s == 3 and tick == 4)]
            entry = []
            for s in live:
                entry.append((s, pos[s]))
                received[s].append(pos[s])
                pos[s] += 1
            schedule.append((tick, entry))
        split_banks = 0
        with make_tracker(6) as tr:
            got = {s: [] for s in range(6)}
            for tick, entry in schedule:
                if tick == 7:
                    tr.reset_stream(2)
                streams = [s for s, _ in entry]
                R, t, ev = tr.step(streams, [seqs[s][i][0] for s, i in entry], [seqs[s][i][1] for s, i in entry])
                st = tr.stats()
                assert st["launches"] > 0, st
                # uploads (one per run of consecutive listed streams), first frames' extraction, alignment, switches (extraction + re-run)
                consecutive = 1 + sum(b != a + 1 for a, b in zip(streams, streams[1:]))
                expected_runs = consecutive + int(1 in ev) + int(any(e != 1 for e in ev)) + (2 if st["key_frames"] else 0)
                extra = st["runs"] - expected_runs                 # runs split because stream 3 writes the other bank
                assert 0 <= extra <= 2 and (extra == 0 or 3 in streams), (tick, st, ev)
                split_banks += extra > 0
                for k, s in enumerate(streams):
                    got[s].append((R[k], t[k], int(ev[k]), None))
        assert split_banks > 0
        for s in range(6):
            parts, cur = [], []
            for x in received[s]:
                if x == "reset":
                    parts.append(cur); cur = []
                else:
                    cur.append(x)
            parts.append(cur)
            want = []
            for part in parts:
                want += single_stream([seqs[s][i] for i in part])
            assert_same(got[s], want, "stream %d" % s)
        assert got[2][7][2] == 1 and got[4][0][2] == 1


def _device_frames(seqs):
    import torch
    return [[(torch.from_numpy(b).cuda(), torch.from_numpy(d).cuda()) for b, d in q] for q in seqs]


def _step_device(tr, streams, dev, n):
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE
    return tr.step(streams, [dev[s][n][0].data_ptr() for s in streams], [dev[s][n][1].data_ptr() for s in streams], flags=DVO_UPLOAD_DEVICE)


def test_scale_256_streams_and_launch_counts():
    with time_limit(1500):
        n_s, n_t = 256, 6
        seqs = [sequence(1000 + s, n_t, ((s % 7) * 0.5 - 1.5, (s % 5) * 0.5 - 1.0)) for s in range(n_s)]
        dev = _device_frames(seqs)
        stats = {}
        for k in (8, n_s):
            with make_tracker(k, points_capacity=[20000, 8000, 3000]) as tr:
                got, st = [[] for _ in range(k)], []
                for n in range(n_t):
                    R, t, ev = _step_device(tr, list(range(k)), dev, n)
                    st.append(tr.stats())
                    for s in range(k):
                        got[s].append((R[s], t[s], int(ev[s]), None))
            stats[k] = st
        for s in range(n_s):
            assert_same(got[s], single_stream(seqs[s]), "stream %d" % s)
        for k in (8, n_s):
            st = stats[k]
            print(k, st)
            assert all(x["launches"] > 0 for x in st), st
            for n in (1, 2, 3, 4):                           # ordinary full ticks
                assert st[n]["syncs"] == 1 and st[n]["runs"] == 2 and st[n]["key_frames"] == 0, (k, n, st[n])
            assert st[5]["key_frames"] == k and st[5]["runs"] == 4, st[5]      # upload, align, reference extraction, ONE re-run
            assert all(x["slab_growths"] == 0 for x in st[1:]), st
        for n in range(1, n_t):
            assert stats[8][n]["launches"] == stats[n_s][n]["launches"], (n, stats[8][n], stats[n_s][n])
        # the key-frame tick adds reference extraction + one alignment launch + reset / gather, the same at K = 8 and 256
        assert stats[n_s][5]["launches"] - stats[n_s][4]["launches"] == stats[8][5]["launches"] - stats[8][4]["launches"]


def test_fragmented_sets_one_launch_sequence():
    """streams 0, 2, 4 start on tick 0, streams 1, 3, 5 on tick 1: the first-frame set of tick 1 and the switching sets of ticks 5 and 6
    are not consecutive streams, yet each is ONE reference extraction and ONE re-run alignment (index-list forms)"""
    with time_limit(600):
        n_t = 8
        seqs = [sequence(600 + s, n_t, MOTIONS[s]) for s in range(6)]
        got, stats = {s: [] for s in range(6)}, []
        with make_tracker(6, points_capacity=[20000, 8000, 3000]) as tr:
            for tick in range(n_t):
                streams = [s for s in range(6) if s % 2 == 0 or tick >= 1]
                n_of = {s: tick - (s % 2) for s in streams}
                R, t, ev = tr.step(streams, [seqs[s][n_of[s]][0] for s in streams], [seqs[s][n_of[s]][1] for s in streams])
                stats.append(tr.stats())
                for k, s in enumerate(streams):
                    got[s].append((R[k], t[k], int(ev[k]), None))
        for s in range(6):
            assert_same(got[s], single_stream(seqs[s][:n_t - (s % 2)]), "stream %d" % s)
        print(stats)
        assert all(x["slab_growths"] == 0 for x in stats), stats
        assert stats[1]["runs"] == 3                                        # upload, extraction of {1, 3, 5}, alignment of {0, 2, 4}
        for tick, sw in ((5, [0, 2, 4]), (6, [1, 3, 5])):
            st = stats[tick]
            assert [e[2] for s in sw for e in got[s][tick - (s % 2):tick - (s % 2) + 1]] == [5, 5, 5]
            assert st["key_frames"] == 3 and st["runs"] == 4 and st["syncs"] == 3, (tick, st)   # one extraction, one re-run
        # the same launches as a tick whose switching set is contiguous would take: nothing per stream
        assert stats[5]["launches"] == stats[6]["launches"] > stats[4]["launches"] > 0


DEMO_N, DEMO_NL, DEMO_IT = 11, 3, 8


def demo_args(dirs, prefix):
    return ["3"] + dirs + ["0", str(DEMO_N - 1), "1", str(DEMO_NL)] + [repr(float(k)) for k in K] + [str(DEMO_IT), str(prefix)]


@pytest.fixture(scope="module")
def demo_run(tmp_path_factory, oracle):
    """three XML sequences and examples/multi_track_demo's plain run on them: dict(dirs, pyr, prefix, stdout)"""
    import subprocess
    import frame_io
    root = tmp_path_factory.mktemp("demo")
    dirs, pyr = [], []
    for s in range(3):
        d = root / ("seq%d" % s)
        d.mkdir()
        pyr.append([oracle.build_pyramid(b, dep, DEMO_NL, 0) for b, dep in sequence(700 + s, DEMO_N, MOTIONS[s])])
        for i, levels in enumerate(pyr[s]):
            frame_io.write_frame_xml(str(d / ("framemono_%04d.xml" % i)), levels)
        dirs.append(str(d))
    exe = os.path.join(ROOT, "rgbd_odometry_amd", "lib", "multi_track_demo")
    run = subprocess.run([exe] + demo_args(dirs, root / "multi_"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    return dict(dirs=dirs, pyr=pyr, prefix=root / "multi_", stdout=run.stdout, exe=exe)


def test_multi_track_demo_matches_track_demo(tmp_path, demo_run):
    """examples/multi_track_demo (dvo_amd::SolveDVOStreams: GOP<double> per stream, printPose) on three XML sequences at once writes,
    per stream, the pose file and key frames examples/track_demo (dvo_amd::SolveDVO) writes for that sequence alone"""
    import subprocess
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    n, nl, it = DEMO_N, DEMO_NL, DEMO_IT
    Ks = [repr(float(k)) for k in K]
    dirs, run = demo_run["dirs"], demo_run
    with time_limit(600):
        for s in range(3):
            one = subprocess.run([os.path.join(lib, "track_demo"), dirs[s], "0", str(n - 1), "1", str(nl)] + Ks +
                                 [str(it), str(tmp_path / ("one_%d.txt" % s))], capture_output=True, text=True, timeout=300)
            assert one.returncode == 0, one.stderr
            keys = one.stdout.split("keyframes:")[1].splitlines()[0].strip()
            assert ("stream %d frames %d keyframes: %s" % (s, n, keys)) in run["stdout"], (keys, run["stdout"])
            a = open(str(run["prefix"]) + "%d.txt" % s).read().split("\n")
            b = (tmp_path / ("one_%d.txt" % s)).read_text().split("\n")
            assert len(a) == len(b) == n                      # n - 1 pose lines, trailing newline
            A = np.array([[float(x) for x in ln.split()] for ln in a if ln])
            B = np.array([[float(x) for x in ln.split()] for ln in b if ln])
            # printPose writes 6 significant digits: the lines agree; a last-bit difference of the poses (the single-pair context may
            # pick another launch shape than the three-stream tracker, see include/dvo_amd.h) could flip the last digit only
            assert np.abs(A - B).max() <= 2e-6, (s, np.abs(A - B).max())


def test_multi_track_demo_options(tmp_path, demo_run):
    """--sigma, --places 2 and --views DIR (the only callers in the tree of SolveDVOStreams::lastInformation, lastView, enableArchive,
    enablePlaces, queryPlaces, matchKeyFrames and packCandidates) print and write what a DvoTracker driven with the same calls
    returns, and leave the pose files as they are without them"""
    import re
    import subprocess
    from rgbd_odometry_amd import DvoTracker
    from rgbd_odometry_amd.capi import DVO_VIEW_REPROJ_ON_DT, DVO_VIEW_RESIDUE_HEAT
    n, nl, pyr = DEMO_N, DEMO_NL, demo_run["pyr"]
    views = tmp_path / "views"
    views.mkdir()
    run = subprocess.run([demo_run["exe"]] + demo_args(demo_run["dirs"], tmp_path / "opt_") + ["--sigma", "--places", "2", "--views", str(views)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    for s in range(3):
        assert (tmp_path / ("opt_%d.txt" % s)).read_text() == open(str(demo_run["prefix"]) + "%d.txt" % s).read(), s
    got_places = [[int(x) for x in re.findall(r"-?\d+", ln)] + (["none"] if "place none" in ln else [])
                  for ln in run.stdout.splitlines() if " place " in ln]
    got_sigma = [ln for ln in run.stdout.splitlines() if " sigma " in ln]
    want_places, want_sigma, n_none = [], [], 0
    streams = [0, 1, 2]
    with DvoTracker(3, iters=[DEMO_IT] * nl, rows=ROWS, cols=COLS, n_levels=nl, first_shift=0) as tr:
        tr.set_information(True)
        tr.set_views(True)
        tr.set_archive(256, 3)
        tr.set_places(nl - 1)
        tr.set_intrinsics(*K)
        for i in range(n):
            _, _, ev = tr.step_pyramids(streams, [pyr[s][i] for s in streams])
            for which, name in ((DVO_VIEW_REPROJ_ON_DT, "reproj"), (DVO_VIEW_RESIDUE_HEAT, "heat")):
                ppm = (views / ("%s_%04d.ppm" % (name, i))).read_bytes()
                head = b"P6\n%d %d\n255\n" % (COLS, ROWS)
                assert ppm.startswith(head) and len(ppm) == len(head) + ROWS * COLS * 3, (name, i, ppm[:20])
                assert ppm[len(head):] == np.ascontiguousarray(tr.view(0, which)[..., ::-1]).tobytes(), (name, i)      # PPM is R G B
            found = tr.places(streams, 2, 10)
            cand = [(s, found[s][0]["key_id"]) for s in streams if found[s]]
            recs = iter(tr.match([c[0] for c in cand], [c[1] for c in cand])[2] if cand else [])
            for s in streams:
                if not found[s]:
                    want_places.append([s, i, "none"])
                    continue
                pl, r = found[s][0], next(recs)
                want_places.append([s, i, pl["key_id"], pl["stream"], pl["frame"], pl["distance"], r["n_visible"], r["n_points"]])
            for s in streams:
                if ev[s] == 1:
                    continue
                C = tr.covariance(s)
                want_sigma.append((s, i, None if C is None else np.sqrt(np.diag(C)), tr.information(s)["n_visible"]))
    print("place lines", len(got_places), "none", sum(p[-1] == "none" for p in want_places), "sigma lines", len(got_sigma))
    assert got_places == want_places
    assert len(want_places) == 3 * n and any(p[-1] != "none" for p in want_places)
    assert len(got_sigma) == len(want_sigma) == 3 * (n - 1)
    for ln, (s, i, sig, nv) in zip(got_sigma, want_sigma):
        if sig is None:
            assert ln == "stream %d frame %d sigma none (%d visible points)" % (s, i, nv), ln
            continue
        head, vals = ln.split(" sigma ")
        assert head == "stream %d frame %d" % (s, i), ln
        # %.6g rounds by up to 5e-6 relative; the tracker's own numbers are the same launches on the same data
        np.testing.assert_allclose([float(x) for x in vals.split()], sig, rtol=1e-5, atol=0, err_msg=ln)


def test_refusals_change_nothing():
    from rgbd_odometry_amd import DvoError
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    with time_limit(600):
        seqs = [sequence(400 + s, 4, MOTIONS[s]) for s in range(3)]
        want = [single_stream(q) for q in seqs]
        with make_tracker(3) as tr:
            got = {s: [] for s in range(3)}
            for n in range(4):
                bad = [([0, 3], 2), ([1, 1], 2), ([0, 1, 2, 0], 4), ([-1], 1)]
                for streams, m in bad:
                    with pytest.raises(DvoError) as ei:
                        tr.step(streams, [seqs[0][n][0]] * m, [seqs[0][n][1]] * m)
                    assert ei.value.code == DVO_ERR_INVALID
                with pytest.raises(DvoError) as ei:                   # geometry other than the tracker's
                    tr.step([0], [seqs[0][n][0][:120]], [seqs[0][n][1][:120]])
                assert ei.value.code == DVO_ERR_INVALID
                R, t, ev = tr.step([0, 1, 2], [q[n][0] for q in seqs], [q[n][1] for q in seqs])
                for s in range(3):
                    got[s].append((R[s], t[s], int(ev[s]), None))
        for s in range(3):
            assert_same(got[s], want[s], "stream %d" % s)
