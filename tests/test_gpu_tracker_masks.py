"""Per-stream ignore masks of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_stream_mask).  A rig of three streams:
stream 0 with mask A, stream 1 with none, stream 2 with mask B.  A masked trajectory must be the oracle chain's
(oracle/tracker_oracle.py, the construction of tests/test_gpu_tracker_streams.py) whose levels are built from `oracle.canny & keep`;
the unmasked stream must not notice its neighbours' masks, bit for bit; a masked stream must not notice its neighbours at all.

Tracker 96 x 128, first_shift 1, 3 levels (48x64, 24x32, 12x16), one launch shape on every side (block_threads 512, team_size 1).
Every frame of a masked stream is checked to have, at every level, an oracle edge pixel its mask drops and one it keeps."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from rgbd_odometry_amd import frame_gen
import mask_reference as mr
import oracle_lib
import views_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tracker_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT, MARGIN = 96, 128, 3, 1, 2
ITERS = [8, 8, 8]
K = (131.25, 131.25, 63.75, 47.75)           # of the first stored level (48 x 64)
ENGINE = dict(block_threads=512, team_size=1)
N_T = 8                                      # key_frame_every = 5: tick 5 is the forced switch and its re-run
SEEDS = (21, 23, 24)
MOTIONS = [(1.0, -2.0), (2.0, 1.0), (-1.0, 2.0)]      # camera pixels per frame; |motion| * (N_T - 1) <= 16, camera_frame's margin
MASK_SEED = {0: 1, 2: 2}


def cm(a_rm):
    return np.ascontiguousarray(np.asarray(a_rm).T).ravel()


@functools.lru_cache(maxsize=None)
def rig():
    """sequences, masks, keep planes, oracle pyramids and edge maps of the three streams: computed once"""
    o = oracle_lib.load()
    seqs = [[frame_gen.camera_frame(SEEDS[s], ROWS, COLS, shift=(int(round(MOTIONS[s][0] * i)), int(round(MOTIONS[s][1] * i))), holes=True)
             for i in range(N_T)] for s in range(3)]
    masks = {s: mr.scene_mask(ROWS, COLS, k) for s, k in MASK_SEED.items()}
    keep = {s: mr.keep_levels(m, NL, SHIFT, MARGIN) for s, m in masks.items()}
    pyr = [[o.build_pyramid(b, d, NL, SHIFT) for b, d in q] for q in seqs]
    canny = [[[o.canny(g) for g, _ in p] for p in q] for q in pyr]
    for s in masks:
        for i in range(N_T):
            for l in range(NL):
                e = canny[s][i][l] != 0
                assert (e & (keep[s][l] == 0)).any() and (e & (keep[s][l] != 0)).any(), (s, i, l)
    return dict(seqs=seqs, masks=masks, keep=keep, pyr=pyr, canny=canny)


def masked_edges(G, s, i, l, keep=None):
    keep = G["keep"].get(s) if keep is None else keep
    e = G["canny"][s][i][l]
    return e if keep is None else e & keep[l]


def oracle_lines(G, s, keep=None, n=N_T):
    """(gop, pose lines) of stream s by the oracle chain, its levels built from canny & keep"""
    o = oracle_lib.load()
    Kf = tuple(np.float32(k) for k in K)
    cache = {}

    def ref_levels(i):
        if ("r", i) not in cache:
            out = []
            for l, (g, d16) in enumerate(G["pyr"][s][i]):
                d = d16.astype(np.uint16).copy()
                d[d == 0] = 1
                out.append(o.enlist_ref_points(l, cm(masked_edges(G, s, i, l, keep)).astype(np.int32), cm(d).astype(np.float32), g.shape[0], g.shape[1], Kf))
            cache[("r", i)] = out
        return cache[("r", i)]

    def now_levels(i):
        if ("n", i) not in cache:
            cache[("n", i)] = [o.now_level_from_edges(cm(masked_edges(G, s, i, l, keep)), g.shape[0], g.shape[1]) for l, (g, _) in enumerate(G["pyr"][s][i])]
        return cache[("n", i)]

    def align(ref, now, R0, t0):
        lv = [dict(xyz=r[0], uv=r[1], dt=m[0], gx=m[1], gy=m[2], rows=g.shape[0], cols=g.shape[1])
              for r, m, (g, _) in zip(ref_levels(ref), now_levels(now), G["pyr"][s][now])]
        r = o.align_pyramid(ITERS, lv, Kf, R0, t0)
        return np.array(r["R"]), np.array(r["t"])

    return T.track(n, align)


def make_tracker(n, **kw):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in ENGINE.items():
        setattr(p, k, v)
    tr = DvoTracker(n, params=p, iters=ITERS, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, **kw)
    tr.set_intrinsics(*K)
    return tr


def run(tr, G, streams, n=N_T, hook=None, local=None):
    """steps the listed rig streams together for n ticks (local[s]: the tracker's stream that plays rig stream s); per rig stream
    [(R, t, event)], and the stats of every tick"""
    local = local or {s: s for s in streams}
    got, stats = {s: [] for s in streams}, []
    for i in range(n):
        if hook:
            hook(i)
        R, t, ev = tr.step([local[s] for s in streams], [G["seqs"][s][i][0] for s in streams], [G["seqs"][s][i][1] for s in streams])
        stats.append(tr.stats())
        for k, s in enumerate(streams):
            got[s].append((R[k], t[k], int(ev[k])))
    return got, stats


def gop_lines(traj):
    g, lines = T.GOP(), []
    for n, (R, t, ev) in enumerate(traj):
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


def ref_len(tr, s, l=0):
    from rgbd_odometry_amd import capi
    n = ctypes.c_int()
    assert capi.load_library().dvo_get_ref_level(tr.context_handle(), s, l, None, 0, ctypes.byref(n)) == 0
    return n.value


def stored_edge(tr, slot, l):
    """the edge map of a frame-store slot of the tracker's context, (rows_l, cols_l)"""
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    r, c = ctypes.c_int(), ctypes.c_int()
    assert lib.dvo_frame_get_level(h, slot, l, ctypes.byref(r), ctypes.byref(c), None, None, None, None) == 0
    e = np.zeros(r.value * c.value, np.uint8)
    assert lib.dvo_frame_get_level(h, slot, l, None, None, None, None, capi._ptr(e), None) == 0
    return e.reshape(c.value, r.value).T.copy()


def resident(tr, s, l):
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    n = ctypes.c_int()
    assert lib.dvo_get_ref_level(h, s, l, None, 0, ctypes.byref(n)) == 0
    xyz = np.zeros(3 * n.value, np.float32)
    assert lib.dvo_get_ref_level(h, s, l, capi._ptr(xyz), n.value, ctypes.byref(n)) == 0
    g = rig()["pyr"][0][0][l][0]
    dt, gx, gy = (np.zeros(g.size, np.float32) for _ in range(3))
    assert lib.dvo_get_now_level(h, s, l, capi._ptr(dt), capi._ptr(gx), capi._ptr(gy)) == 0
    return xyz.reshape(-1, 3), dt, gx, gy


@pytest.fixture(scope="module")
def rig_run():
    """the rig (masks on streams 0 and 2) and a tracker that never heard of masks, both over all ticks: run once"""
    G = rig()
    with make_tracker(3) as tr:
        for s, m in G["masks"].items():
            tr.set_stream_mask(s, m, MARGIN)
        got, stats = run(tr, G, [0, 1, 2])
        lens = {s: ref_len(tr, s) for s in range(3)}
    with make_tracker(3) as plain:
        base, base_stats = run(plain, G, [0, 1, 2])
        base_lens = {s: ref_len(plain, s) for s in range(3)}
    return dict(got=got, stats=stats, lens=lens, base=base, base_stats=base_stats, base_lens=base_lens)


def test_masked_trajectories_are_the_oracle_chains(rig_run):
    G = rig()
    for s in (0, 2):
        gop, want_lines = oracle_lines(G, s)
        ggop, got_lines = gop_lines(rig_run["got"][s])
        assert [(e["key"], e["reason"]) for e in ggop.elems] == [(e["key"], e["reason"]) for e in gop.elems], s
        assert [e[2] for e in rig_run["got"][s]] == [1, 0, 0, 0, 0, 5, 0, 0]
        Gm = np.array([[float(x) for x in ln.split()] for ln in got_lines])
        W = np.array([[float(x) for x in ln.split()] for ln in want_lines])
        print("stream", s, "pose lines: largest difference from the oracle chain", np.abs(Gm - W).max())
        assert np.abs(Gm - W).max() <= 2e-5                   # the comparison of tests/test_gpu_tracker_streams.py
        # and the mask matters: the chain without it is another trajectory
        _, plain_lines = oracle_lines(G, s, keep=[np.full(k.shape, 255, np.uint8) for k in G["keep"][s]])
        assert plain_lines != want_lines


def test_streams_do_not_notice_each_other(rig_run):
    G = rig()
    assert_same(rig_run["got"][1], rig_run["base"][1], "stream 1 beside masked neighbours")
    with make_tracker(1) as one:
        one.set_stream_mask(0, G["masks"][0], MARGIN)
        alone, _ = run(one, G, [0])
    assert_same(rig_run["got"][0], alone[0], "stream 0 alone")
    assert not all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(rig_run["got"][0], rig_run["base"][0]))
    for s in (0, 2):
        assert 0 < rig_run["lens"][s] < rig_run["base_lens"][s], (s, rig_run["lens"], rig_run["base_lens"])
    assert rig_run["lens"][1] == rig_run["base_lens"][1]


def test_stats(rig_run):
    from rgbd_odometry_amd.capi import DVO_FRAMES_MASK_LAUNCHES
    G = rig()
    for i, (st, b) in enumerate(zip(rig_run["stats"], rig_run["base_stats"])):
        assert st["runs"] == b["runs"] and st["syncs"] == b["syncs"] and st["key_frames"] == b["key_frames"], (i, st, b)
        # one upload run per tick (three consecutive streams, one bank): one more launch, whatever else the tick does
        assert st["launches"] == b["launches"] + DVO_FRAMES_MASK_LAUNCHES, (i, st, b)
    with make_tracker(3) as tr:                                # masks set and removed again: the counts of a tracker without the feature
        tr.set_stream_mask(-1, G["masks"][0], MARGIN)
        tr.set_stream_mask(-1, None)
        got, stats = run(tr, G, [0, 1, 2], n=3)
        assert stats == rig_run["base_stats"][:3]
        for s in range(3):
            assert_same(got[s], rig_run["base"][s][:3], "stream %d after removal" % s)


def test_mask_set_mid_stream_reset_and_all_streams():
    from rgbd_odometry_amd import DvoError, capi
    G = rig()
    with make_tracker(3) as tr:
        slot_of = {}

        def hook(i):
            if i == 4:                                        # after frame 3
                tr.set_stream_mask(0, G["masks"][0], MARGIN)
                hook.before = [stored_edge(tr, slot_of[3], l) for l in range(NL)]
            # stream 0 keeps its frames in slot bank * 3 + 0, the bank alternating from its first frame on
            slot_of[i] = (i % 2) * 3
        got, _ = run(tr, G, [0, 1, 2], n=6, hook=hook)
        for l in range(NL):
            # frame 3 sits in its slot as it was uploaded, unmasked; frames 4 and 5 (the other bank, then frame 3's) are masked
            assert np.array_equal(hook.before[l], G["canny"][0][3][l])
            assert np.array_equal(stored_edge(tr, slot_of[4], l), G["canny"][0][4][l] & G["keep"][0][l])
            assert np.array_equal(stored_edge(tr, slot_of[5], l), G["canny"][0][5][l] & G["keep"][0][l])
        # the bank bookkeeping of this test is right: frame 3's slot held frame 3 until frame 5 took it
        assert slot_of[3] == slot_of[5] != slot_of[4]
        # reset keeps the mask: the stream starts over (event 1) on masked edges
        tr.reset_stream(0)
        R, t, ev = tr.step([0], [G["seqs"][0][6][0]], [G["seqs"][0][6][1]])
        assert list(ev) == [1]
        assert any(np.array_equal(stored_edge(tr, q, 0), G["canny"][0][6][0] & G["keep"][0][0]) for q in (0, 3))
        assert np.array_equal(tr_keep(tr, 0, 0), G["keep"][0][0])
        # stream = -1: every stream has the same planes
        tr.set_stream_mask(-1, G["masks"][2], MARGIN)
        for s in range(3):
            for l in range(NL):
                assert np.array_equal(tr_keep(tr, s, l), G["keep"][2][l])
        for bad in (dict(stream=3), dict(stream=-2), dict(margin=-1), dict(margin=capi.DVO_MASK_MAX_MARGIN + 1)):
            args = dict(stream=1, mask=G["masks"][0], margin=MARGIN)
            args.update(bad)
            with pytest.raises(DvoError) as ei:
                tr.set_stream_mask(**args)
            assert ei.value.code == capi.DVO_ERR_INVALID
        with pytest.raises(ValueError):
            tr.set_stream_mask(1, np.zeros((ROWS, COLS + 1), np.uint8))
        for s in range(3):
            assert np.array_equal(tr_keep(tr, s, 1), G["keep"][2][1])


def tr_keep(tr, s, l):
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    r, c = ctypes.c_int(), ctypes.c_int()
    assert lib.dvo_frames_get_pair_mask_level(h, s, l, None, 0, ctypes.byref(r), ctypes.byref(c)) == 0
    k = np.zeros(r.value * c.value, np.uint8)
    assert lib.dvo_frames_get_pair_mask_level(h, s, l, capi._ptr(k), k.size, None, None) == 0
    return k.reshape(c.value, r.value).T.copy()


def test_archive_and_views_see_the_masked_edges(oracle):
    from rgbd_odometry_amd.capi import DVO_VIEW_REPROJ_ON_DT
    G = rig()
    Kf = tuple(np.float32(k) for k in K)
    with make_tracker(3) as tr:
        tr.set_archive(8)
        tr.set_views(True)
        for s, m in G["masks"].items():
            tr.set_stream_mask(s, m, MARGIN)
        for i in range(2):
            R, t, ev = tr.step([0, 1, 2], [G["seqs"][s][i][0] for s in range(3)], [G["seqs"][s][i][1] for s in range(3)])
            for s in (0, 2):
                k = s                                         # every stream is listed: entry = stream
                g0 = G["pyr"][s][i][0][0]
                rows, cols = g0.shape
                want_now = oracle.now_level_from_edges(cm(masked_edges(G, s, i, 0)), rows, cols)
                view = tr.view(s, DVO_VIEW_REPROJ_ON_DT)
                xyz, dt, gx, gy = resident(tr, s, 0)
                assert np.array_equal(dt.view(np.uint32), want_now[0].view(np.uint32))
                if i == 0:
                    assert ev[k] == 1
                    # the archived list of the masked key frame is the resident list of this step, and that is the oracle's on masked edges
                    kid = tr.key_frame_id(s)
                    assert kid >= 0
                    for l in range(NL):
                        g, d16 = G["pyr"][s][0][l]
                        d = d16.astype(np.uint16).copy()
                        d[d == 0] = 1
                        want_xyz, _ = oracle.enlist_ref_points(l, cm(masked_edges(G, s, 0, l)).astype(np.int32), cm(d).astype(np.float32), g.shape[0], g.shape[1], Kf)
                        arch = tr.archive_points(kid, l)
                        assert np.array_equal(arch, resident(tr, s, l)[0]) and np.array_equal(arch, np.asarray(want_xyz, np.float32).reshape(-1, 3)), (s, l)
                    # first frame: the view is the plain background, the restated convertTo of the masked distance transform
                    assert np.array_equal(view, vr.unmarked(want_now[0], g0, rows, cols)[0])
                    assert not np.array_equal(view, vr.unmarked(oracle.now_level_from_edges(cm(G["canny"][s][0][0]), rows, cols)[0], g0, rows, cols)[0])
                else:
                    want = vr.compose(oracle, 0, xyz, want_now[0], want_now[1], want_now[2], g0, rows, cols, K, R[k], t[k])
                    assert np.array_equal(view, want["reproj"])
                    bg = vr.unmarked(want_now[0], g0, rows, cols)[0]
                    assert np.array_equal(view[~want["marked"]], bg[~want["marked"]]) and int(want["marked"].sum()) > 0
