"""The views of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_views / dvo_tracker_get_residue_histogram /
dvo_tracker_get_view / dvo_tracker_view_device): after every step, per listed stream, the residue histogram and two BGR8 images --
the reference points reprojected on the distance transform and the residue heat map on the now grey image -- from two extra launches
per rendering (dvo_tracker_views.hip) and no extra host synchronisation.

Expected values: tests/views_reference.py on the reference points and the now level the tracker's context holds AFTER the step
(dvo_get_ref_level / dvo_get_now_level of dvo_tracker_context), the CPU oracle's eval_points at the pose the step returned with the
stream's own intrinsics, and the grey level of the oracle's pyramid of the frame that was fed.  Everything is integers and bytes:
every comparison is np.array_equal."""
import ctypes

import numpy as np
import pytest

import frame_gen
import frame_reference as fr
import views_reference as vr

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 240, 320, 3, 0                 # the geometry of tests/test_gpu_tracker_information.py
ITERS = [8, 8, 8]
K = (262.5, 262.5, 159.75, 119.75)
ENGINE = dict(block_threads=512, team_size=1)
MOTIONS = [(0.5, -1.0), (1.0, 0.5), (-0.5, 1.5), (1.5, -0.5), (0.0, 1.4)]
N_S, N_T = 5, 7                                        # key_frame_every = 5: tick 5 is the forced switch and its re-run
GEOM = dict(rows=ROWS, cols=COLS, nl=NL, shift=SHIFT)


def sequence(seed, n, motion, rows=ROWS, cols=COLS):
    dy, dx = motion
    return [frame_gen.camera_frame(seed, rows, cols, shift=(int(round(dy * i)), int(round(dx * i))), holes=True) for i in range(n)]


def tracked(n, iters=ITERS, views=True, information=False, geom=GEOM, **engine):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in dict(ENGINE, **engine).items():
        setattr(p, k, v)
    tr = DvoTracker(n, params=p, iters=iters, rows=geom["rows"], cols=geom["cols"], n_levels=geom["nl"], first_shift=geom["shift"])
    tr.set_intrinsics(*K)
    if views:
        tr.set_views(True)
    if information:
        tr.set_information(True)
    tr.views_on, tr.information_on, tr.geom = views, information, geom
    return tr


def level_dims(geom, level):
    return fr.level_size(geom["rows"], geom["shift"] + level), fr.level_size(geom["cols"], geom["shift"] + level)


def resident(tr, stream, level):
    """reference points and now level of `stream` as the tracker's context holds them"""
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    n = ctypes.c_int()
    assert lib.dvo_get_ref_level(h, stream, level, None, 0, ctypes.byref(n)) == 0
    xyz = np.zeros(3 * n.value, np.float32)
    assert lib.dvo_get_ref_level(h, stream, level, capi._ptr(xyz), n.value, ctypes.byref(n)) == 0
    rows, cols = level_dims(tr.geom, level)
    dt, gx, gy = (np.zeros(rows * cols, np.float32) for _ in range(3))
    assert lib.dvo_get_now_level(h, stream, level, capi._ptr(dt), capi._ptr(gx), capi._ptr(gy)) == 0
    return xyz.reshape(-1, 3), dt, gx, gy


def now_form(tr, stream, level):
    """(palette size or refusal code, partial, texel mode of the last alignment) of the stream's now level"""
    from rgbd_odometry_amd import capi
    lib, h = capi.load_library(), tr.context_handle()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.dvo_get_now_compact_info(h, stream, level, ctypes.byref(a)) == 0
    assert lib.dvo_get_now_compact_partial(h, stream, level, ctypes.byref(b)) == 0
    assert lib.dvo_get_level_texel_mode(h, stream, level, ctypes.byref(c)) == 0
    return a.value, bool(b.value), c.value & 3


class Greys:
    """grey level of the oracle's pyramid of a fed frame, computed once per frame"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, frame, geom, level):
        key = (id(frame[0]), geom["nl"], geom["shift"])
        if key not in self.cache:
            self.cache[key] = (frame, self.oracle.build_pyramid(frame[0], frame[1], n_levels=geom["nl"], first_shift=geom["shift"]))
        rows, cols = level_dims(geom, level)
        return np.asarray(self.cache[key][1][level][0], np.uint8).reshape(rows, cols)


@pytest.fixture(scope="module")
def greys(oracle):
    return Greys(oracle)


def get_views(tr, s):
    from rgbd_odometry_amd.capi import DVO_VIEW_REPROJ_ON_DT, DVO_VIEW_RESIDUE_HEAT
    return dict(rec=tr.residue_histogram(s), reproj=tr.view(s, DVO_VIEW_REPROJ_ON_DT), heat=tr.view(s, DVO_VIEW_RESIDUE_HEAT))


def same_views(a, b):
    return (np.array_equal(a["rec"]["hist"], b["rec"]["hist"]) and a["rec"]["n_points"] == b["rec"]["n_points"] and
            a["rec"]["level"] == b["rec"]["level"] and np.array_equal(a["reproj"], b["reproj"]) and np.array_equal(a["heat"], b["heat"]))


def check_against_reference(oracle, greys, tr, s, level, Ks, R, t, first, frame, got, what):
    xyz, dt, gx, gy = resident(tr, s, level)
    rows, cols = level_dims(tr.geom, level)
    grey = greys(frame, tr.geom, level)
    rec = got["rec"]
    assert got["reproj"].shape == got["heat"].shape == (rows, cols, 3)
    if first:
        want = vr.unmarked(dt, grey, rows, cols)
        assert rec["level"] == -1 and rec["n_points"] == 0 and not rec["hist"].any(), what
        assert np.array_equal(got["reproj"], want[0]) and np.array_equal(got["heat"], want[1]), what
        return 0
    want = vr.compose(oracle, level, xyz, dt, gx, gy, grey, rows, cols, Ks, R, t)
    n_marked = int(want["marked"].sum())
    print(what, "N", len(xyz), "visible", int(want["visible"].sum()), "marked pixels", n_marked, "bins used", int((want["hist"] > 0).sum()),
          "hist equal", np.array_equal(rec["hist"], want["hist"]), "reproj differs at", int((got["reproj"] != want["reproj"]).any(2).sum()),
          "heat differs at", int((got["heat"] != want["heat"]).any(2).sum()))
    assert rec["level"] == level and rec["n_points"] == len(xyz), what
    assert np.array_equal(rec["hist"], want["hist"]), what
    assert int(rec["hist"].sum()) == len(xyz) and rec["hist"][0] == 0, what
    assert np.array_equal(got["reproj"], want["reproj"]), what
    assert np.array_equal(got["heat"], want["heat"]), what
    assert n_marked >= 50, what                                           # two empty pictures would show nothing
    return n_marked


def run(tr, seqs, schedule, oracle=None, greys=None, level=0, Ks=None):
    """schedule: per tick [(stream, frame index)].  Per tick: dict(R, t, ev, stats, views={stream: ...}, sig, info); with an oracle
    every stream's views are checked against the reference right after its step"""
    ticks = []
    for n, entry in enumerate(schedule):
        streams = [s for s, _ in entry]
        R, t, ev = tr.step(streams, [seqs[s][i][0] for s, i in entry], [seqs[s][i][1] for s, i in entry])
        out = dict(R=R, t=t, ev=ev.copy(), stats=tr.stats(), views={}, sig={}, info={})
        for k, (s, i) in enumerate(entry):
            if tr.views_on:
                out["views"][s] = get_views(tr, s)
                if oracle is not None:
                    check_against_reference(oracle, greys, tr, s, level, (Ks or {}).get(s, K), R[k], t[k], ev[k] == 1, seqs[s][i],
                                            out["views"][s], ("tick", n, "stream", s, "event", int(ev[k])))
            if ev[k] != 1:
                out["sig"][s] = tr.signals(s)
            if tr.information_on:
                out["info"][s] = tr.information(s)
        ticks.append(out)
    return ticks


FULL = [[(s, n) for s in range(N_S)] for n in range(N_T)]


@pytest.fixture(scope="module")
def seqs():
    return [sequence(900 + s, N_T, MOTIONS[s]) for s in range(N_S)]


@pytest.fixture(scope="module")
def on_run(seqs):
    """five streams, seven ticks, views and information on; nothing but the steps and the getters touches the context"""
    with tracked(N_S, information=True) as tr:
        return run(tr, seqs, FULL)


def test_parity_on_every_tick_and_stream(seqs, oracle, greys, on_run):
    with tracked(N_S) as tr:
        assert tr.view_size() == (ROWS, COLS, 0)
        ticks = run(tr, seqs, FULL, oracle=oracle, greys=greys)
        assert all(now_form(tr, s, 0)[0] > 0 and not now_form(tr, s, 0)[1] and now_form(tr, s, 0)[2] == 2 for s in range(N_S))      # the compact form
    assert [x["ev"].tolist() for x in ticks] == [[1] * N_S] + [[0] * N_S] * 4 + [[5] * N_S] + [[0] * N_S]
    assert ticks[5]["stats"]["key_frames"] == N_S           # the views of tick 5 are the re-run's, against the new reference
    # reading the resident levels between the steps changed nothing
    for a, b in zip(ticks, on_run):
        assert all(same_views(a["views"][s], b["views"][s]) for s in range(N_S))


def test_coarse_finest_level(seqs, oracle, greys):
    """the views are taken on the finest level that RAN: 120 x 160"""
    with tracked(2, iters=[0, 8, 8]) as tr:
        assert tr.view_size() == (120, 160, 1)
        ticks = run(tr, seqs, [[(0, n), (1, n)] for n in range(3)], oracle=oracle, greys=greys, level=1)
    assert all(v["rec"]["level"] == 1 for x in ticks[1:] for v in x["views"].values())


def test_odd_geometry(oracle, greys):
    """250 x 322 camera frames at full resolution: rows no multiple of the compact form's 6, cols no multiple of its 4 nor of the
    background tile's 64, a row of 966 bytes (rows of the images start on every alignment)"""
    geom = dict(rows=250, cols=322, nl=2, shift=0)
    s = [sequence(77, 3, (1.0, -1.5), 250, 322)]
    with tracked(1, iters=[8, 8], geom=geom) as tr:
        assert tr.view_size() == (250, 322, 0)
        run(tr, s, [[(0, n)] for n in range(3)], oracle=oracle, greys=greys)


def test_both_resident_forms(seqs, oracle, greys):
    """a tracker whose now levels are held as 16-byte texels (engine_variant = 4: no compact form): the same views"""
    sched = [[(0, n), (1, n)] for n in range(3)]
    with tracked(2, engine_variant=4) as tr:
        texels = run(tr, seqs, sched, oracle=oracle, greys=greys)
        forms = [now_form(tr, s, 0) for s in (0, 1)]
        assert all(f[0] <= 0 and not f[1] and f[2] != 2 for f in forms), forms
    with tracked(2) as tr:
        compact = run(tr, seqs, sched)
        forms = [now_form(tr, s, 0) for s in (0, 1)]
        assert all(f[0] > 0 and not f[1] and f[2] == 2 for f in forms), forms
    for a, b in zip(texels, compact):
        assert all(same_views(a["views"][s], b["views"][s]) for s in (0, 1))


def test_mixed_rig(seqs, oracle, greys):
    """two streams with their own intrinsics, each against the reference with ITS camera model"""
    Ks = {0: (250.0, 254.0, 161.0, 118.0), 1: (275.0, 271.5, 157.5, 121.25)}
    with tracked(2) as tr:
        for s, k in Ks.items():
            tr.set_stream_intrinsics(s, *k)
        run(tr, seqs, [[(0, n), (1, n)] for n in range(3)], oracle=oracle, greys=greys, Ks=Ks)


def test_views_depend_on_the_stream_alone(seqs, on_run):
    """identical bytes: stream 3 of the five-stream tracker, the same frames as the only stream of a one-stream tracker, and as stream 3
    of steps that list [1, 3] in that order or the other"""
    with tracked(1) as tr:
        alone = run(tr, [seqs[3]], [[(0, n)] for n in range(N_T)])
    with tracked(N_S) as tr:
        first = run(tr, seqs, [[(3, n), (1, n)] for n in range(N_T)])
    with tracked(N_S) as tr:
        last = run(tr, seqs, [[(1, n), (3, n)] for n in range(N_T)])
    for n in range(N_T):
        a = on_run[n]["views"][3]
        assert same_views(a, alone[n]["views"][0]) and same_views(a, first[n]["views"][3]) and same_views(a, last[n]["views"][3]), n
    assert on_run[5]["ev"][3] == 5 and on_run[5]["views"][3]["rec"]["n_points"] > 50


def test_nothing_else_moves(seqs, on_run):
    """views on against off (information on in both): the same poses, events, signals and information records, the same host
    synchronisations, DVO_TRACKER_VIEW_LAUNCHES more launches per rendering"""
    from rgbd_odometry_amd.capi import DVO_TRACKER_VIEW_LAUNCHES
    with tracked(N_S, views=False, information=True) as tr:
        off = run(tr, seqs, FULL)
    for n, (a, b) in enumerate(zip(on_run, off)):
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"], n
        for s in range(N_S):
            assert all(np.array_equal(a["info"][s][k], b["info"][s][k]) for k in ("H", "g", "sum_eps2", "n_visible", "level")), (n, s)
        assert a["stats"]["syncs"] == b["stats"]["syncs"], (n, a["stats"], b["stats"])
        renderings = 2 if b["stats"]["key_frames"] else 1
        assert a["stats"]["launches"] == b["stats"]["launches"] + DVO_TRACKER_VIEW_LAUNCHES * renderings, (n, a["stats"], b["stats"])
        assert {k: v for k, v in a["stats"].items() if k != "launches"} == {k: v for k, v in b["stats"].items() if k != "launches"}, n
    assert [x["stats"]["key_frames"] for x in off] == [0, 0, 0, 0, 0, N_S, 0]


def test_view_device(seqs):
    """the resident image behind dvo_tracker_view_device holds the bytes dvo_tracker_get_view copies"""
    from rgbd_odometry_amd import capi
    hip = ctypes.CDLL("libamdhip64.so")                                   # the runtime the library already runs on
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    with tracked(2) as tr:
        for n in range(2):
            tr.step([0, 1], [seqs[s][n][0] for s in (0, 1)], [seqs[s][n][1] for s in (0, 1)])
        rows, cols, _ = tr.view_size()
        seen = set()
        for s in (0, 1):
            for which in (capi.DVO_VIEW_REPROJ_ON_DT, capi.DVO_VIEW_RESIDUE_HEAT):
                addr = tr.view_device(s, which)
                assert addr and addr not in seen
                seen.add(addr)
                host = np.zeros((rows, cols, 3), np.uint8)
                assert hip.hipMemcpy(host.ctypes.data, addr, host.nbytes, 2) == 0       # hipMemcpyDeviceToHost
                assert np.array_equal(host, tr.view(s, which)), (s, which)
                assert host.any()


def test_contract(seqs):
    from rgbd_odometry_amd import DvoError
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE, DVO_TRACKER_VIEW_LAUNCHES, DVO_VIEW_RESIDUE_HEAT

    def refused(code, fn, *a):
        with pytest.raises(DvoError) as ei:
            fn(*a)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    assert DVO_TRACKER_VIEW_LAUNCHES == 2
    with tracked(2, views=False) as tr:
        step = lambda n, streams=(0, 1): tr.step(list(streams), [seqs[s][n][0] for s in streams], [seqs[s][n][1] for s in streams])
        step(0)
        refused(DVO_ERR_STATE, tr.residue_histogram, 0)            # off by default
        refused(DVO_ERR_STATE, tr.view, 0, 0)
        refused(DVO_ERR_STATE, tr.view_device, 0, 0)
        step(1)
        plain = tr.stats()                                         # an ordinary step while views are off
        tr.set_views(True)
        refused(DVO_ERR_STATE, tr.residue_histogram, 0)            # on, not stepped since
        refused(DVO_ERR_STATE, tr.view, 0, 0)
        refused(DVO_ERR_INVALID, tr.residue_histogram, 2)
        refused(DVO_ERR_INVALID, tr.residue_histogram, -1)
        refused(DVO_ERR_INVALID, tr.view, 2, 0)
        step(2)
        on = tr.stats()
        assert on["syncs"] == plain["syncs"]                                                   # no host synchronisation added
        assert on["launches"] == plain["launches"] + DVO_TRACKER_VIEW_LAUNCHES                 # one rendering per ordinary step
        refused(DVO_ERR_INVALID, tr.view, 0, 2)                    # view out of range
        refused(DVO_ERR_INVALID, tr.view, 0, -1)
        refused(DVO_ERR_INVALID, tr.view_device, 0, 2)
        rec = tr.residue_histogram(0)
        assert rec["level"] == 0 and rec["n_points"] > 50 and int(rec["hist"].sum()) == rec["n_points"]
        tr.set_information(True)                                   # independent of information: both on
        step(3)
        both = tr.stats()
        assert both["launches"] == plain["launches"] + DVO_TRACKER_VIEW_LAUNCHES + 1 and both["syncs"] == plain["syncs"]
        assert tr.information(0)["level"] == 0 and tr.residue_histogram(0)["level"] == 0
        tr.set_information(False)
        tr.reset_stream(1)
        refused(DVO_ERR_STATE, tr.residue_histogram, 1)            # reset: nothing until its next step
        refused(DVO_ERR_STATE, tr.view, 1, DVO_VIEW_RESIDUE_HEAT)
        assert tr.residue_histogram(0)["n_points"] > 50
        step(4, streams=(1,))                                      # stream 1 starts over: the zero record
        rec = tr.residue_histogram(1)
        assert rec["level"] == -1 and rec["n_points"] == 0 and not rec["hist"].any()
        tr.set_views(False)
        refused(DVO_ERR_STATE, tr.residue_histogram, 0)
        refused(DVO_ERR_STATE, tr.view, 0, 0)
    # a step with a key-frame switch: two renderings; steps after set_views(0): the launches of a tracker that never had views
    with tracked(1, views=False) as never, tracked(1) as onoff:
        for n in range(N_T):
            if n == 6:
                onoff.set_views(False)
            for tr in (never, onoff):
                tr.step([0], [seqs[0][n][0]], [seqs[0][n][1]])
            a, b = onoff.stats(), never.stats()
            renderings = 0 if n == 6 else (2 if b["key_frames"] else 1)
            assert b["key_frames"] == (1 if n == 5 else 0), (n, b)
            assert a["launches"] == b["launches"] + DVO_TRACKER_VIEW_LAUNCHES * renderings and a["syncs"] == b["syncs"], (n, a, b)
    for kw in (dict(interpolate_dt=1), dict(engine_variant=1), dict(debug_alias_mod=1)):
        with tracked(1, views=False, **kw) as tr:
            refused(DVO_ERR_INVALID, tr.set_views, True)
            refused(DVO_ERR_STATE, tr.residue_histogram, 0)        # nothing changed: still off
            tr.set_views(False)
