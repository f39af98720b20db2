"""Unregistered depth into the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_stream_depth_rig, dvo_tracker_step_raw_depth).
The contract: poses, events and signals are those of dvo_tracker_step_fmt fed dvo_depth_register_host's output as 16-bit depth, bit for
bit; with frames in HBM a step costs DVO_DEPTH_REGISTER_LAUNCHES more launches per run and no more host synchronisations.

The setup of tests/test_gpu_tracker_masks.py: 96 x 128, first_shift 1, 3 levels, iterations [8, 8, 8], one launch shape on every side
(block_threads 512, team_size 1), 8 ticks so that the forced key-frame switch and its re-run are inside.  Three streams:
  stream 0   96 x 128 depth, 25 mm baseline
  stream 1   60 x 80 depth, rotation and colour distortion, and the matching dvo_tracker_set_stream_undistort
  stream 2   an identity rig: the registered image is the raw image
The raw depth images are frame_gen.camera_frame depths as 16-bit millimetres, resampled to the rig's geometry by nearest neighbour."""
import ctypes
import functools

import numpy as np
import pytest

from rgbd_odometry_amd import frame_gen
import depth_register_reference as dr

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 96, 128, 3, 1
ITERS = [8, 8, 8]
K = (131.25, 131.25, 63.75, 47.75)           # of the first stored level (48 x 64)
ENGINE = dict(block_threads=512, team_size=1)
N_T = 8                                      # key_frame_every = 5: tick 5 is the forced switch and its re-run
SEEDS = (21, 23, 24)
MOTIONS = [(1.0, -2.0), (2.0, 1.0), (-1.0, 2.0)]
KC = dr.colour_K(ROWS, COLS)
DC5 = [0.1, -0.05, 0.001, -0.002, 0.01]


def rig_defs():
    R = dr.rot("z", 0.01) @ dr.rot("y", 0.02) @ dr.rot("x", -0.01)
    return [dr.rig((96, 128), KC, KC, t=[0.025, 0.0, 0.0]),
            dr.rig((60, 80), dr.scaled_K(KC, (ROWS, COLS), (60, 80)), KC, R=R, t=[0.03, -0.005, 0.002], Dc5=DC5),
            dr.rig((ROWS, COLS), KC, KC)]


def c_rig(g):
    from rgbd_odometry_amd import capi
    return capi.DvoDepthRig.make(g["depth_shape"], g["Kd4"], g["Kc4"], R=g["R"], t=g["t"], Dc5=g["Dc5"])


@functools.lru_cache(maxsize=None)
def rig():
    """colour images, raw depth images and the host-registered depth images of the three streams: computed once"""
    from rgbd_odometry_amd import capi
    defs = rig_defs()
    bgr, raw, reg = [], [], []
    for s in range(3):
        frames = [frame_gen.camera_frame(SEEDS[s], ROWS, COLS, shift=(int(round(MOTIONS[s][0] * i)), int(round(MOTIONS[s][1] * i))), holes=True)
                  for i in range(N_T)]
        bgr.append([b for b, _ in frames])
        raw.append([dr.resample_nn(frame_gen.as_format(b, d, "bgr8", "u16")[1], defs[s]["depth_shape"]) for b, d in frames])
        reg.append([capi.depth_register_host(c_rig(defs[s]), r, ROWS, COLS) for r in raw[s]])
    for i in range(N_T):
        assert np.array_equal(reg[2][i], raw[2][i]) and (raw[2][i] == 0).any()          # the identity rig returns its input, holes included
        assert not np.array_equal(reg[0][i], raw[0][i]) and (reg[1][i] != 0).mean() > 0.5
    return dict(defs=defs, bgr=bgr, raw=raw, reg=reg)


def make_tracker(n, rigs=True, **kw):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    for k, v in ENGINE.items():
        setattr(p, k, v)
    tr = DvoTracker(n, params=p, iters=ITERS, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, **kw)
    tr.set_intrinsics(*K)
    if n > 1:
        tr.set_stream_undistort(1, KC, DC5)                    # on both sides: the rig's Kc4 / Dc5 describe the image as it is uploaded
    if rigs:
        for s, g in enumerate(rig()["defs"][:n]):
            tr.set_stream_depth_rig(s, c_rig(g))
    return tr


def to_device(arr):
    import torch
    t = torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint8).copy()).cuda()
    return t, t.data_ptr()


@functools.lru_cache(maxsize=None)
def device_frames():
    G = rig()
    return {k: [[to_device(a) for a in seq] for seq in G[k]] for k in ("bgr", "raw", "reg")}


def signals_of(tr, s):
    from rgbd_odometry_amd import DvoError
    try:
        b, r, n = tr.signals(s)
        return (np.float32(b).view(np.uint32).item(), np.float32(r).view(np.uint32).item(), int(n))
    except DvoError:
        return None


def run(tr, streams_at, depth_key, device, raw_step, n=N_T):
    """steps tr for n ticks; streams_at(i): the streams listed at tick i, each on its own next frame.  Per stream [(R, t, event,
    signals)], and the stats of every tick"""
    from rgbd_odometry_amd import capi
    G, D = rig(), device_frames() if device else None
    frame = {s: 0 for s in range(3)}
    got, stats = {s: [] for s in range(3)}, []
    for i in range(n):
        streams = streams_at(i)
        f = [frame[s] for s in streams]
        if device:
            b = [D["bgr"][s][k][1] for s, k in zip(streams, f)]
            d = [D[depth_key][s][k][1] for s, k in zip(streams, f)]
            kw = dict(flags=capi.DVO_UPLOAD_DEVICE, image_format=capi.DVO_CAM_BGR8, depth_format=capi.DVO_DEPTH_U16)
        else:
            b = [G["bgr"][s][k] for s, k in zip(streams, f)]
            d = [G[depth_key][s][k] for s, k in zip(streams, f)]
            kw = {}
        R, t, ev = (tr.step_raw_depth if raw_step else tr.step)(streams, b, d, **kw)
        stats.append(tr.stats())
        for k, s in enumerate(streams):
            got[s].append((R[k], t[k], int(ev[k]), signals_of(tr, s)))
            frame[s] += 1
    return got, stats


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for n, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (what, n, "event", g[2], w[2])
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (what, n, "pose", g[0], w[0], g[1], w[1])
        assert g[3] == w[3], (what, n, "signals", g[3], w[3])


ALL = lambda i: [0, 1, 2]
RIGLESS_COUNTS = [(28, 8), (14, 1), (14, 1), (14, 1), (14, 1), (32, 3), (14, 1), (14, 1)]


@pytest.fixture(scope="module")
def runs():
    """tracker A (rigs, step_raw_depth) and tracker B (no rigs, step_fmt on the host-registered depth), with host and with device
    sources: run once"""
    out = {}
    for device in (False, True):
        with make_tracker(3) as A:
            out["A", device] = run(A, ALL, "raw", device, True)
        with make_tracker(3, rigs=False) as B:
            out["B", device] = run(B, ALL, "reg", device, False)
    return out


@pytest.mark.parametrize("device", [False, True])
def test_poses_events_and_signals_are_those_of_the_host_registered_depth(runs, device):
    (a, _), (b, _) = runs["A", device], runs["B", device]
    for s in range(3):
        assert_same(a[s], b[s], "stream %d, %s sources" % (s, "device" if device else "host"))
        assert [e[2] for e in a[s]] == [1, 0, 0, 0, 0, 5, 0, 0]
        assert_same(runs["A", True][0][s], runs["A", False][0][s], "stream %d, device against host sources" % s)
    # the registration matters: the trajectory on the raw image of stream 0 taken as registered is another one
    with make_tracker(3, rigs=False) as plain:
        p, _ = run(plain, lambda i: [0], "raw", False, False, n=3)
    assert not all(np.array_equal(x[1], y[1]) for x, y in zip(p[0], a[0][:3]))


def test_identity_rig_is_a_plain_step(runs):
    """stream 2 (identity rig): the trajectory of dvo_tracker_step_fmt on the unregistered input"""
    with make_tracker(3, rigs=False) as plain:
        p, _ = run(plain, lambda i: [2], "raw", False, False)
    assert_same(runs["A", False][0][2], p[2], "stream 2 against a plain step on its raw depth")


def test_launches_and_synchronisations(runs):
    from rgbd_odometry_amd.capi import DVO_DEPTH_REGISTER_LAUNCHES
    (_, sa), (_, sb) = runs["A", True], runs["B", True]
    for i, (a, b) in enumerate(zip(sa, sb)):
        # one upload run per tick (three consecutive streams, one bank): two more launches, whatever else the tick does
        assert a["launches"] == b["launches"] + DVO_DEPTH_REGISTER_LAUNCHES, (i, a, b)
        assert a["syncs"] == b["syncs"] and a["runs"] == b["runs"] and a["key_frames"] == b["key_frames"], (i, a, b)
    # a tracker that never gets a rig: the (launches, synchronisations) per tick the library had before depth registration existed,
    # read off the parent commit's library on these frames, host and device sources alike (first frames, ordinary ticks, the key tick)
    for device in (False, True):
        assert [(st["launches"], st["syncs"]) for st in runs["B", device][1]] == RIGLESS_COUNTS, device
    # a tracker whose rigs were set and removed again steps with the counts of one that never heard of them
    with make_tracker(3) as tr:
        for s in range(3):
            tr.set_stream_depth_rig(s, None)
        got, stats = run(tr, ALL, "reg", True, False, n=3)
    assert stats == sb[:3]
    for s in range(3):
        assert_same(got[s], runs["B", True][0][s][:3], "stream %d after removal" % s)


def test_a_subset_step_that_splits_the_run():
    """stream 1 skips tick 3: that tick is two runs (streams 0 and 2 are not neighbours), and from then on stream 1 writes the other
    bank than its neighbours -- three runs per tick"""
    from rgbd_odometry_amd.capi import DVO_DEPTH_REGISTER_LAUNCHES
    listed = lambda i: [0, 2] if i == 3 else [0, 1, 2]
    upload_runs = [1, 1, 1, 2, 3, 3]
    with make_tracker(3) as A:
        a, sa = run(A, listed, "raw", True, True, n=6)
    with make_tracker(3, rigs=False) as B:
        b, sb = run(B, listed, "reg", True, False, n=6)
    for s in range(3):
        assert_same(a[s], b[s], "stream %d" % s)
    assert len(a[1]) == 5
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert x["launches"] == y["launches"] + DVO_DEPTH_REGISTER_LAUNCHES * upload_runs[i], (i, x, y)
        assert x["syncs"] == y["syncs"] and x["runs"] == y["runs"], (i, x, y)
    with make_tracker(3) as A:                                 # the same with host sources: the staging pools of several runs per step
        a2, _ = run(A, listed, "raw", False, True, n=6)
    for s in range(3):
        assert_same(a2[s], a[s], "stream %d, host sources" % s)


def test_refusals_leave_the_tracker_as_it_was(runs):
    from rgbd_odometry_amd import DvoError, capi
    G = rig()
    with make_tracker(4) as tr:                                # stream 3 has no rig
        frames = lambda i, ss: ([G["bgr"][s % 3][i] for s in ss], [G["raw"][s % 3][i] for s in ss])
        got = {s: [] for s in range(3)}

        def good(i):
            R, t, ev = tr.step_raw_depth([0, 1, 2], *frames(i, [0, 1, 2]))
            for s in range(3):
                got[s].append((R[s], t[s], int(ev[s]), signals_of(tr, s)))

        def refused(code, fn):
            with pytest.raises(DvoError) as ei:
                fn()
            assert ei.value.code == code

        refused(capi.DVO_ERR_STATE, lambda: tr.step_raw_depth([0, 1, 2, 3], *frames(0, [0, 1, 2, 3])))       # before the first frame
        good(0)
        good(1)
        refused(capi.DVO_ERR_STATE, lambda: tr.set_stream_depth_rig(0, c_rig(G["defs"][0])))               # a running stream
        refused(capi.DVO_ERR_STATE, lambda: tr.set_stream_depth_rig(1, None))
        refused(capi.DVO_ERR_STATE, lambda: tr.step_raw_depth([0, 1, 2, 3], *frames(2, [0, 1, 2, 3])))
        refused(capi.DVO_ERR_STATE, lambda: tr.step_raw_depth([3], *frames(2, [3])))
        for flags in (capi.DVO_UPLOAD_DEPTH_RAW, capi.DVO_UPLOAD_MAPPED, capi.DVO_UPLOAD_DIRECT, capi.DVO_UPLOAD_ASYNC,
                      capi.DVO_UPLOAD_DEVICE | capi.DVO_UPLOAD_DEPTH_RAW):
            refused(capi.DVO_ERR_INVALID, lambda: _step_flags(tr, frames(2, [0, 1, 2]), flags))
        bad = c_rig(G["defs"][0])
        bad.Kd4[0] = float("nan")
        refused(capi.DVO_ERR_INVALID, lambda: tr.set_stream_depth_rig(3, bad))
        refused(capi.DVO_ERR_INVALID, lambda: tr.set_stream_depth_rig(4, c_rig(G["defs"][0])))
        with pytest.raises(ValueError):
            tr.step_raw_depth([0, 1, 2], G["bgr"][0][2:5], [G["raw"][1][2]] * 3)
        for i in range(2, 5):
            good(i)
        # a stream at its start may get a rig, and a reset stream may change it
        tr.set_stream_depth_rig(3, c_rig(G["defs"][2]))
        tr.reset_stream(0)
        tr.set_stream_depth_rig(0, c_rig(G["defs"][0]))
    for s in range(3):
        assert_same(got[s], runs["A", False][0][s][:5], "stream %d across refused calls" % s)


def _step_flags(tr, frames, flags):
    """step_raw_depth on host frames with flags the binding would not pass on its own"""
    from rgbd_odometry_amd import capi
    bl, dl = [np.ascontiguousarray(b) for b in frames[0]], [np.ascontiguousarray(d) for d in frames[1]]
    n = len(bl)
    S = (ctypes.c_int * n)(*range(n))
    B = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bl])
    D = (ctypes.c_void_p * n)(*[d.ctypes.data for d in dl])
    R, t, ev = np.zeros((n, 9)), np.zeros((n, 3)), np.zeros(n, np.int32)
    tr._chk(tr.lib.dvo_tracker_step_raw_depth(tr._h, n, S, B, capi.DVO_CAM_BGR8, D, capi.DVO_DEPTH_U16, ROWS, COLS, flags, capi._ptr(R), capi._ptr(t),
                                              ev.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))


def test_device_colour_images_that_cannot_be_read_in_place(runs):
    """colour images in HBM one byte off a 4-byte boundary: the upload gathers both sources on its copy streams instead of reading
    them in place, and that gather must come after the registration that writes the depth images it reads"""
    import torch
    from rgbd_odometry_amd import capi
    G = rig()
    nbytes = ROWS * COLS * 3
    raw = device_frames()["raw"]
    with make_tracker(3) as A:
        got = {s: [] for s in range(3)}
        for i in range(N_T):
            bufs = []
            for s in range(3):
                t = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
                t[1:1 + nbytes] = torch.from_numpy(G["bgr"][s][i].reshape(-1)).cuda()
                bufs.append(t)
            torch.cuda.synchronize()
            assert all((t.data_ptr() + 1) % 4 == 1 for t in bufs)
            R, t_, ev = A.step_raw_depth([0, 1, 2], [t.data_ptr() + 1 for t in bufs], [raw[s][i][1] for s in range(3)],
                                         flags=capi.DVO_UPLOAD_DEVICE, image_format=capi.DVO_CAM_BGR8, depth_format=capi.DVO_DEPTH_U16)
            for s in range(3):
                got[s].append((R[s], t_[s], int(ev[s]), signals_of(A, s)))
    for s in range(3):
        assert_same(got[s], runs["B", True][0][s], "stream %d, colour one byte off alignment" % s)
