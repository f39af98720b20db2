"""The multi-stream trackers fed camera frames in sensor formats (dvo_tracker_step_fmt, dvo_photo_streams_step_fmt): poses, events,
signals and the per-tick launch and synchronisation counts must equal, bit for bit and tick for tick, those of the existing entry
points on a second handle fed the (BGR8, float depth) input the formats stand for (include/dvo_amd.h)."""
import ctypes

import numpy as np
import pytest

import frame_gen
import frame_reference as fr

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 240, 320, 3, 0                 # the geometry of tests/test_gpu_tracker_streams.py
ITERS = [8, 8, 8]
K = (262.5, 262.5, 159.75, 119.75)
BARREL = ((255.0, 250.0, 161.7, 118.3), (-0.3, 0.1, 0.002, 0.001, -0.02))
MOTIONS = [(0.5, -1.0), (1.0, 0.5), (-0.5, 1.5)]


def to_u16(depth_m):
    """a sensor's 16-bit millimetres of a frame_gen depth image: holes (0.0, NaN) are 0"""
    return np.clip(np.nan_to_num(np.rint(depth_m * 1000.0), nan=0.0), 0, 65535).astype(np.uint16)


def sequences(seed, n, rows, cols):
    out = []
    for s, (dy, dx) in enumerate(MOTIONS):
        frames = [frame_gen.camera_frame(seed + s, rows, cols, shift=(int(round(dy * i)), int(round(dx * i))), holes=True) for i in range(n)]
        out.append([(bgr, to_u16(d)) for bgr, d in frames])
        assert all((d == 0).any() for _, d in out[-1])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_tracker(n):
    from rgbd_odometry_amd import DvoTracker, capi
    p = capi.DvoParams()
    capi.load_library().dvo_params_default(ctypes.byref(p))
    p.block_threads, p.team_size = 512, 1
    tr = DvoTracker(n, params=p, iters=ITERS, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT)
    tr.set_intrinsics(*K)
    tr.set_stream_undistort(1, np.array(BARREL[0]), np.array(BARREL[1]))          # one stream with a calibration of its own
    return tr


@pytest.fixture(scope="module")
def tracker_frames():
    return sequences(100, 8, ROWS, COLS)


@pytest.mark.parametrize("fmt", ["mono8", "rgb8"])
def test_tracker_step_fmt_equals_tracker_step(tracker_frames, fmt):
    """three streams, eight ticks (tick 5 forces a key frame), 16-bit depth with holes as the pyramid publisher takes it (0 -> 1)"""
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    seqs, streams, events = tracker_frames, [0, 1, 2], []
    with make_tracker(3) as new, make_tracker(3) as old:
        for n in range(8):
            bgr = [seqs[s][n][0] for s in streams]
            d16 = [seqs[s][n][1] for s in streams]
            if fmt == "mono8":
                grey = [fr.bgr2gray(b) for b in bgr]
                got = new.step(streams, grey, d16)
                bgr = [np.repeat(g[..., None], 3, 2) for g in grey]
            else:
                got = new.step(streams, [np.ascontiguousarray(b[..., ::-1]) for b in bgr], d16, rgb=True)
            as_float = [np.where(d == 0, 1, d).astype(np.float32) for d in d16]
            want = old.step(streams, bgr, as_float, flags=DVO_UPLOAD_DEPTH_RAW)
            for g, w, name in zip(got, want, ("R_rel", "t_rel", "event")):
                assert same_bits(g, w), (fmt, n, name, g, w)
            sn, so = new.stats(), old.stats()
            assert sn == so, (fmt, n, sn, so)                               # launches and host synchronisations, tick for tick
            for s in streams:
                if got[2][s] != 1:
                    assert new.signals(s) == old.signals(s), (fmt, n, s)
            events.append(got[2].tolist())
    assert events[0] == [1, 1, 1] and any(e >= 2 for ev in events[1:] for e in ev), events      # a key-frame switch happened


def test_photo_streams_step_fmt_equals_photo_streams_step():
    """three streams, a reference every fourth frame, six ticks; 16-bit depth with holes, which stay 0 (DVO_UPLOAD_DEPTH_RAW is forced)"""
    from rgbd_odometry_amd import DvoPhotoStreams
    seqs, streams = sequences(50, 6, 480, 640), [0, 1, 2]
    Kp = (525.0, 525.0, 319.5, 239.5)
    with DvoPhotoStreams(3, Kp, ref_every=4) as new, DvoPhotoStreams(3, Kp, ref_every=4) as old:
        for n in range(6):
            bgr = [seqs[s][n][0] for s in streams]
            d16 = [seqs[s][n][1] for s in streams]
            got = new.step(streams, bgr, d16)                               # uint16 arrays go up as DVO_DEPTH_U16
            want = old.step(streams, bgr, [d.astype(np.float32) for d in d16])
            for name in ("T", "norms", "updates", "event"):
                assert same_bits(got[name], want[name]), (n, name, got[name], want[name])
            assert got["event"].tolist() == [1 if n % 4 == 0 else 0] * 3, (n, got["event"])
            assert new.stats() == old.stats(), (n, new.stats(), old.stats())
        # the depth the engine holds is the sensor's: holes are still 0
        from rgbd_odometry_amd import capi
        lib, h = capi.load_library(), new.context_handle()
        dep = np.zeros(480 * 640, np.float32)
        assert lib.dvo_frame_get_level(h, 0, 0, None, None, None, capi._ptr(dep), None, None) == 0
        assert np.array_equal(dep.reshape(640, 480).T, seqs[0][5][1].astype(np.float32))
