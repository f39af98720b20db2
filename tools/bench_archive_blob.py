"""Time of dvo_tracker_archive_export and dvo_tracker_archive_import on a few hundred 640x480 key frames (include/dvo_amd.h, "export
and import of the key-frame archive"; profiles/tracker_archive_blob/README.md).

Four streams of 640x480 camera frames (frame_gen.camera_frame), every stream reset before every tick so that each of its frames is a first frame and becomes a key
frame, TICKS ticks into a ring of 256 slots with place descriptors at the coarsest level.  Then the whole archive is exported into a
caller's buffer and imported into a second tracker, through the C ABI itself (no numpy copies in the timed region).  An export ends in its
own synchronisation; an import returns with its scatter launch in flight, so the timed region of an import ends with dvo_synchronize.
Per call: ROUNDS rounds of WARM untimed and REPS timed calls; the figure is the median over the rounds of each round's median, lo / hi
the smallest and largest round median.  GB/s = blob bytes / that time.

The numbers are recorded, not asserted: there is no earlier path to compare against.  What is asserted are the launch and
synchronisation counts the header promises: (1, 1) per export, (2, 1) per import.

    python tools/bench_archive_blob.py [--ticks N] [--label NAME] [--out FILE.jsonl]"""
import argparse
import ctypes
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--ticks", type=int, default=64)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
from rgbd_odometry_amd import DvoTracker, capi  # noqa: E402
from rgbd_odometry_amd.frame_gen import camera_frame  # noqa: E402

ROWS, COLS, NL, S, SLOTS = 480, 640, 3, 4, 256
WARM, REPS, ROUNDS = 3, 20, 5
DISTINCT = 8
frames = [[camera_frame(500 + s, ROWS, COLS, shift=(i, -2 * i)) for i in range(DISTINCT)] for s in range(S)]


def make():
    tr = DvoTracker(S, iters=[8, 8, 8], rows=ROWS, cols=COLS, n_levels=NL, first_shift=0)
    tr.set_intrinsics(525.0, 525.0, 319.5, 239.5)
    tr.set_archive(SLOTS, 1)
    tr.set_places(NL - 1)
    return tr


def timed(fn):
    rounds = []
    for _ in range(ROUNDS):
        for _ in range(WARM):
            fn()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        rounds.append(float(np.median(ts)) * 1e3)
    return dict(median=round(float(np.median(rounds)), 4), lo=round(min(rounds), 4), hi=round(max(rounds), 4))


lib = capi.load_library()
res = dict(label=args.label, rows=ROWS, cols=COLS, n_levels=NL, streams=S, ticks=args.ticks, slots=SLOTS, warm=WARM, reps=REPS, rounds=ROUNDS)
with make() as A, make() as B:
    for i in range(args.ticks):
        for s in range(S):
            A.reset_stream(s)
        A.step(list(range(S)), [frames[s][i % DISTINCT][0] for s in range(S)], [frames[s][i % DISTINCT][1] for s in range(S)])
    size = A.export_size()
    info = capi.archive_blob_info(A.export_archive())
    res.update(key_frames=info["n_key_frames"], blob_bytes=size, descriptor_bytes=info["D"])
    buf = np.zeros(size, np.uint8)
    got = ctypes.c_size_t()

    def export():
        assert lib.dvo_tracker_archive_export(A._h, 0, None, capi._ptr(buf), size, ctypes.byref(got)) == 0

    res["export_ms"] = timed(export)
    st = A.archive_stats()
    assert (st["last_launches"], st["last_syncs"]) == (capi.DVO_TRACKER_EXPORT_LAUNCHES, 1), st
    res["export_launches_syncs"] = [st["last_launches"], st["last_syncs"]]
    blob = buf.tobytes()
    ids = (ctypes.c_longlong * info["n_key_frames"])()
    n_in = ctypes.c_int()
    ctx = B.context_handle()

    def load():
        assert lib.dvo_tracker_archive_import(B._h, blob, size, ids, len(ids), ctypes.byref(n_in)) == 0
        assert lib.dvo_synchronize(ctx) == 0

    res["import_ms"] = timed(load)
    st = B.archive_stats()
    assert (st["last_launches"], st["last_syncs"]) == (capi.DVO_TRACKER_IMPORT_LAUNCHES, 1), st
    res["import_launches_syncs"] = [st["last_launches"], st["last_syncs"]]
    assert B.export_archive(list(ids)) == blob              # what went in is what comes out
    for k in ("export", "import"):
        res[k + "_GBps"] = round(size / (res[k + "_ms"]["median"] * 1e-3) / 1e9, 3)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
