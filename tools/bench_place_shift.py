"""Time of one dvo_tracker_place_shifts call beside the dvo_tracker_query_places call that produced its candidates, and what the
guess of dvo_tracker_place_guess does to one dvo_tracker_match (include/dvo_amd.h, "shift search on place descriptors";
profiles/tracker_place_shift/README.md).

Timing.  K = 256 streams of 640x480 camera frames (frame_gen.camera_frame, SCENES distinct scenes shared among the streams), 4 levels,
descriptors of the coarsest level (60 x 80, D = 4800).  Tick 0 archives one key frame per stream; at tick 1 stream s sees the scene of
stream s + 1, moved.  Then one query of all streams with k = 8 and one shift search of radius 6 over the 256 x 8 candidates it
returned.  A call ends in its own synchronisation, so the host clock around it is the call's time: ROUNDS rounds of WARM untimed and
REPS timed calls of the C function on arrays made once (shifts_binding_us: the same through DvoTracker.place_shifts_raw); the figure is the median over the rounds of each round's median, lo / hi the smallest and largest round median.

Demonstration.  A tracker of two 320x240 streams (3 levels, descriptors of level 2): stream 0's first frame becomes a key frame, stream
1's current frame is the same frame moved by (-16, 16) camera pixels.  For the candidate (stream 1, key frame of stream 0): the shift
record, then dvo_tracker_match + dvo_tracker_verify from the identity and from the guess of the best shift.  Recorded, not judged.

    python tools/bench_place_shift.py [--what both|time|demo] [--streams K] [--label NAME] [--out FILE.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--what", default="both", choices=("both", "time", "demo"))
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.package_root)

import numpy as np  # noqa: E402
import rgbd_odometry_amd  # noqa: E402
from rgbd_odometry_amd import DvoTracker  # noqa: E402
from rgbd_odometry_amd.capi import DvoTrackerPlace, DvoTrackerPlaceShift  # noqa: E402
from rgbd_odometry_amd.frame_gen import camera_frame  # noqa: E402

KQ, RADIUS, SCENES = 8, 6, 16
WARM, REPS, ROUNDS = 5, 40, 5
res = dict(label=args.label, package=os.path.dirname(rgbd_odometry_amd.__file__), warm=WARM, reps=REPS, rounds=ROUNDS)


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
        rounds.append(float(np.median(ts)) * 1e6)
    return dict(median=round(float(np.median(rounds)), 2), lo=round(min(rounds), 2), hi=round(max(rounds), 2))


if args.what in ("both", "time"):
    rows, cols, nl, S = 480, 640, 4, args.streams
    scenes = [[camera_frame(500 + j, rows, cols, shift=sh) for sh in ((0, 0), (-16, 16))] for j in range(SCENES)]
    caps = [90000, 30000, 9000, 3000]      # these scenes have more edge pixels than the archive's default slot (1/8 of a level) holds
    with DvoTracker(S, iters=[8] * nl, rows=rows, cols=cols, n_levels=nl, first_shift=0, points_capacity=caps) as tr:
        tr.set_intrinsics(525.0, 525.0, 319.5, 239.5)
        tr.set_archive(2 * S, 32, caps)
        tr.set_places(nl - 1)
        streams = list(range(S))
        tr.step(streams, [scenes[s % SCENES][0][0] for s in streams], [scenes[s % SCENES][0][1] for s in streams])
        tr.step(streams, [scenes[(s + 1) % SCENES][1][0] for s in streams], [scenes[(s + 1) % SCENES][1][1] for s in streams])
        found = tr.places(streams, KQ)
        cs = [s for s, row in zip(streams, found) for _ in row]
        ck = [e["key_id"] for row in found for e in row]
        res.update(streams=S, k=KQ, radius=RADIUS, rows=rows, cols=cols, level=nl - 1, candidates=len(cs), archive=tr.archive_stats())
        if len(cs) != S * KQ:
            raise SystemExit("the query returned %d candidates, not %d: %r" % (len(cs), S * KQ, res["archive"]))
        # the C calls themselves, on arrays made once: the Python binding's marshalling of 2048 candidates costs more than the call
        n = len(cs)
        a_s, a_out, a_found = (C.c_int * S)(*streams), (DvoTrackerPlace * (S * KQ))(), (C.c_int * S)()
        a_cs, a_ck, a_rec = (C.c_int * n)(*cs), (C.c_longlong * n)(*ck), (DvoTrackerPlaceShift * n)()
        lib, h = tr.lib, tr._h
        assert lib.dvo_tracker_query_places(h, S, a_s, KQ, 0, a_out, a_found) == 0
        res["query_us"] = timed(lambda: lib.dvo_tracker_query_places(h, S, a_s, KQ, 0, a_out, a_found))
        st = tr.archive_stats()
        res["query_launches_syncs"] = [st["last_launches"], st["last_syncs"]]
        for key, radius in (("shifts_us", RADIUS), ("shifts_r0_us", 0), ("shifts_r8_us", 8)):
            assert lib.dvo_tracker_place_shifts(h, n, a_cs, a_ck, radius, a_rec) == 0
            res[key] = timed(lambda: lib.dvo_tracker_place_shifts(h, n, a_cs, a_ck, radius, a_rec))
        st = tr.archive_stats()
        res["shifts_launches_syncs"] = [st["last_launches"], st["last_syncs"]]
        res["shifts_binding_us"] = timed(lambda: tr.place_shifts_raw(cs, ck, RADIUS))
        rec = tr.place_shifts_raw(cs, ck, RADIUS)
        # what the search says about the query's own ranking: per stream, the rank (by distance) of the candidate with the smallest best-shift SAD
        best_rank = [int(np.argmin(rec["sad"][i * KQ:(i + 1) * KQ])) for i in range(S)]
        res["best_shift_sad_rank_histogram"] = np.bincount(best_rank, minlength=KQ).tolist()
        res["shift_histogram"] = sorted(((int(dy), int(dx)), int(n)) for (dy, dx), n in
                                        zip(*np.unique(np.stack([rec["dy"], rec["dx"]], 1), axis=0, return_counts=True)))[:12]

if args.what in ("both", "demo"):
    rows, cols, nl, level = 240, 320, 3, 2
    key = camera_frame(900, rows, cols, shift=(0, 0), holes=True)
    moved = camera_frame(900, rows, cols, shift=(-16, 16), holes=True)
    with DvoTracker(2, iters=[8] * nl, rows=rows, cols=cols, n_levels=nl, first_shift=0) as tr:
        tr.set_intrinsics(262.5, 262.5, 159.75, 119.75)
        tr.set_archive(4, 2)
        tr.set_places(level)
        tr.step([0, 1], [key[0], moved[0]], [key[1], moved[1]])
        kid = tr.key_frame_id(0)
        shift = tr.place_shifts([1], [kid], RADIUS)[0]
        R0, t0 = tr.place_guess(1, shift["dy"], shift["dx"])
        demo = dict(shift=shift, query_distance=[e for e in tr.places([1], 4)[0] if e["key_id"] == kid], guess_R0=R0.tolist())
        for name, (Rg, tg) in (("identity", (np.eye(3), np.zeros(3))), ("place_guess", (R0, t0))):
            R, t, recs = tr.match([1], [kid], Rg[None], tg[None])
            start = tr.score([1], [kid], 0, Rg[None], tg[None])[0]
            ver = tr.verify([1], [kid], 0, R, t)[0]
            demo[name] = dict(start=dict(n_points=start["n_points"], n_visible=start["n_visible"], sum_eps2=start["sum_eps2"]),
                              match=dict(n_points=recs[0]["n_points"], n_visible=recs[0]["n_visible"], sum_eps2=recs[0]["sum_eps2"]),
                              R=R[0].tolist(), t=t[0].tolist(), verify=ver)
        res["demo"] = demo

line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
