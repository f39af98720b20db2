"""Time of one dvo_tracker_verify call beside one dvo_tracker_score call on the same candidates (include/dvo_amd.h, "depth
verification of loop-closure candidates"; profiles/tracker_verify/README.md).

Four streams of 640x480 camera frames (frame_gen.camera_frame), two ticks, every key frame archived; then n = 1, 4 and 16 candidates
(stream i % 4 against a key frame of its own or of a neighbour) at level 0 and the identity pose.  A call ends in its own
synchronisation, so the host clock around it is the call's time: per n and call, ROUNDS rounds of WARM untimed and REPS timed calls;
the figure is the median over the rounds of each round's median, lo / hi are the smallest and largest round median (the spread).

    python tools/bench_verify.py [--what both|score|verify] [--package-root DIR] [--label NAME] [--out FILE.jsonl]

--package-root: the directory holding the rgbd_odometry_amd package to measure (default: this tree).  A build of an earlier commit
measured this way gives the yardstick; run the two alternately, each in a process of its own."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--what", default="both", choices=("both", "score", "verify"))
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.package_root)

import numpy as np  # noqa: E402
import rgbd_odometry_amd  # noqa: E402
from rgbd_odometry_amd import DvoTracker  # noqa: E402
from rgbd_odometry_amd.frame_gen import camera_frame  # noqa: E402

ROWS, COLS, NL, S, M = 480, 640, 3, 4, 16
WARM, REPS, ROUNDS = 30, 300, 5
frames = [[camera_frame(500 + s, ROWS, COLS, shift=(i, -2 * i)) for i in range(2)] for s in range(S)]
res = dict(label=args.label, package=os.path.dirname(rgbd_odometry_amd.__file__), rows=ROWS, cols=COLS, level=0, warm=WARM, reps=REPS,
           rounds=ROUNDS)
with DvoTracker(S, iters=[8, 8, 8], rows=ROWS, cols=COLS, n_levels=NL, first_shift=0) as tr:
    tr.set_intrinsics(525.0, 525.0, 319.5, 239.5)
    tr.set_archive(16, M)
    for i in range(2):
        tr.step(list(range(S)), [frames[s][i][0] for s in range(S)], [frames[s][i][1] for s in range(S)])
    keys = [tr.key_frame_id(s) for s in range(S)]
    res["n_points"] = [tr.archive_info(k)["n_points"][0] for k in keys]
    for n in (1, 4, 16):
        streams = [i % S for i in range(n)]
        kids = [keys[(i + i // S) % S] for i in range(n)]
        Rn, tn = np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3))
        for w in [w for w in ("score", "verify") if args.what in (w, "both")]:
            fn = getattr(tr, w)
            rounds = []
            for _ in range(ROUNDS):
                for _ in range(WARM):
                    fn(streams, kids, 0, Rn, tn)
                ts = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    fn(streams, kids, 0, Rn, tn)
                    ts.append(time.perf_counter() - t0)
                rounds.append(float(np.median(ts)) * 1e6)
            res["%s_n%d_us" % (w, n)] = dict(median=round(float(np.median(rounds)), 2), lo=round(min(rounds), 2), hi=round(max(rounds), 2))
            st = tr.archive_stats()
            res["%s_n%d_launches_syncs" % (w, n)] = [st["last_launches"], st["last_syncs"]]
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
