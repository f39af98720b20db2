#!/usr/bin/env python3
"""Times of the frame-to-model alignment (include/dvo_amd.h, "frame-to-model alignment") at camera resolution: 640 x 480 views of the
analytic corner scene of tests/icp_reference.py -- 16-bit now depth, float model depth and normals, 16 distinct views (model pose,
motion and holes vary), repeated as separate device copies up to the largest batch -- aligned with the default parameters (three
levels, 19 updates and the record's sweep: 20 sweeps) from device inputs (DVO_UPLOAD_DEVICE).

  --views 1,16,256   the batches: that many views in one call

A time is the host clock around the call, which ends in its one synchronisation; one warm-up, then --repeats timed calls: median
(min .. max), and the same divided by the call's sweeps.  --verify compares the first 16 views of the largest batch with
dvo_icp_align_host, byte for byte.  Prints one JSON line.  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tsdf_bench import COLS, ROWS, spread  # noqa: E402

DISTINCT = 16


def make_views():
    import icp_reference as ir
    motions, models = ["shift", "turn", "both"], ["front", "aside"]
    return [ir.make_view("corner", (ROWS, COLS), models[k % 2], motions[k % 3], holes=0.03, seed=100 + k) for k in range(DISTINCT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="1,16,256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    import torch
    from rgbd_odometry_amd import capi
    if not torch.cuda.is_available():
        sys.exit("icp_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 5:
        sys.exit("--repeats: at least five timed calls")
    batches = [int(v) for v in a.views.split(",") if v]
    views = make_views()
    prm = capi.DvoIcpParams.default()
    out = dict(rows=ROWS, cols=COLS, distinct_views=DISTINCT, repeats=a.repeats, sweeps=prm.sweeps(), now_format="u16", model_format="f32", batches={})
    most = max(batches)
    up = lambda arr: torch.from_numpy(np.array(arr).view(np.int16) if arr.dtype == np.uint16 else np.array(arr)).cuda()
    now = [up(views[k % DISTINCT]["now_u16"]) for k in range(most)]
    model = [up(views[k % DISTINCT]["model_f32"]) for k in range(most)]
    nrm = [up(views[k % DISTINCT]["normals"]) for k in range(most)]
    K = np.array([views[k % DISTINCT]["K"] for k in range(most)])
    Pm = np.stack([views[k % DISTINCT]["model_pose"] for k in range(most)])
    torch.cuda.synchronize()
    out["device_bytes_per_view"] = int(now[0].numel() * 2 + model[0].numel() * 4 + nrm[0].numel() * 4)
    with capi.DvoIcp(most) as h:
        for n in batches:
            times = []
            for rep in range(a.repeats + 1):                      # the first is the warm-up
                t0 = time.perf_counter()
                poses, recs = h.align(now[:n], model[:n], nrm[:n], K[:n], Pm[:n], Pm[:n], prm, device=True)
                t1 = time.perf_counter()
                if rep:
                    times.append(t1 - t0)
            res = dict(per_call=spread(times), per_sweep={k: v / prm.sweeps() for k, v in spread(times).items()}, launches_syncs=h.stats(),
                       status_counts=np.bincount(recs["status"], minlength=3).tolist(), updates_min=int(recs["iterations"].min()),
                       count_mean=float(recs["count"].mean()), rms_mean=float(recs["rms"].mean()))
            out["batches"][str(n)] = res
        if a.verify:
            n = min(most, DISTINCT)
            poses, recs = h.align(now[:n], model[:n], nrm[:n], K[:n], Pm[:n], Pm[:n], prm, device=True)
            t0 = time.perf_counter()
            want_poses, want = capi.icp_align_host([v["now_u16"] for v in views[:n]], [v["model_f32"] for v in views[:n]], [v["normals"] for v in views[:n]],
                                                   K[:n], Pm[:n], Pm[:n], prm)
            import icp_reference as ir
            errs = [ir.pose_errors(poses[k], views[k]["true_pose"]) for k in range(n)]
            out["verify"] = dict(views=n, equal=bool(poses.tobytes() == want_poses.tobytes() and recs.tobytes() == want.tobytes()),
                                 host_definition_ms_one_core_per_view=1e3 * (time.perf_counter() - t0) / n,
                                 worst_rotation_error_rad=max(e[0] for e in errs), worst_translation_error_m=max(e[1] for e in errs))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
