#!/usr/bin/env python3
"""Times of the depth front end (include/dvo_amd.h, "preparing a depth frame") at camera resolution, on the views of tools/icp_bench.py:
640 x 480 now-depth images of the analytic corner scene, 16 distinct ones repeated as separate device copies up to the largest batch.

  dvo_icp_prepare with the default parameters (7 x 7 window), device in and out (DVO_UPLOAD_DEVICE), 16-bit and float input, with
  normals: per call and per frame;
  dvo_icp_align_gated (normal_cos_min 0.9, the normals prepare wrote) beside dvo_icp_align on the same views, default parameters.

  --frames 1,16,256   the batches: that many images or views in one call

A time is the host clock around the C call, which ends in its one synchronisation; one warm-up, then --repeats timed calls: median
(min .. max).  The output buffers are allocated once, before the clock starts.  --verify compares the first 16 images of the largest
batch with dvo_icp_prepare_host and their gated alignment with dvo_icp_align_gated_host, byte for byte.  Prints one JSON line.  Needs a
HIP device: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icp_bench import DISTINCT, make_views  # noqa: E402
from tsdf_bench import COLS, ROWS, spread  # noqa: E402

COS_MIN = 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,16,256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    import torch
    from rgbd_odometry_amd import capi
    if not torch.cuda.is_available():
        sys.exit("icp_prepare_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 5:
        sys.exit("--repeats: at least five timed calls")
    batches = [int(v) for v in a.frames.split(",") if v]
    most = max(batches)
    views = make_views()
    fp = capi.DvoIcpPrepareParams.default()
    prm = capi.DvoIcpParams.default()
    up = lambda arr: torch.from_numpy(np.array(arr).view(np.int16) if arr.dtype == np.uint16 else np.array(arr)).cuda()
    K = np.array([views[k % DISTINCT]["K"] for k in range(most)])
    Pm = np.stack([views[k % DISTINCT]["model_pose"] for k in range(most)])
    out = dict(rows=ROWS, cols=COLS, distinct_views=DISTINCT, repeats=a.repeats, radius=int(fp.radius), prepare={}, align={})
    filtered = [torch.zeros((ROWS, COLS), dtype=torch.float32, device="cuda") for _ in range(most)]
    normals = [torch.zeros((ROWS, COLS, 3), dtype=torch.float32, device="cuda") for _ in range(most)]
    ptrs = lambda ts, n: (C.c_void_p * n)(*[int(t.data_ptr()) for t in ts[:n]])
    with capi.DvoIcp(most) as h:
        lib = h.lib
        for fmt, code in (("u16", capi.DVO_DEPTH_U16), ("f32", capi.DVO_DEPTH_F32)):
            depth = [up(views[k % DISTINCT]["now_" + fmt]) for k in range(most)]
            torch.cuda.synchronize()
            out["prepare"][fmt] = {}
            for n in batches:
                dp, op, qp = ptrs(depth, n), ptrs(filtered, n), ptrs(normals, n)
                times = []
                for rep in range(a.repeats + 1):                  # the first is the warm-up
                    t0 = time.perf_counter()
                    rc = lib.dvo_icp_prepare(h._h, C.byref(fp), n, code, ROWS, COLS, capi._ptr(K), dp, op, qp, capi.DVO_UPLOAD_DEVICE)
                    t1 = time.perf_counter()
                    h._chk(rc)
                    if rep:
                        times.append(t1 - t0)
                out["prepare"][fmt][str(n)] = dict(per_call=spread(times), per_frame={k: v / n for k, v in spread(times).items()}, launches_syncs=h.stats())
            if a.verify and fmt == "f32":
                n = min(most, DISTINCT)
                want, want_n = capi.icp_prepare_host([v["now_f32"] for v in views[:n]], K[:n], fp)
                out["verify_prepare"] = dict(images=n, equal=bool(all(filtered[k].cpu().numpy().tobytes() == want[k].tobytes() and
                                                                       normals[k].cpu().numpy().tobytes() == want_n[k].tobytes() for k in range(n))))
            del depth
        # `normals` now holds the normals of the float images: the gate's
        now = [up(views[k % DISTINCT]["now_u16"]) for k in range(most)]
        model = [up(views[k % DISTINCT]["model_f32"]) for k in range(most)]
        nrm = [up(views[k % DISTINCT]["normals"]) for k in range(most)]
        torch.cuda.synchronize()
        for n in batches:
            res = {}
            for name, gate in (("ungated", None), ("gated", normals[:n]), ("ungated_again", None)):
                times = []
                for rep in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    poses, recs = h.align(now[:n], model[:n], nrm[:n], K[:n], Pm[:n], Pm[:n], prm, device=True, now_normals=gate, normal_cos_min=COS_MIN)
                    t1 = time.perf_counter()
                    if rep:
                        times.append(t1 - t0)
                res[name] = dict(per_call=spread(times), launches_syncs=h.stats(), status_counts=np.bincount(recs["status"], minlength=3).tolist(),
                                 count_mean=float(recs["count"].mean()), rms_mean=float(recs["rms"].mean()))
            out["align"][str(n)] = res
        if a.verify:
            n = min(most, DISTINCT)
            poses, recs = h.align(now[:n], model[:n], nrm[:n], K[:n], Pm[:n], Pm[:n], prm, device=True, now_normals=normals[:n], normal_cos_min=COS_MIN)
            want_poses, want = capi.icp_align_host([v["now_u16"] for v in views[:n]], [v["model_f32"] for v in views[:n]], [v["normals"] for v in views[:n]],
                                                   K[:n], Pm[:n], Pm[:n], prm, now_normals=[t.cpu().numpy() for t in normals[:n]], normal_cos_min=COS_MIN)
            out["verify_gated"] = dict(views=n, equal=bool(poses.tobytes() == want_poses.tobytes() and recs.tobytes() == want.tobytes()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
