#!/usr/bin/env python3
"""Times of the ray cast of a fused volume (include/dvo_amd.h, "from the map back to depth") on the workload of tools/tsdf_bench.py: a
--dim^3 volume (default 256^3 at 1 cm, trunc 4 cm) fused from 16 640 x 480 depth images of its synthetic room, rendered back from the
same 16 poses.

  16in1   16 views in 1 call
  16x1    the same views, one call each
  1x1     1 view in 1 call

Each shape is timed for 16-bit depth alone and for float depth with normals, with the outputs resident on the device
(DVO_UPLOAD_DEVICE: the view-record upload, the launch and the synchronisation) and with host outputs (the copy back included).  A time
is the host clock around the call(s), which end in their one synchronisation each; one warm-up, then --repeats timed runs: median
(min .. max).  --verify compares view 0 with dvo_raycast_host, byte for byte.  --configs limits the shapes (for a rocprofv3
--kernel-trace --stats run of its own).  Prints one JSON line.  Needs a HIP device: there is no fallback.

--count-gathers needs no device: it fuses the volume with the host definition, marches every --stride-th pixel of every view in numpy
(tests/tsdf_raycast_reference.py) and counts, scaled by stride^2, the samples inside the volume's box and the voxel words the definition
reads for them -- one for a sample whose first corner fails min_weight, eight otherwise, and 48 for the normal of a hit -- which is what
a time is to be held against (profiles/tsdf_raycast/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tsdf_bench import COLS, K4, ROWS, arc_pose, room, spread  # noqa: E402


def count_gathers(a, vol_dict, words, poses):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tsdf_map_reference as tr
    import tsdf_raycast_reference as rr
    nx, ny, nz = vol_dict["dims"]
    W = np.asarray(words, np.uint32)
    u, v = np.meshgrid(np.arange(0, COLS, a.stride, dtype=np.float64), np.arange(0, ROWS, a.stride, dtype=np.float64))
    xn, yn = (u - K4[2]) / K4[0], (v - K4[3]) / K4[1]
    step = rr.STEP_TRUNC * vol_dict["trunc"]
    tot = dict(rays=0, samples_marched=0, samples_in_box=0, words_march=0, hits=0, words_normals=0)
    for pose in poses:
        active = np.ones(u.shape, bool)
        prev_valid, S_prev = np.zeros(u.shape, bool), np.zeros(u.shape)
        k = 0
        tot["rays"] += u.size
        while active.any():
            Z = rr.Z_NEAR + step * float(k)
            if not Z <= rr.Z_FAR:
                break
            g = rr.ray_point(vol_dict, pose, xn, yn, Z)
            fl = [np.floor(x) for x in g]
            box = ((fl[0] >= 0) & (fl[0] + 1 <= nx - 1) & (fl[1] >= 0) & (fl[1] + 1 <= ny - 1) & (fl[2] >= 0) & (fl[2] + 1 <= nz - 1))
            base = (np.where(box, fl[0], 0).astype(np.int64) + nx * (np.where(box, fl[1], 0).astype(np.int64) + ny * np.where(box, fl[2], 0).astype(np.int64)))
            first = tr.word_w(W[base]) >= rr.MIN_WEIGHT
            valid, S = rr.sample(vol_dict, W, rr.MIN_WEIGHT, *g)
            tot["samples_marched"] += int(active.sum())
            tot["samples_in_box"] += int((active & box).sum())
            tot["words_march"] += int((active & box).sum()) + 7 * int((active & box & first).sum())
            end = active & valid & (S <= 0.0)
            tot["hits"] += int((end & prev_valid & (S_prev > 0.0) & (k > 0)).sum())
            active &= ~end
            prev_valid, S_prev = valid, S
            k += 1
    tot["words_normals"] = 48 * tot["hits"]
    scale = a.stride * a.stride
    return dict(stride=a.stride, views=len(poses), scaled_to_all_pixels={k: v * scale for k, v in tot.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="16in1,16x1,1x1")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--count-gathers", action="store_true")
    ap.add_argument("--stride", type=int, default=8)
    a = ap.parse_args()
    from rgbd_odometry_amd import capi

    n, F = a.dim ** 3, a.views
    half = 0.5 * a.dim * a.voxel_size
    geometry = ((a.dim,) * 3, a.voxel_size, (-half, -half, 0.4), 4.0 * a.voxel_size)
    vol = capi.DvoTsdfVolume.make(*geometry)
    imgs = [room(k) for k in range(F)]
    poses = np.stack([arc_pose(k, F) for k in range(F)])
    out = dict(dim=a.dim, voxel_size=a.voxel_size, voxels=n, views=F, rows=ROWS, cols=COLS, repeats=a.repeats, shapes={})

    if a.count_gathers:
        words = capi.tsdf_integrate_host(vol, None, imgs, K4, poses)
        out["gathers"] = count_gathers(a, dict(dims=geometry[0], voxel_size=geometry[1], origin=geometry[2], trunc=geometry[3]), words, poses)
        print(json.dumps(out))
        return

    import torch
    if not torch.cuda.is_available():
        sys.exit("tsdf_raycast_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 5:
        sys.exit("--repeats: at least five timed calls")
    configs = [c for c in a.configs.split(",") if c]
    calls_of = {"16in1": [list(range(F))], "16x1": [[i] for i in range(F)], "1x1": [[0]]}
    with capi.DvoTsdfVolumes(1, n) as h:
        h.set_volume(0, vol)
        h.integrate([0] * F, imgs, K4, poses)
        out["seen_voxels"] = int((h.voxels(0) != 0).sum())
        for name in configs:
            res = dict(calls=len(calls_of[name]), views=sum(len(c) for c in calls_of[name]))
            for fmt, normals in (("u16", False), ("f32", True)):
                for device in (True, False):
                    times = []
                    for rep in range(a.repeats + 1):              # the first is the warm-up
                        t0 = time.perf_counter()
                        for c in calls_of[name]:
                            last = h.raycast([0] * len(c), K4, poses[c], ROWS, COLS, fmt=fmt, normals=normals, device=device)
                        t1 = time.perf_counter()
                        if rep:
                            times.append(t1 - t0)
                    key = "%s%s_%s_outputs" % (fmt, "_normals" if normals else "", "device" if device else "host")
                    res[key] = spread(times)
                    if not device:
                        d = last[0] if normals else last
                        res["hit_share_last_view_" + fmt] = float((d[-1] > 0).mean())
            res["launches_syncs_of_last_call"] = h.stats()
            out["shapes"][name] = res
        if a.verify:
            got = h.raycast([0], K4, poses[:1], ROWS, COLS, fmt="f32", normals=True)
            t0 = time.perf_counter()
            want = capi.tsdf_raycast_host(vol, h.voxels(0), K4, poses[:1], ROWS, COLS, None, "f32", True)
            out["verify_view0_f32_normals"] = dict(equal=bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()),
                                                   hits=int((want[0] > 0).sum()), host_definition_ms_one_core=1e3 * (time.perf_counter() - t0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
