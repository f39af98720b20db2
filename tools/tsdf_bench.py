#!/usr/bin/env python3
"""Times of depth fusion (include/dvo_amd.h, "depth fusion") at a size a user would run: --dim^3 volumes (default 256^3 at 1 cm) and
640 x 480 16-bit depth images of a synthetic room (a wall at 1.6 m with a nearer box), seen from poses on a small arc.

  1x1     1 frame in 1 call
  16in1   16 frames in 1 call (one volume: the re-fusion shape)
  16x1    16 frames in 16 calls (the same frames, one call each)
  16vol   16 volumes x 1 frame in one call
  extract dvo_tsdf_extract_points of the volume that holds the 16 frames

A time is the host clock around the call, which ends in its one synchronisation; the volumes are cleared before every timed call (not
timed), so that every call does the same work.  Each shape runs once as a warm-up, then --repeats times; median (min .. max).  Every
shape is timed twice: with the images resident on the device (DVO_UPLOAD_DEVICE: the kernel and the descriptor upload) and with host
images (the staging copy and the upload of the images included).  Beside each time: the algorithmic bytes -- 8 per voxel of every
listed volume per call (one read, one write) plus the images -- and what share of the 8 TB/s HBM peak that is over the device-image time.
--verify compares the device words of the 1x1 shape with dvo_tsdf_integrate_host, byte for byte.  --configs limits the shapes (for a
rocprofv3 --kernel-trace --stats run of its own; tools/rocprof_kernel_stats.py reads its database).  Prints one JSON line.
Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
ROWS, COLS = 480, 640
K4 = (525.0, 525.0, 319.5, 239.5)


def room(seed):
    """16-bit millimetres: a wall at 1600 mm, a box at 1100 mm, 3 % holes"""
    d = np.full((ROWS, COLS), 1600, np.uint16)
    d[140:340, 200:440] = 1100
    d[np.random.RandomState(seed).rand(ROWS, COLS) < 0.03] = 0
    return d


def arc_pose(k, n):
    """camera k of n on a small arc around the y axis, looking at the room: 12 doubles {R column-major, t}, camera to world"""
    a = 0.3 * (k / max(n - 1, 1) - 0.5)
    c, s = np.cos(a), np.sin(a)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    t = np.array([-0.8 * s, 0.02 * k, 0.0])
    return np.concatenate([R.T.ravel(), t])


def spread(times):
    t = sorted(times)
    return dict(ms_median=1e3 * t[len(t) // 2], ms_min=1e3 * t[0], ms_max=1e3 * t[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="1x1,16in1,16x1,16vol,extract")
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    import torch
    from rgbd_odometry_amd import capi
    if not torch.cuda.is_available():
        sys.exit("tsdf_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 5:
        sys.exit("--repeats: at least five timed calls")

    n, F = a.dim ** 3, a.frames
    half = 0.5 * a.dim * a.voxel_size
    vol = capi.DvoTsdfVolume.make((a.dim,) * 3, a.voxel_size, (-half, -half, 0.4), 4.0 * a.voxel_size)
    imgs = [room(k) for k in range(F)]
    poses = np.stack([arc_pose(k, F) for k in range(F)])
    dev = [torch.from_numpy(i.view(np.int16)).cuda().contiguous() for i in imgs]
    torch.cuda.synchronize()
    image_bytes = ROWS * COLS * 2
    configs = [c for c in a.configs.split(",") if c]
    n_vols = F if "16vol" in configs else 1
    out = dict(dim=a.dim, voxel_size=a.voxel_size, voxels=n, frames=F, rows=ROWS, cols=COLS, depth_format="u16", repeats=a.repeats,
               hbm_peak_bytes_per_s=HBM_PEAK, shapes={})

    with capi.DvoTsdfVolumes(n_vols, n_vols * n) as h:
        for v in range(n_vols):
            h.set_volume(v, vol)

        def timed(name, calls, volumes_touched):
            """calls: [(volume list, frame index list)] issued one after the other inside one timed window"""
            res = dict(calls=len(calls), frames=sum(len(f) for _, f in calls))
            res["algorithmic_bytes"] = sum(8 * n * len(set(v)) + image_bytes * len(f) for v, f in calls)
            for key, device in (("device_images", True), ("host_images", False)):
                times = []
                for rep in range(a.repeats + 1):              # the first is the warm-up
                    for v in volumes_touched:
                        h.clear(v)
                    t0 = time.perf_counter()
                    for v, f in calls:
                        h.integrate(v, [dev[i] if device else imgs[i] for i in f], K4, poses[f], device=device)
                    t1 = time.perf_counter()
                    if rep:
                        times.append(t1 - t0)
                res[key] = spread(times)
            res["launches_syncs_of_last_call"] = h.stats()
            res["share_of_hbm_peak_device_images"] = res["algorithmic_bytes"] / HBM_PEAK / (1e-3 * res["device_images"]["ms_median"])
            res["algorithmic_GB_per_s_device_images"] = res["algorithmic_bytes"] / (1e-3 * res["device_images"]["ms_median"]) / 1e9
            out["shapes"][name] = res

        every = list(range(F))
        if "1x1" in configs:
            timed("1x1", [([0], [0])], [0])
            if a.verify:
                words = h.voxels(0)
                t0 = time.perf_counter()
                want = capi.tsdf_integrate_host(vol, None, imgs[:1], K4, poses[:1])
                out["verify_1x1"] = dict(equal=bool(np.array_equal(words, want)), updated_voxels=int((want != 0).sum()),
                                         host_definition_ms_one_core=1e3 * (time.perf_counter() - t0))
        if "16vol" in configs:
            timed("16vol", [(every, every)], every)
        if "16x1" in configs:
            timed("16x1", [([0], [i]) for i in every], [0])
        if "16in1" in configs or "extract" in configs:
            timed("16in1", [([0] * F, every)], [0])
            out["updated_voxels_16in1"] = int((h.voxels(0) != 0).sum())
        if "extract" in configs:
            pts, count = h.points(0, 1)
            times = []
            for rep in range(a.repeats + 1):
                t0 = time.perf_counter()
                _, c2 = h.points(0, 1, capacity=count)
                t1 = time.perf_counter()
                if rep:
                    times.append(t1 - t0)
            assert c2 == count
            res = spread(times)
            res.update(points=int(count), launches_syncs=h.stats(), algorithmic_bytes=8 * n + 12 * int(count))      # the words are read by the count and by the write pass
            out["shapes"]["extract"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
