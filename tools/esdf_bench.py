#!/usr/bin/env python3
"""Times of the distance fields (include/dvo_amd.h, "distance fields") on the workload of tools/tsdf_bench.py: a --dim^3 volume (default
256^3 at 1 cm, trunc 4 cm) fused from 16 640 x 480 depth images of its synthetic room from poses on a small arc.

  base      dvo_tsdf_integrate (16 frames in 1 call, device images), dvo_raycast_views (the 16 poses as 640 x 480 views, 16-bit depth,
            device outputs) and dvo_mesh_extract (device buffers of exactly the counts) on a handle that did NOT enable the distance
            fields: the calls an A/B against the parent commit compares (--package-root runs them on another tree's library and binding)
  esdf      dvo_esdf_update of the fused volume in both `sites` modes, dvo_esdf_get_distances of one plane and of the whole volume
            (device output), dvo_esdf_query of 4096 points (device memory), and with --host dvo_esdf_host on one core

A time is the host clock around one call, which ends in its one synchronisation; the volume is cleared before every timed integration
(not timed); one warm-up, then --repeats timed calls: median (min .. max).  --verify compares the device words of the last update with
dvo_esdf_host, byte for byte.  Prints one JSON line.  Needs a HIP device: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tsdf_bench import COLS, K4, ROWS, arc_pose, room, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="base,esdf")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from rgbd_odometry_amd import capi
    if not torch.cuda.is_available():
        sys.exit("esdf_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 7:
        sys.exit("--repeats: at least seven timed calls")
    configs = [c for c in a.configs.split(",") if c]
    if "esdf" in configs and not hasattr(capi.DvoTsdfVolumes, "enable_esdf"):
        sys.exit("this library has no distance fields: --configs base")

    n, F = a.dim ** 3, a.frames
    half = 0.5 * a.dim * a.voxel_size
    vol = capi.DvoTsdfVolume.make((a.dim,) * 3, a.voxel_size, (-half, -half, 0.4), 4.0 * a.voxel_size)
    depth = [room(k) for k in range(F)]
    poses = np.stack([arc_pose(k, F) for k in range(F)])
    d_dev = [torch.from_numpy(i.view(np.int16)).cuda().contiguous() for i in depth]
    torch.cuda.synchronize()
    out = dict(library_of=os.path.relpath(os.path.abspath(a.package_root), ROOT), dim=a.dim, voxel_size=a.voxel_size, voxels=n, frames=F, rows=ROWS, cols=COLS,
               repeats=a.repeats, calls={})

    def timed(h, name, call, before=None, **more):
        times = []
        for rep in range(a.repeats + 1):                                  # the first is the warm-up
            if before:
                before()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if rep:
                times.append(t1 - t0)
        out["calls"][name] = dict(spread(times), launches_syncs=h.stats(), **more)

    if "base" in configs:
        with capi.DvoTsdfVolumes(1, n) as h:
            h.set_volume(0, vol)
            timed(h, "integrate_%d_device_images" % F, lambda: h.integrate([0] * F, d_dev, K4, poses, device=True), lambda: h.clear(0))
            timed(h, "raycast_%d_views" % F, lambda: h.raycast([0] * F, K4, poses, ROWS, COLS, fmt="u16", device=True))
            lib, nv, nt = h.lib, C.c_longlong(0), C.c_longlong(0)
            h._chk(lib.dvo_mesh_extract(h._h, 0, 1, None, 0, None, 0, C.byref(nv), C.byref(nt), 0))
            V, T = nv.value, nt.value
            xyz = torch.zeros((max(V, 1), 3), dtype=torch.float32, device="cuda")
            tri = torch.zeros((max(T, 1), 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            px, pt = int(xyz.data_ptr()), int(tri.data_ptr())
            timed(h, "mesh", lambda: h._chk(lib.dvo_mesh_extract(h._h, 0, 1, px, V, pt, T, C.byref(nv), C.byref(nt), capi.DVO_UPLOAD_DEVICE)),
                  vertices=V, triangles=T)
    if "esdf" in configs:
        with capi.DvoTsdfVolumes(1, n) as h:
            h.set_volume(0, vol)
            h.enable_esdf()
            h.integrate([0] * F, d_dev, K4, poses, device=True)
            words = None
            for sites, key in ((capi.DVO_ESDF_SITES_SURFACE, "surface"), (capi.DVO_ESDF_SITES_SURFACE_AND_UNKNOWN, "surface_and_unknown")):
                p = capi.DvoEsdfParams.default(sites=sites)
                timed(h, "update_" + key, lambda: h.update_esdf([0], p))
                words = h.esdf_words(0)
                d2 = words & capi.DVO_ESDF_NO_SITE
                out["calls"]["update_" + key].update(sites=int((d2 == 0).sum()), unknown=int((words >> 31).sum()), inside=int(((words >> 30) & 1).sum()),
                                                     max_d2=int(d2.max()), mean_distance_voxels=float(np.sqrt(d2.astype(np.float64)).mean()))
                if a.verify or a.host:
                    t0 = time.perf_counter()
                    hw = capi.esdf_host(vol, h.voxels(0), p)
                    out["calls"]["update_" + key].update(host_definition_ms_one_core=1e3 * (time.perf_counter() - t0), equal=bool(np.array_equal(hw, words)))
            timed(h, "distances_one_plane", lambda: h.esdf_distances(0, a.dim // 2, 1, device=True))
            timed(h, "distances_whole_volume", lambda: h.esdf_distances(0, 0, a.dim, device=True))
            rng = np.random.RandomState(1)
            P = np.array([-half, -half, 0.4]) + a.voxel_size * (a.dim - 1) * rng.uniform(0.0, 1.0, size=(4096, 3))
            Pd = torch.from_numpy(P).cuda().contiguous()
            torch.cuda.synchronize()
            timed(h, "query_4096_points", lambda: h.esdf_query(0, Pd, device=True))
            rec = np.frombuffer(h.esdf_query(0, Pd, device=True).cpu().numpy().tobytes(), capi.ESDF_SAMPLE_DTYPE)
            out["query_found"] = int((rec["status"] == capi.DVO_ESDF_FOUND).sum())
            if a.verify:
                out["query_equal"] = bool(rec.tobytes() == capi.esdf_query_host(vol, words, P).tobytes())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
