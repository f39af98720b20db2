#!/usr/bin/env python3
"""Times of the triangle mesh of a fused volume (include/dvo_amd.h, "the surface as a triangle mesh") on the workload of
tools/tsdf_bench.py: a --dim^3 volume (default 256^3 at 1 cm, trunc 4 cm) fused from 16 640 x 480 depth images of its synthetic room.

  count          dvo_mesh_extract with two zero capacities: the counts alone (the first call of the two-call pattern)
  host_buffers   dvo_mesh_extract into host memory of exactly the counts: the copy back included
  device_buffers the same into device memory (DVO_UPLOAD_DEVICE): only the counts come back
  points         dvo_tsdf_extract_points on the same volume in the same process, host memory of exactly its count: the comparison on the
                 device, because it walks the same words for three of the seven edges

A time is the host clock around one call, which ends in its one synchronisation; one warm-up, then --repeats timed calls: median
(min .. max).  --host also times dvo_mesh_host on one core (twice: counts, then the mesh) and compares the device's mesh with it, byte
for byte.  --configs limits the shapes (for a rocprofv3 --kernel-trace --stats run of its own).  Prints one JSON line.  Needs a HIP
device: there is no fallback."""
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

from tsdf_bench import K4, arc_pose, room, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--min-weight", type=int, default=1)
    ap.add_argument("--configs", default="count,host_buffers,device_buffers,points")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    import torch
    from rgbd_odometry_amd import capi
    if not torch.cuda.is_available():
        sys.exit("tsdf_mesh_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 5:
        sys.exit("--repeats: at least five timed calls")

    n, F = a.dim ** 3, a.frames
    half = 0.5 * a.dim * a.voxel_size
    vol = capi.DvoTsdfVolume.make((a.dim,) * 3, a.voxel_size, (-half, -half, 0.4), 4.0 * a.voxel_size)
    imgs = [room(k) for k in range(F)]
    poses = np.stack([arc_pose(k, F) for k in range(F)])
    out = dict(dim=a.dim, voxel_size=a.voxel_size, voxels=n, volume_bytes=4 * n, frames=F, repeats=a.repeats, min_weight=a.min_weight, calls={})
    configs = [c for c in a.configs.split(",") if c]
    with capi.DvoTsdfVolumes(1, n) as h:
        h.set_volume(0, vol)
        h.integrate([0] * F, imgs, K4, poses)
        lib, nv, nt, npts = h.lib, C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        h._chk(lib.dvo_mesh_extract(h._h, 0, a.min_weight, None, 0, None, 0, C.byref(nv), C.byref(nt), 0))
        h._chk(lib.dvo_tsdf_extract_points(h._h, 0, a.min_weight, None, 0, C.byref(npts)))
        V, T, P = nv.value, nt.value, npts.value
        out.update(vertices=V, triangles=T, points=P, mesh_bytes=12 * (V + T))
        xyz, tri, pts = np.zeros((V, 3), np.float32), np.zeros((T, 3), np.int32), np.zeros((P, 3), np.float32)
        dxyz = torch.zeros((max(V, 1), 3), dtype=torch.float32, device="cuda")
        dtri = torch.zeros((max(T, 1), 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        mesh_call = lambda px, cv, pt, ct, flags: h._chk(lib.dvo_mesh_extract(h._h, 0, a.min_weight, px, cv, pt, ct, C.byref(nv), C.byref(nt), flags))
        calls = dict(count=lambda: mesh_call(None, 0, None, 0, 0),
                     host_buffers=lambda: mesh_call(capi._ptr(xyz), V, capi._ptr(tri), T, 0),
                     device_buffers=lambda: mesh_call(int(dxyz.data_ptr()), V, int(dtri.data_ptr()), T, capi.DVO_UPLOAD_DEVICE),
                     points=lambda: h._chk(lib.dvo_tsdf_extract_points(h._h, 0, a.min_weight, capi._ptr(pts), P, C.byref(npts))))
        for name in configs:
            times = []
            for rep in range(a.repeats + 1):                          # the first is the warm-up
                t0 = time.perf_counter()
                calls[name]()
                t1 = time.perf_counter()
                if rep:
                    times.append(t1 - t0)
            out["calls"][name] = dict(spread(times), launches_syncs=h.stats())
        if a.host:
            mesh_call(capi._ptr(xyz), V, capi._ptr(tri), T, 0)
            words = h.voxels(0)
            t0 = time.perf_counter()
            hv, ht = capi.tsdf_mesh_host(vol, words, a.min_weight)
            t1 = time.perf_counter()
            dev = (dxyz[:V].cpu().numpy(), dtri[:T].cpu().numpy()) if "device_buffers" in configs else (xyz, tri)
            out["host_definition"] = dict(ms_one_core_counts_then_mesh=1e3 * (t1 - t0), seen_voxels=int((words != 0).sum()),
                                          equal_host_buffers=bool(hv.tobytes() == xyz.tobytes() and ht.tobytes() == tri.tobytes()),
                                          equal_device_buffers=bool(hv.tobytes() == dev[0].tobytes() and ht.tobytes() == dev[1].tobytes()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
