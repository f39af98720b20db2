#!/usr/bin/env python3
"""Times of colour in the map (include/dvo_amd.h, "colour in the map") on the workload of tools/tsdf_bench.py: a --dim^3 volume (default
256^3 at 1 cm, trunc 4 cm), 16 640 x 480 depth images of its synthetic room from poses on a small arc, plus seeded bgr8 images.

  plain     dvo_tsdf_integrate: 1 frame in 1 call and 16 frames in 1 call, device images and host images
  colour    dvo_colour_integrate on the same shapes (the handle has its colour pool)
  raycast   dvo_raycast_views and dvo_colour_raycast_views: the 16 poses as 640 x 480 views of the fused volume, 16-bit depth, device outputs
  mesh      dvo_mesh_extract and dvo_colour_mesh_extract of the fused volume into device buffers of exactly the counts

A time is the host clock around one call, which ends in its one synchronisation; the volume is cleared before every timed integration
(not timed); one warm-up, then --repeats timed calls: median (min .. max).  Algorithmic bytes of an integration: 8 per voxel for the
words (one read, one write) and, with colour, 16 more for the colour words, plus the images -- an upper bound, a group that did not
change is not stored.  --package-root runs the `plain` shapes on another tree's library and binding (the parent commit's, for the
comparison).  --verify compares the device state of the 16-frame colour call with dvo_colour_integrate_host, byte for byte.  --configs
and --counts limit the shapes (for a rocprofv3 --kernel-trace --stats run of its own; --counts 16 leaves one integration shape per
kernel).  Prints one JSON line.  Needs a HIP device: there is no fallback."""
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


def colour_image(seed):
    """bgr8: smooth ramps with a little seeded noise"""
    v, u = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    base = np.stack([(u // 3 + seed * 5) % 256, (v // 2 + 2 * seed) % 256, (u + v) // 5 % 256], axis=-1)
    noise = np.random.RandomState(100 + seed).randint(0, 8, size=base.shape)
    return np.clip(base + noise, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="plain,colour,raycast,mesh")
    ap.add_argument("--counts", default="1,16", help="frames per integration call: the shapes of plain and colour")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from rgbd_odometry_amd import capi
    if not torch.cuda.is_available():
        sys.exit("tsdf_colour_bench.py needs a HIP device: the engine has no CPU fallback")
    if a.repeats < 7:
        sys.exit("--repeats: at least seven timed calls")
    configs = [c for c in a.configs.split(",") if c]
    has_colour = hasattr(capi.DvoTsdfVolumes, "enable_colour")
    if not has_colour and configs != ["plain"]:
        sys.exit("this library has no colour: --configs plain")

    n, F = a.dim ** 3, a.frames
    half = 0.5 * a.dim * a.voxel_size
    vol = capi.DvoTsdfVolume.make((a.dim,) * 3, a.voxel_size, (-half, -half, 0.4), 4.0 * a.voxel_size)
    depth = [room(k) for k in range(F)]
    image = [colour_image(k) for k in range(F)]
    poses = np.stack([arc_pose(k, F) for k in range(F)])
    d_dev = [torch.from_numpy(i.view(np.int16)).cuda().contiguous() for i in depth]
    i_dev = [torch.from_numpy(i).cuda().contiguous() for i in image]
    torch.cuda.synchronize()
    out = dict(library_of=os.path.relpath(os.path.abspath(a.package_root), ROOT), dim=a.dim, voxel_size=a.voxel_size, voxels=n, frames=F, rows=ROWS, cols=COLS,
               repeats=a.repeats, calls={})

    def timed(name, call, before=None, **more):
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

    with capi.DvoTsdfVolumes(1, n) as h:
        h.set_volume(0, vol)
        if has_colour and configs != ["plain"]:
            h.enable_colour()
        clear = lambda: h.clear(0)
        for count in [int(c) for c in a.counts.split(",") if c]:
            f = list(range(count))
            for key, device in (("device_images", True), ("host_images", False)):
                D, I = ([d_dev[i] for i in f], [i_dev[i] for i in f]) if device else ([depth[i] for i in f], [image[i] for i in f])
                if "plain" in configs:
                    timed("plain_%d_%s" % (count, key), lambda: h.integrate([0] * count, D, K4, poses[f], device=device), clear,
                          algorithmic_bytes=8 * n + count * ROWS * COLS * 2)
                if "colour" in configs:
                    timed("colour_%d_%s" % (count, key), lambda: h.integrate_colour([0] * count, D, I, K4, poses[f], image_format="bgr8", device=device),
                          clear, algorithmic_bytes=24 * n + count * ROWS * COLS * 5)
        if "colour" in configs and a.verify:
            words, colours = h.voxels(0), h.get_colours(0)
            t0 = time.perf_counter()
            hw, hc = capi.tsdf_integrate_colour_host(vol, None, None, depth, image, K4, poses, image_format="bgr8")
            out["verify_colour_16"] = dict(equal=bool(np.array_equal(words, hw) and np.array_equal(colours, hc)), updated_voxels=int((hw != 0).sum()),
                                           coloured_voxels=int((hc != 0).sum()), host_definition_ms_one_core=1e3 * (time.perf_counter() - t0))
        if "raycast" in configs or "mesh" in configs:
            clear()
            h.integrate_colour([0] * F, d_dev, i_dev, K4, poses, image_format="bgr8", device=True)
        if "raycast" in configs:
            timed("raycast_%d_views" % F, lambda: h.raycast([0] * F, K4, poses, ROWS, COLS, fmt="u16", device=True))
            timed("raycast_colour_%d_views" % F, lambda: h.raycast([0] * F, K4, poses, ROWS, COLS, fmt="u16", device=True, image_format="bgr8"))
            d, img = h.raycast([0] * F, K4, poses, ROWS, COLS, fmt="u16", device=True, image_format="bgr8")
            out["raycast_hit_pixels"] = int((d != 0).sum().item())
            out["raycast_coloured_pixels"] = int((img.to(torch.int32).sum(dim=-1) != 0).sum().item())
        if "mesh" in configs:
            lib, nv, nt = h.lib, C.c_longlong(0), C.c_longlong(0)
            h._chk(lib.dvo_mesh_extract(h._h, 0, 1, None, 0, None, 0, C.byref(nv), C.byref(nt), 0))
            V, T = nv.value, nt.value
            xyz = torch.zeros((max(V, 1), 3), dtype=torch.float32, device="cuda")
            rgb = torch.zeros((max(V, 1), 3), dtype=torch.uint8, device="cuda")
            tri = torch.zeros((max(T, 1), 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            px, pc, pt = int(xyz.data_ptr()), int(rgb.data_ptr()), int(tri.data_ptr())
            timed("mesh", lambda: h._chk(lib.dvo_mesh_extract(h._h, 0, 1, px, V, pt, T, C.byref(nv), C.byref(nt), capi.DVO_UPLOAD_DEVICE)),
                  vertices=V, triangles=T)
            timed("mesh_colour", lambda: h._chk(lib.dvo_colour_mesh_extract(h._h, 0, 1, px, pc, V, pt, T, C.byref(nv), C.byref(nt), capi.DVO_UPLOAD_DEVICE)),
                  vertices=V, triangles=T, coloured_vertices=None)
            out["calls"]["mesh_colour"]["coloured_vertices"] = int((rgb[:V].to(torch.int32).sum(dim=-1) != 0).sum().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
