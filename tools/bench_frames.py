#!/usr/bin/env python3
"""Rows f1+f2 measured: camera frames (BGR8 + depth in metres, host memory) -> resident now / reference levels,
batched, and the end-to-end rate frames-in -> poses-out.  Not the headline bench (bench.py); DESIGN.md quotes it.

    python tools/bench_frames.py [--batch 256] [--width 640 --height 480] [--levels 4] [--first-shift 0] [--pinned]
                                 [--image-format bgr8|rgb8|mono8] [--depth-format f32|u16]

--image-format / --depth-format: the sensor format the frames arrive in (dvo_frames_upload_cameras_fmt).  The `formats` block of the
result holds the two rates DESIGN.md section 7 tabulates per format -- now frames in -> poses out against resident references, and full
pairs (reference frame with depth + now frame) in -> poses out -- from pageable memory (the engine's pinned mirror), from HBM and, with
--pinned, from pinned mapped memory pulled by the gather kernel.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--first-shift", type=int, default=0)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pinned", action="store_true", help="frames live in pinned host memory (torch pin_memory)")
    ap.add_argument("--image-format", choices=("bgr8", "rgb8", "mono8"), default="bgr8")
    ap.add_argument("--depth-format", choices=("f32", "u16"), default="f32", help="f32: metres; u16: 16-bit millimetres")
    args = ap.parse_args()
    from rgbd_odometry_amd import frame_gen
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_IDENTITY_START, DVO_UPLOAD_ASYNC, DVO_UPLOAD_DIRECT
    ifmt, dfmt = frame_gen.IMAGE_FORMATS.index(args.image_format), frame_gen.DEPTH_FORMATS.index(args.depth_format)
    bpp, dpp = (1 if args.image_format == "mono8" else 3), (2 if args.depth_format == "u16" else 4)

    B, D = args.batch, min(args.distinct, args.batch)
    ref = [frame_gen.camera_frame(100 + i, args.height, args.width) for i in range(D)]
    now = [frame_gen.camera_frame(100 + i, args.height, args.width, shift=(1 + i % 2, -2)) for i in range(D)]
    ref = [frame_gen.as_format(b, d, args.image_format, args.depth_format) for b, d in ref]
    now = [frame_gen.as_format(b, d, args.image_format, args.depth_format) for b, d in now]

    def hold(a):
        if not args.pinned:
            return a
        t = torch.empty(a.nbytes, dtype=torch.uint8, pin_memory=True)        # bytes: every pixel type, 16-bit depth included
        v = t.numpy().view(a.dtype).reshape(a.shape)
        v[...] = a
        return v
    ref = [(hold(b), hold(d)) for b, d in ref]
    now = [(hold(b), hold(d)) for b, d in now]
    ref_b, ref_d = [ref[i % D][0] for i in range(B)], [ref[i % D][1] for i in range(B)]
    now_b = [now[i % D][0] for i in range(B)]

    ctx = DvoContext(B)
    s = 2.0 ** (-args.first_shift) * args.width / 640.0
    ctx.set_intrinsics(525.0 * s, 525.0 * s, 319.5 * s, 239.5 * s * args.height / 480.0 * 640.0 / args.width)
    ctx.frames_reserve(2 * B)
    iters = [args.iters] * args.levels
    res = {}

    def timed(name, fn, units):
        fn(); ctx.synchronize()                       # warm-up (allocations)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        res[name] = dict(ms=1e3 * dt, per_s=units / dt)

    kw = dict(n_levels=args.levels, first_shift=args.first_shift, flags=DVO_UPLOAD_ASYNC | DVO_UPLOAD_DIRECT,    # the frames sit in pinned host memory that outlives the context
              rgb=args.image_format == "rgb8")
    timed("upload_ref_frames(bgr+depth: H2D, pyramid, Canny)", lambda: ctx.frames_upload_cameras(ref_b, ref_d, first_slot=0, **kw), B)
    timed("upload_now_frames(bgr only: H2D, pyramid, Canny)", lambda: ctx.frames_upload_cameras(now_b, None, first_slot=B, **kw), B)
    timed("frames_as_ref(selectedPts+enlistRefEdgePts)", lambda: ctx.frames_as_ref(0, 0, B), B)
    timed("frames_as_now(EDT+normalise+gradients+texels)", lambda: ctx.frames_as_now(B, 0, B), B)
    timed("align(%s)" % iters, lambda: ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START), B)

    # the node's own wire format: mono8 + mono16 pyramids (RGBDFramePyd), row-major; built here by reading the device pyramid back
    pyr = []
    for i in range(D):
        ctx.frames_upload_cameras([ref[i][0]], [ref[i][1]], first_slot=0, n_levels=args.levels, first_shift=args.first_shift, rgb=kw["rgb"])
        lv = []
        for l in range(args.levels):
            g, d, _, _ = ctx.frame_level(0, l)
            lv.append((hold(np.ascontiguousarray(g)), hold(np.ascontiguousarray(d.astype(np.uint16)))))
        pyr.append(lv)
    pyr_b = [pyr[i % D] for i in range(B)]
    res["config_pyramid_bytes_per_frame"] = int(sum(g.nbytes + d.nbytes for g, d in pyr[0]))
    timed("upload_pyramids(mono8+mono16 row-major: H2D, import, Canny)", lambda: ctx.frames_upload_pyramids(pyr_b, first_slot=0, flags=DVO_UPLOAD_ASYNC | DVO_UPLOAD_DIRECT), B)
    if args.pinned:
        from rgbd_odometry_amd.capi import DVO_UPLOAD_MAPPED as _MAPPED
        timed("upload_pyramids, pinned levels pulled by the gather kernel (DVO_UPLOAD_MAPPED)", lambda: ctx.frames_upload_pyramids(pyr_b, first_slot=0, flags=DVO_UPLOAD_ASYNC | _MAPPED), B)

    def tracking_step():                              # every pair gets a fresh now frame against its resident reference
        ctx.frames_upload_cameras(now_b, None, first_slot=B, **kw)
        ctx.frames_as_now(B, 0, B)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()
    timed("now frame in -> pose out (reference resident)", tracking_step, B)

    def tracking_step_fused():                        # as_now rides in the upload pipeline (now_first_pair)
        ctx.frames_upload_cameras(now_b, None, first_slot=B, now_first_pair=0, **kw)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()
    timed("now frame in -> pose out, as_now inside the upload pipeline", tracking_step_fused, B)

    def tracking_step_chunked(ch=32):                 # same, in chunks: copies of chunk k+1 overlap the kernels of chunk k
        for b in range(0, B, ch):
            n = min(ch, B - b)
            ctx.frames_upload_cameras(now_b[b:b + n], None, first_slot=B + b, **kw)
            ctx.frames_as_now(B + b, b, n)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()
    for ch in (64,):
        timed("now frame in -> pose out, chunks of %d" % ch, lambda ch=ch: tracking_step_chunked(ch), B)

    # the same camera frames as device buffers (DVO_UPLOAD_DEVICE): no PCIe
    import torch as _torch
    dev_now = [_torch.from_numpy(np.ascontiguousarray(now_b[i])).cuda() for i in range(D)]
    dev_ptrs = [dev_now[i % D].data_ptr() for i in range(B)]
    dkw = dict(n_levels=args.levels, first_shift=args.first_shift, first_slot=B, flags=DVO_UPLOAD_ASYNC, image_format=ifmt, depth_format=dfmt)
    timed("now frames in HBM: gather, pyramid, Canny", lambda: ctx.frames_upload_cameras_device(dev_ptrs, None, args.height, args.width, **dkw), B)
    timed("now frames in HBM: gather, pyramid, Canny, EDT -> compact form", lambda: ctx.frames_upload_cameras_device(dev_ptrs, None, args.height, args.width, now_first_pair=0, **dkw), B)

    if args.pinned:      # pinned host buffers are device-accessible: the gather kernel pulls them over PCIe itself (one launch per 32 images)
        from rgbd_odometry_amd.capi import DVO_UPLOAD_MAPPED
        host_ptrs = [now_b[i].ctypes.data for i in range(B)]
        mkw = dict(dkw, flags=DVO_UPLOAD_ASYNC | DVO_UPLOAD_MAPPED)
        timed("now frames in pinned host memory, pulled by the gather kernel: pyramid, Canny", lambda: ctx.frames_upload_cameras_device(host_ptrs, None, args.height, args.width, **mkw), B)

        def tracking_step_zero_copy():
            ctx.frames_upload_cameras_device(host_ptrs, None, args.height, args.width, now_first_pair=0, **mkw)
            ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
            return ctx.get_poses()
        timed("now frame in pinned host memory -> pose out, pulled by the gather kernel", tracking_step_zero_copy, B)

    def tracking_step_device():
        ctx.frames_upload_cameras_device(dev_ptrs, None, args.height, args.width, now_first_pair=0, **dkw)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()
    timed("now frame in HBM -> pose out", tracking_step_device, B)

    def pair_step():                                  # both frames of every pair from the host
        ctx.frames_upload_cameras(ref_b, ref_d, first_slot=0, **kw)
        ctx.frames_upload_cameras(now_b, None, first_slot=B, **kw)
        ctx.frames_as_ref(0, 0, B)
        ctx.frames_as_now(B, 0, B)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()
    timed("frame pair in -> pose out", pair_step, B)

    # per source of the frames: now frames in -> poses out (references resident), and full pairs in -> poses out
    dev_ref = [(_torch.from_numpy(np.ascontiguousarray(ref[i][0])).cuda(), _torch.from_numpy(np.ascontiguousarray(ref[i][1])).cuda()) for i in range(D)]
    sources = {"hbm": ([dev_ref[i % D][0].data_ptr() for i in range(B)], [dev_ref[i % D][1].data_ptr() for i in range(B)], dev_ptrs, dkw)}
    if args.pinned:
        sources["pinned_mapped"] = ([b.ctypes.data for b in ref_b], [d.ctypes.data for d in ref_d], host_ptrs, mkw)
    formats = {}
    for name, (rb, rd, nb, fkw) in sources.items():
        def now_step():
            ctx.frames_upload_cameras_device(nb, None, args.height, args.width, now_first_pair=0, **fkw)
            ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
            return ctx.get_poses()

        def pairs_step():
            ctx.frames_upload_cameras_device(rb, rd, args.height, args.width, **dict(fkw, first_slot=0))
            ctx.frames_upload_cameras_device(nb, None, args.height, args.width, now_first_pair=0, **fkw)
            ctx.frames_as_ref(0, 0, B)
            ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
            return ctx.get_poses()
        timed("formats/%s/now" % name, now_step, B)
        timed("formats/%s/pairs" % name, pairs_step, B)
    pkw = dict(kw, flags=DVO_UPLOAD_ASYNC)            # pageable memory: through the engine's pinned mirror (the default upload path)

    def pageable_now():
        ctx.frames_upload_cameras(now_b, None, first_slot=B, now_first_pair=0, **pkw)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()

    def pageable_pairs():
        ctx.frames_upload_cameras(ref_b, ref_d, first_slot=0, **pkw)
        ctx.frames_upload_cameras(now_b, None, first_slot=B, now_first_pair=0, **pkw)
        ctx.frames_as_ref(0, 0, B)
        ctx.enqueue(iters, flags=DVO_FLAG_IDENTITY_START)
        return ctx.get_poses()
    if not args.pinned:
        timed("formats/pageable/now", pageable_now, B)
        timed("formats/pageable/pairs", pageable_pairs, B)
    for k in [k for k in res if k.startswith("formats/")]:
        _, src, what = k.split("/")
        formats.setdefault(src, {})[what + "_per_s"] = round(res.pop(k)["per_s"], 1)
    R, t = tracking_step()
    out = dict(config=dict(batch=B, width=args.width, height=args.height, levels=args.levels, first_shift=args.first_shift,
                           pinned=args.pinned, image_format=args.image_format, depth_format=args.depth_format,
                           host_bytes_per_ref_frame=args.width * args.height * (bpp + dpp),
                           host_bytes_per_now_frame=args.width * args.height * bpp),
               formats=formats,
               stages={k: v for k, v in res.items() if isinstance(v, dict)}, pyramid_bytes_per_frame=res.get("config_pyramid_bytes_per_frame"), mean_translation_m=float(np.linalg.norm(t, axis=1).mean()))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
