"""Multi-stream photometric engine throughput (include/dvo_amd.h, "many camera streams on the photometric engine").

K streams of 640x480 camera frames (BGR8 + depth in u16 millimetres, taken as float), the node's defaults (levels 3 then 2, 3
iterations, ref_every 10000, plus one run with ref_every 5): frames/s, ms per ordinary tick and per reference tick, kernel launches
and host synchronisations per tick, once with the frames already in HBM (DVO_UPLOAD_DEVICE) and once from pinned host memory
(DVO_UPLOAD_MAPPED).  Beside it: the single-stream baseline -- the call sequence of dvo_amd::RGBDOdometry::processFrame (upload,
photo_set_ref on a reference tick, photo_align) run stream after stream on the same device frames.

Frames: 16 synthetic scenes (frame_gen.camera_frame) x 8 camera positions; stream s plays scene s % 16 back and forth.

    python tools/bench_photo_streams.py [--ticks 30] [--ks 1,8,64,256] [--out profiles/photo_streams/bench_photo_streams.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS = 480, 640
K640 = (525.0, 525.0, 319.5, 239.5)
from rgbd_odometry_amd.frame_gen import DEPTH_FORMATS, IMAGE_FORMATS, as_format
N_SCENES, N_POS = 16, 8
IMAGE_FORMAT, DEPTH_FORMAT = "bgr8", "f32"             # --image-format / --depth-format: what the streams runs are fed


def scenes():
    from rgbd_odometry_amd.frame_gen import camera_frame
    out = []
    for sc in range(N_SCENES):
        dy, dx = (sc % 3) - 1, 1 + sc % 2
        fr = []
        for i in range(N_POS):
            bgr, depth_m = camera_frame(700 + sc, ROWS, COLS, shift=(dy * i, dx * i))
            d = np.clip(np.nan_to_num(np.round(depth_m * 1000.0), nan=0.0, posinf=65535, neginf=0), 1, 65535).astype(np.float32)
            fr.append((bgr, d))
        out.append(fr)
    return out


def frame_index(s, tick):
    p = (tick + s // N_SCENES) % (2 * N_POS - 2)
    return p if p < N_POS else 2 * N_POS - 2 - p


def run(k, frames, ticks, flags, ref_every, log, calibrations=1):
    """calibrations C > 1: C per-stream camera matrices, round robin (1: the handle's for every stream)"""
    import torch
    from rgbd_odometry_amd import DvoPhotoStreams
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE
    ps = DvoPhotoStreams(k, K640, ref_every=ref_every)
    for s in range(k if calibrations > 1 else 0):
        c = s % calibrations
        ps.set_stream_intrinsics(s, K640[0] * (1 + 0.02 * c), K640[1] * (1 + 0.015 * c), K640[2] + c, K640[3] - c)
    streams = list(range(k))
    ordinary, ref, st_o, st_r = [], [], [], []
    for tick in range(ticks + 1):
        idx = [(s % N_SCENES, frame_index(s, tick)) for s in streams]
        b = [frames[a][i][0].data_ptr() for a, i in idx]
        d = [frames[a][i][1].data_ptr() for a, i in idx]
        t0 = time.perf_counter()
        res = ps.step(streams, b, d, flags=flags, image_format=IMAGE_FORMATS.index(IMAGE_FORMAT), depth_format=DEPTH_FORMATS.index(DEPTH_FORMAT))
        dt = (time.perf_counter() - t0) * 1e3
        s = ps.stats()
        assert (res["event"] >= 0).all()
        if tick == 0:                       # first frames: warm-up (allocations of the frame store)
            continue
        (ref if s["ref_events"] else ordinary).append(dt)
        (st_r if s["ref_events"] else st_o).append(s)
    ps.close()
    torch.cuda.synchronize()
    total = sum(ordinary) + sum(ref)
    out = dict(K=k, image_format=IMAGE_FORMAT, depth_format=DEPTH_FORMAT, frames_in="HBM" if flags & DVO_UPLOAD_DEVICE else "pinned host", ref_every=ref_every, ticks=ticks, calibrations=calibrations,
               frames_per_s=round(k * ticks / total * 1e3, 1), ms_per_frame=round(total / ticks / k, 5),
               ms_ordinary_tick=round(float(np.median(ordinary)), 4) if ordinary else None,
               ms_ref_tick=round(float(np.median(ref)), 4) if ref else None, n_ref_ticks=len(ref),
               launches_ordinary=sorted({x["launches"] for x in st_o}), syncs_ordinary=sorted({x["syncs"] for x in st_o}),
               launches_ref=sorted({x["launches"] for x in st_r}), syncs_ref=sorted({x["syncs"] for x in st_r}),
               runs=sorted({x["runs"] for x in st_o + st_r}))
    log(json.dumps(out))
    return out


def single_stream(k, frames, ticks, ref_every, log):
    """RGBDOdometry::processFrame's calls, stream after stream, frames from the same device buffers (one context per stream)"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    ctxs = [DvoContext(1) for _ in range(k)]
    for c in ctxs:
        c.photo_configure(K640)
    T = [np.eye(4) for _ in range(k)]
    ms = []
    for tick in range(ticks + 1):
        t0 = time.perf_counter()
        for s, c in enumerate(ctxs):
            bgr, depth = frames[s % N_SCENES][frame_index(s, tick)]
            up = lambda slot: c.frames_upload_cameras_device([bgr.data_ptr()], [depth.data_ptr()], ROWS, COLS, n_levels=4, first_shift=0,
                                                             first_slot=slot, flags=DVO_UPLOAD_DEPTH_RAW)
            if tick % ref_every == 0:
                up(0)
                c.photo_set_ref(0)
                T[s] = np.eye(4)
            up(1)
            T[s], _, _ = c.photo_align(1, T[s], levels=(3, 2))
        if tick:
            ms.append((time.perf_counter() - t0) * 1e3)
    for c in ctxs:
        c.close()
    out = dict(single_stream_loop=True, K=k, frames_in="HBM", ref_every=ref_every, ticks=ticks,
               ms_per_frame=round(float(np.mean(ms)) / k, 5), frames_per_s=round(k * 1e3 / float(np.mean(ms)), 1))
    log(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--single-ks", default="1,8,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calibrations", type=int, default=0,
                    help="C > 1: only compare, at each K of --ks, the handle's camera matrix against C per-stream ones (round robin), frames "
                         "in HBM, reference every 5 frames; twice, interleaved")
    ap.add_argument("--image-format", choices=IMAGE_FORMATS, default="bgr8", help="format the streams' frames arrive in")
    ap.add_argument("--depth-format", choices=DEPTH_FORMATS, default="f32", help="f32: sensor units as float; u16: the sensor's 16 bits")
    a = ap.parse_args()
    global IMAGE_FORMAT, DEPTH_FORMAT
    IMAGE_FORMAT, DEPTH_FORMAT = a.image_format, a.depth_format
    import torch
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE, DVO_UPLOAD_MAPPED, MappedHostArray
    host = scenes()
    base = [[(torch.from_numpy(b).cuda(), torch.from_numpy(d).cuda()) for b, d in sc] for sc in host]         # the single-stream loop takes BGR8 + float
    fed = [[as_format(b, d, IMAGE_FORMAT, DEPTH_FORMAT, depth_unit_mm=True) for b, d in sc] for sc in host]
    dev = [[(torch.from_numpy(b).cuda(), torch.from_numpy(d).cuda()) for b, d in sc] for sc in fed]
    pinned = []
    for sc in fed:
        row = []
        for b, d in sc:
            mb, md = MappedHostArray(b.shape, np.uint8), MappedHostArray(d.shape, d.dtype)
            mb.array[...] = b
            md.array[...] = d
            row.append((mb, md))
        pinned.append(row)

    class P:                                # MappedHostArray with the data_ptr() of a tensor
        def __init__(self, m):
            self.m = m

        def data_ptr(self):
            return self.m.array.ctypes.data

    pinned_p = [[(P(b), P(d)) for b, d in sc] for sc in pinned]
    fh = open(a.out, "a") if a.out else None

    def log(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    ks = [int(x) for x in a.ks.split(",")]
    if a.calibrations > 1:
        run(min(ks), dev, 4, DVO_UPLOAD_DEVICE, 5, lambda s: None, a.calibrations)
        for rep in range(2):
            for k in ks:
                for c in (1, a.calibrations):
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, 5, log, c)
        if fh:
            fh.close()
        return
    for k in ks:
        run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, 10000, log)
    for k in ks:
        run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, 5, log)
    for k in ks:
        run(k, pinned_p, a.ticks, DVO_UPLOAD_MAPPED, 10000, log)
    for k in [int(x) for x in a.single_ks.split(",") if x]:
        single_stream(k, base, min(a.ticks, 10), 10000, log)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
