"""Multi-stream tracker throughput (include/dvo_amd.h, "many camera streams").

K streams of 640x480 camera frames (BGR8 + depth in metres), 4 levels, 10 iterations per level, key frame every 5 frames (plus one run
with the adaptive exits): frames/s, ms per ordinary tick and per key-frame tick, kernel launches and host synchronisations per tick,
once with the frames already in HBM (DVO_UPLOAD_DEVICE) and once from pinned host memory (DVO_UPLOAD_MAPPED).  Two pyramids, labelled
in every line: level 0 = the full 640x480 frame (first_shift 0, the pyramid of bench.py's frames-in line: 1.35 ms / 190 k frames/s
per 256 frames) and level 0 = 320x240 (first_shift 1, what the reference's publisher sends).  Beside it: the single-stream path
(the engine calls of dvo_amd::SolveDVO::processFrame for one camera, frames read from the same device buffers) and the CPU oracle's
alignment of one frame pair.

Frames: 32 synthetic scenes (frame_gen.camera_frame, distinct seeds) x 8 camera positions each; stream s plays scene s % 32 back and
forth from its own starting position and direction, so that streams differ and every stream keeps moving.

    python tools/bench_streams.py [--ticks 50] [--ks 1,8,64,256] [--out profiles/streams/bench_streams.jsonl]
    python tools/bench_streams.py --archive --ks 256 --out profiles/tracker_archive/bench_streams_archive.jsonl
    python tools/bench_streams.py --places --ks 256 --out profiles/tracker_places/bench_streams_places.jsonl
    python tools/bench_streams.py --masks both --ks 256 --out profiles/frame_masks/bench_streams_masks.jsonl
    python tools/bench_streams.py --raw-depth --depth-format u16 --ks 256 --ticks 40 --out profiles/depth_register/this_1.jsonl
    python tools/bench_streams.py --ks 1,256 --ticks 50 --out profiles/tracker_plan/plain_change_1.jsonl         (K = 1: host time of a step)
    python tools/bench_streams.py --archive --places --ks 256 --out profiles/tracker_plan/places_change_1.jsonl  (--places decides the form)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rgbd_odometry_amd.frame_gen import DEPTH_FORMATS, IMAGE_FORMATS, as_format

ROWS, COLS, NL, IT = 480, 640, 4, 10
FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5
N_SCENES, N_POS = 32, 8
IMAGE_FORMAT, DEPTH_FORMAT = "bgr8", "f32"             # --image-format / --depth-format: what the tracker runs are fed


def scenes():
    from rgbd_odometry_amd.frame_gen import camera_frame
    out = []
    for sc in range(N_SCENES):
        dy, dx = (sc % 3) - 1, 1 + sc % 2
        out.append([camera_frame(500 + sc, ROWS, COLS, shift=(dy * i, dx * i)) for i in range(N_POS)])
    return out


def frame_index(s, tick):
    """ping-pong over the scene's positions, per-stream phase"""
    p = (tick + s // N_SCENES) % (2 * N_POS - 2)
    return p if p < N_POS else 2 * N_POS - 2 - p


def level0(shift):
    return "%dx%d" % (COLS >> shift, ROWS >> shift)


def calibration(c):
    """calibration c of a rig (--calibrations): intrinsics and a distortion that differ per c"""
    return (FX * (1 + 0.02 * c), FY * (1 + 0.015 * c), CX + c, CY - c), (-0.05 - 0.01 * c, 0.01, 0.0005 * c, -0.0003, 0.0)


ARCHIVE_NS = (1, 32, 256)                              # candidates per dvo_tracker_score / dvo_tracker_match call of an --archive run


def stream_mask(s):
    """the ignore mask of stream s (--masks): the lowest fifth of the image (a bonnet) and a disc whose place depends on the stream"""
    i, j = np.mgrid[0:ROWS, 0:COLS]
    cy, cx = 100 + 37 * (s % 5), 120 + 53 * (s % 8)
    return ((i >= ROWS - ROWS // 5) | ((i - cy) ** 2 + (j - cx) ** 2 <= 40 * 40)).astype(np.uint8)


def stream_rig(s):
    """the depth rig of stream s (--raw-depth): a 640x480 depth camera with the colour camera's intrinsics, 50 mm to its side, turned
    by a small angle that depends on the stream"""
    from rgbd_odometry_amd.capi import DvoDepthRig
    a = 0.004 + 0.001 * (s % 5)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return DvoDepthRig.make((ROWS, COLS), (FX, FY, CX, CY), (FX, FY, CX, CY), R=R, t=(0.05, 0.0, 0.0))


def run(k, frames, ticks, flags, adaptive, log, shift, calibrations=0, information=False, views=False, archive=None, masks=None,
        raw_depth=None):
    """raw_depth (None: not a --raw-depth comparison, the line says nothing of it; False / True: its two sides): every stream gets a
    depth rig (stream_rig) and the depth frames are taken as UNREGISTERED: DvoTracker.step_raw_depth registers them on the device
    (two more launches per upload run) before the frame stage reads them.
    masks (None: not a --masks comparison, the line says nothing of it; False / True: its two sides): every stream gets an ignore
    mask of its own (DvoTracker.set_stream_mask, margin 2: K sets of keep planes, one more launch per upload run).
    archive (None: not an --archive comparison, the line says nothing of it; False / True: its two sides): the key-frame archive
    (DvoTracker.set_archive: 2 K slots) during the run, then score() and match() of n = 1, 32, 256 candidates -- stream i % K against
    the current key frame of stream (i + 1) % K -- timed after the last tick; candidates whose key frame is not in the archive
    (refused or evicted: id -1) are left out and counted in the line.
    calibrations 0: no undistortion; 1: one handle-wide calibration with distortion; C > 1: C per-stream calibrations round robin;
    information: the 6x6 pose information with every pose (DvoTracker.set_information); views: the debug views of every stream
    (DvoTracker.set_views; the images stay in HBM, as in a rig that looks at them on request)"""
    import torch
    from rgbd_odometry_amd import DvoTracker, capi
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE
    tr = DvoTracker(k, iters=[IT] * NL, rows=ROWS, cols=COLS, n_levels=NL, first_shift=shift, adaptive=adaptive,
                    points_capacity=[90000, 30000, 9000, 3000] if shift == 0 else [40000, 12000, 4000, 1200])
    tr.set_intrinsics(FX, FY, CX, CY)
    if calibrations == 1:
        K4, D5 = (np.array(x, np.float64) for x in calibration(0))
        assert capi.load_library().dvo_frames_set_undistort(tr.context_handle(), ROWS, COLS, capi._ptr(K4), capi._ptr(D5)) == 0
    for s in range(k if calibrations > 1 else 0):
        K4, D5 = calibration(s % calibrations)
        tr.set_stream_intrinsics(s, *K4)
        tr.set_stream_undistort(s, K4, D5)
    if information:
        tr.set_information(True)
    if views:
        tr.set_views(True)
    if archive:
        tr.set_archive(2 * k, max(ARCHIVE_NS))
    for s in range(k if masks else 0):
        tr.set_stream_mask(s, stream_mask(s), 2)
    for s in range(k if raw_depth else 0):
        tr.set_stream_depth_rig(s, stream_rig(s))
    step = tr.step_raw_depth if raw_depth else tr.step
    streams = list(range(k))
    ordinary, key, st = [], [], []
    for tick in range(ticks + 1):
        idx = [(s % N_SCENES, frame_index(s, tick)) for s in streams]
        b = [frames[a][i][0].data_ptr() for a, i in idx]
        d = [frames[a][i][1].data_ptr() for a, i in idx]
        t0 = time.perf_counter()
        step(streams, b, d, flags=flags, image_format=IMAGE_FORMATS.index(IMAGE_FORMAT), depth_format=DEPTH_FORMATS.index(DEPTH_FORMAT))
        dt = (time.perf_counter() - t0) * 1e3
        s = tr.stats()
        if tick == 0:                       # first frames: references only
            continue
        (key if s["key_frames"] else ordinary).append(dt)
        st.append(s)
    loop = {}
    for n in ARCHIVE_NS if archive else ():
        cand = [(i % k, tr.key_frame_id((i + 1) % k)) for i in range(n)]
        cs, ck = [c for c, kid in cand if kid >= 0], [kid for c, kid in cand if kid >= 0]
        loop["candidates_n%d" % n] = len(cs)
        if not cs:
            continue
        R, t = np.tile(np.eye(3), (len(cs), 1, 1)), np.zeros((len(cs), 3))
        for name, call in (("score", lambda: tr.score(cs, ck, 0, R, t)), ("match", lambda: tr.match(cs, ck, R, t))):
            ms = []
            for rep in range(6):
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            loop["ms_%s_n%d" % (name, n)] = round(float(np.median(ms[1:])), 4)      # the first call allocates
    if archive:
        loop["archive_stats"] = tr.archive_stats()
    tr.close()
    torch.cuda.synchronize()
    total = sum(ordinary) + sum(key)
    res = dict(K=k, **({} if archive is None else dict(archive=bool(archive))), **({} if masks is None else dict(masks=bool(masks))), **({} if raw_depth is None else dict(raw_depth=bool(raw_depth))), **loop, level0=level0(shift), calibrations=calibrations, information=bool(information), views=bool(views), image_format=IMAGE_FORMAT, depth_format=DEPTH_FORMAT, frames_in="HBM" if flags & DVO_UPLOAD_DEVICE else "pinned host", adaptive=bool(adaptive), ticks=ticks,
               frames_per_s=round(k * ticks / total * 1e3, 1), ms_per_tick=round(total / ticks, 4),
               ms_ordinary_tick=round(float(np.median(ordinary)), 4) if ordinary else None,
               ms_key_tick=round(float(np.median(key)), 4) if key else None, n_key_ticks=len(key),
               launches_ordinary=sorted({x["launches"] for x in st if not x["key_frames"]}),
               launches_key=sorted({x["launches"] for x in st if x["key_frames"]}),
               syncs_ordinary=sorted({x["syncs"] for x in st if not x["key_frames"]}),
               syncs_key=sorted({x["syncs"] for x in st if x["key_frames"]}),
               runs=sorted({x["runs"] for x in st}), slab_growths=sum(x["slab_growths"] for x in st))
    log(json.dumps(res))
    return res


PLACES_K, PLACES_MATCHES = 8, 32                       # nearest key frames per stream; candidates of the reference dvo_tracker_match


def run_places(k, frames, capacity, places, log, query=True):
    """--places: an archive of `capacity` slots filled by a tracker that makes a key frame nearly every tick (key_frame_every = 2),
    with (places = True) or without place descriptors at the coarsest level; ms per key-frame tick of both sides.  With places: one
    dvo_tracker_query_places for all K streams, timed by HIP events on the context's stream around the call (upload of the query list,
    two launches, copy of the result) and by the host clock (the same plus the call's one synchronisation), beside a dvo_tracker_match
    of PLACES_MATCHES candidates taken from the query's own result"""
    import torch
    from rgbd_odometry_amd import DvoTracker, capi
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE
    caps = [90000, 30000, 9000, 3000]                      # these scenes have more edge pixels than the archive's default slot (1/8 of a level) holds
    tr = DvoTracker(k, iters=[IT] * NL, rows=ROWS, cols=COLS, n_levels=NL, first_shift=0, key_frame_every=2, points_capacity=caps)
    tr.set_intrinsics(FX, FY, CX, CY)
    stream = torch.cuda.Stream()
    assert capi.load_library().dvo_set_stream(tr.context_handle(), stream.cuda_stream) == 0
    tr.set_archive(capacity, PLACES_MATCHES, caps)
    if places:
        tr.set_places()
    streams = list(range(k))
    ticks, key_ms, st = 0, [], []
    while tr.archive_stats()["archived"] < capacity + k:   # until the ring is full and has wrapped
        idx = [(s % N_SCENES, frame_index(s, ticks)) for s in streams]
        b = [frames[a][i][0].data_ptr() for a, i in idx]
        d = [frames[a][i][1].data_ptr() for a, i in idx]
        t0 = time.perf_counter()
        tr.step(streams, b, d, flags=DVO_UPLOAD_DEVICE, image_format=IMAGE_FORMATS.index(IMAGE_FORMAT), depth_format=DEPTH_FORMATS.index(DEPTH_FORMAT))
        dt = (time.perf_counter() - t0) * 1e3
        x = tr.stats()
        if ticks > 0 and x["key_frames"] == k:
            key_ms.append(dt)
            st.append(x)
        ticks += 1
    res = dict(K=k, capacity=capacity, places=bool(places), ticks=ticks, level0=level0(0), ms_key_tick=round(float(np.median(key_ms)), 4),
               ms_key_tick_min=round(float(np.min(key_ms)), 4), n_key_ticks=len(key_ms), launches_key=sorted({x["launches"] for x in st}),
               syncs_key=sorted({x["syncs"] for x in st}), archive_stats=tr.archive_stats())
    if places and query:
        ev_ms, wall_ms, rows = [], [], None
        with torch.cuda.stream(stream):
            for rep in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                rows = tr.places_raw(streams, PLACES_K)
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                e1.record(stream)
                e1.synchronize()
                ev_ms.append(e0.elapsed_time(e1))
        q = tr.archive_stats()
        cs = [s for s in streams if rows[1][s] > 0][:PLACES_MATCHES]
        ck = [int(rows[0][s, 0]["key_id"]) for s in cs]
        m_ms = []
        for rep in range(6):
            t0 = time.perf_counter()
            tr.match(cs, ck)
            m_ms.append((time.perf_counter() - t0) * 1e3)
        res.update(query_k=PLACES_K, descriptor_bytes=len(tr.archive_descriptor(ck[0])), query_ms_events=round(float(np.median(ev_ms[2:])), 4),
                   query_ms_events_min=round(float(np.min(ev_ms[2:])), 4), query_ms_wall=round(float(np.median(wall_ms[2:])), 4),
                   query_launches=q["last_launches"], query_syncs=q["last_syncs"], found_min=int(rows[1].min()),
                   match_n=len(cs), match_ms_wall=round(float(np.median(m_ms[1:])), 4))
    tr.close()
    torch.cuda.synchronize()
    log(json.dumps(res))
    return res


def single_stream_ms(dev_frames, ticks, log, shift):
    """the engine calls of dvo_amd::SolveDVO::processFrame for one camera (upload, now frame, alignment, key frame every 5), the frames
    read from the same device buffers as the tracker's (DVO_UPLOAD_DEVICE)"""
    from rgbd_odometry_amd import DvoContext
    with DvoContext(1) as ctx:
        ctx.set_intrinsics(FX, FY, CX, CY)
        ctx.frames_reserve(2)
        cR, cT, last_ref, ms = np.eye(3), np.zeros(3), 0, []
        for n in range(ticks + 1):
            bgr, depth = dev_frames[frame_index(0, n)]
            slot = n % 2
            t0 = time.perf_counter()
            ctx.frames_upload_cameras_device([bgr.data_ptr()], [depth.data_ptr()], ROWS, COLS, n_levels=NL, first_shift=shift, first_slot=slot)
            if n == 0:
                ctx.frames_as_ref(slot, 0, 1)
                continue
            ctx.frames_as_now(slot, 0, 1)
            R, t = ctx.align_batch([IT] * NL, cR[None], cT[None])
            cR, cT = R[0], t[0]
            if n - last_ref == 5 and last_ref != n - 1:
                last_ref = n - 1
                ctx.frames_as_ref(1 - slot, 0, 1)
                R, t = ctx.align_batch([IT] * NL, np.eye(3)[None], np.zeros((1, 3)))
                cR, cT = R[0], t[0]
            ms.append((time.perf_counter() - t0) * 1e3)
    res = dict(single_stream_path_ms_per_frame=round(float(np.mean(ms)), 4), frames_per_s=round(1e3 / float(np.mean(ms)), 1),
               level0=level0(shift), frames_in="HBM", ticks=ticks)
    log(json.dumps(res))
    return res


def oracle_ms(host_frames, log, shift):
    try:
        import oracle_lib
        o = oracle_lib.load()
    except Exception as e:                   # the oracle is built by build(); report, do not fail the measurement
        log(json.dumps(dict(cpu_oracle="unavailable: %s" % e)))
        return
    K = tuple(np.float32(k) for k in (FX, FY, CX, CY))
    pyr = [o.build_pyramid(b, d, NL, shift) for b, d in host_frames[:2]]
    ref = [o.ref_level_from_grey(l, g, d, K) for l, (g, d) in enumerate(pyr[0])]
    now = [o.now_level_from_grey(g) for g, _ in pyr[1]]
    lv = [dict(xyz=r[0], uv=r[1], dt=m[0], gx=m[1], gy=m[2], rows=g.shape[0], cols=g.shape[1]) for r, m, (g, _) in zip(ref, now, pyr[1])]
    t0 = time.perf_counter()
    o.align_pyramid([IT] * NL, lv, K, np.eye(3), np.zeros(3))
    ms = (time.perf_counter() - t0) * 1e3
    log(json.dumps(dict(cpu_oracle_alignment_ms_per_frame=round(ms, 3), frames_per_s=round(1e3 / ms, 1), level0=level0(shift),
                        note="alignment only, one CPU thread, frame preprocessing not included")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calibrations", type=int, default=0,
                    help="C > 1: only compare, at each K of --ks, one handle-wide calibration against C per-stream ones (round robin), "
                         "distortion on in both, frames in HBM; twice, interleaved")
    ap.add_argument("--information", action="store_true",
                    help="only compare, at each K of --ks, the tracker without and with the pose information (one more launch per step), "
                         "level 0 = 640x480, frames in HBM; three times, interleaved")
    ap.add_argument("--views", action="store_true",
                    help="only compare, at each K of --ks, the tracker without and with its debug views (two more launches per rendering), "
                         "level 0 = 640x480, frames in HBM; three times, interleaved")
    ap.add_argument("--archive", action="store_true",
                    help="only compare, at each K of --ks, the tracker without and with the key-frame archive (one more launch per batch of "
                         "new key frames), level 0 = 640x480, frames in HBM; three times, interleaved; the runs with the archive also time "
                         "score() and match() of 1, 32 and 256 candidates")
    ap.add_argument("--places", action="store_true",
                    help="only the place descriptors: at each K of --ks fill an archive of --capacity slots (key frame nearly every tick) "
                         "without and with descriptors of the coarsest level, three times, interleaved: ms per key-frame tick of both "
                         "sides, and one query of all K streams (HIP events, launches, synchronisations) beside a match of 32 candidates")
    ap.add_argument("--masks", choices=("both", "off"), default=None,
                    help="only compare, at each K of --ks, the tracker without and with a per-stream ignore mask on every stream (one more "
                         "launch per upload run), level 0 = 320x240, frames in HBM; three times, interleaved.  off: the lines without "
                         "masks alone (a library that lacks the feature can run them)")
    ap.add_argument("--raw-depth", action="store_true",
                    help="only compare, at each K of --ks, the tracker fed registered depth (step) with the tracker fed the same frames as "
                         "UNREGISTERED depth under a per-stream rig (step_raw_depth: 640x480 depth, 50 mm baseline, small rotation; two more "
                         "launches per upload run), level 0 = 320x240, frames in HBM; three times, interleaved")
    ap.add_argument("--capacity", type=int, default=4096, help="--places: slots of the archive")
    ap.add_argument("--image-format", choices=IMAGE_FORMATS, default="bgr8", help="format the tracker's frames arrive in")
    ap.add_argument("--depth-format", choices=DEPTH_FORMATS, default="f32", help="f32: metres; u16: 16-bit millimetres")
    a = ap.parse_args()
    global IMAGE_FORMAT, DEPTH_FORMAT
    IMAGE_FORMAT, DEPTH_FORMAT = a.image_format, a.depth_format
    import torch
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE, DVO_UPLOAD_MAPPED
    torch.cuda.set_device(0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    host = scenes()
    base = [[(torch.from_numpy(b).cuda(), torch.from_numpy(d).cuda()) for b, d in sc] for sc in host[:1]]     # the baselines take BGR8 + metres
    fed = [[as_format(b, d, IMAGE_FORMAT, DEPTH_FORMAT) for b, d in sc] for sc in host]
    dev = [[(torch.from_numpy(b).cuda(), torch.from_numpy(d).cuda()) for b, d in sc] for sc in fed]
    if a.calibrations > 1:
        ks = [int(x) for x in a.ks.split(",")]
        run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, 1, a.calibrations)
        for rep in range(2):
            for k in ks:
                for c in (1, a.calibrations):
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, 1, c)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.information:
        ks = [int(x) for x in a.ks.split(",")]
        for on in (False, True):
            run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, 0, information=on)      # warm-up: code objects, buffers
        for rep in range(3):
            for k in ks:
                for on in (False, True):
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, 0, information=on)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.views:
        ks = [int(x) for x in a.ks.split(",")]
        for on in (False, True):
            run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, 0, views=on)            # warm-up: code objects, buffers
        for rep in range(3):
            for k in ks:
                for on in (False, True):
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, 0, views=on)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.masks:
        ks = [int(x) for x in a.ks.split(",")]
        sides = (False, True) if a.masks == "both" else (False,)
        for on in sides:
            run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, 1, masks=on)            # warm-up: code objects, buffers
        for rep in range(3):
            for k in ks:
                for on in sides:
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, 1, masks=on)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.raw_depth:
        ks = [int(x) for x in a.ks.split(",")]
        for on in (False, True):
            run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, 1, raw_depth=on)        # warm-up: code objects, buffers
        for rep in range(3):
            for k in ks:
                for on in (False, True):
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, 1, raw_depth=on)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.places:
        ks = [int(x) for x in (a.ks if a.ks != "1,8,64,256" else "256").split(",")]
        for on in (False, True):
            run_places(min(ks), dev, 4 * min(ks), on, lambda s: None)      # warm-up: code objects, buffers
        for rep in range(3):
            for k in ks:
                for on in (False, True):
                    run_places(k, dev, a.capacity, on, log)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.archive:
        ks = [int(x) for x in a.ks.split(",")]
        for on in (False, True):
            run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, 0, archive=on)          # warm-up: code objects, buffers
        for rep in range(3):
            for k in ks:
                for on in (False, True):
                    run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, 0, archive=on)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    pinned = [[(torch.from_numpy(b).pin_memory(), torch.from_numpy(d).pin_memory()) for b, d in sc] for sc in fed]
    ks = [int(x) for x in a.ks.split(",")]
    for shift in (0, 1):
        run(min(ks), dev, 6, DVO_UPLOAD_DEVICE, False, lambda s: None, shift)    # warm-up: code objects, lazily allocated buffers
        for k in ks:
            run(k, dev, a.ticks, DVO_UPLOAD_DEVICE, False, log, shift)
        for k in ks:
            run(k, pinned, a.ticks, DVO_UPLOAD_MAPPED, False, log, shift)
        run(max(ks) if max(ks) <= 64 else 64, dev, a.ticks, DVO_UPLOAD_DEVICE, True, log, shift)
        single_stream_ms(base[0], a.ticks, log, shift)
        oracle_ms(host[0], log, shift)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
