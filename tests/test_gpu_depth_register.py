"""Depth registration of the frame stage on the device (include/dvo_amd.h, "depth registration": dvo_frames_set_pair_depth_rig,
dvo_frames_register_depth, dvo_frames_get_registered_depth) against the host builder (dvo_depth_register_host, itself pinned to the
numpy restatement by tests/test_depth_register_cpu.py).  One context of four pairs with four different rigs -- two with 60 x 80 depth, one
with 96 x 128, one with rotation and colour distortion on 72 x 96 -- for 96 x 128 colour images.  All comparisons are byte equality:
the z-buffer takes minima, which no schedule can reorder."""
import functools

import numpy as np
import pytest

from rgbd_odometry_amd import frame_gen
import depth_register_reference as dr

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT = 96, 128, 3, 1


def rigs_for(rows, cols):
    Kc = dr.colour_K(rows, cols)
    sk = lambda shape: dr.scaled_K(Kc, (rows, cols), shape)
    R = dr.rot("z", 0.02) @ dr.rot("y", 0.03) @ dr.rot("x", -0.01)
    return [dr.rig((60, 80), sk((60, 80)), Kc, t=[0.05, 0.0, 0.0]),
            dr.rig((60, 80), sk((60, 80)), Kc, R=dr.rot("y", -0.02), t=[-0.03, 0.01, 0.002]),
            dr.rig((96, 128), sk((96, 128)), Kc, t=[0.025, 0.0, 0.0]),
            dr.rig((72, 96), sk((72, 96)), Kc, R=R, t=[0.04, -0.01, 0.005], Dc5=[0.1, -0.05, 0.001, -0.002, 0.01])]


def raw_image(g, seed):
    """a raw depth image of rig g: a ramp with a foreground box, 5 % holes"""
    shape = g["depth_shape"]
    rng = np.random.default_rng(seed)
    d = dr.ramp(shape, 900 + 37 * (seed % 7), 3500)
    box = dr.box_scene(shape)[1]
    d[np.roll(box, (seed % 5) - 2, axis=1)] = 700 + 10 * (seed % 9)
    d[rng.random(shape) < 0.05] = 0
    return d


def c_rig(g):
    from rgbd_odometry_amd import capi
    r = capi.DvoDepthRig.make(g["depth_shape"], g["Kd4"], g["Kc4"], R=g["R"], t=g["t"], Dc5=g["Dc5"])
    r.has_Dc5 = int(g["has_Dc5"])                              # 0 with the numbers in place: the rig of the case dc5_ignored
    return r


@functools.lru_cache(maxsize=None)
def want(rows, cols, pair, seed, f32=False):
    """the host builder's image for rig `pair` of rigs_for(rows, cols) and raw_image(seed): computed once"""
    from rgbd_odometry_amd import capi
    g = rigs_for(rows, cols)[pair]
    d = raw_image(g, seed)
    return capi.depth_register_host(c_rig(g), dr.as_f32(d) if f32 else d, rows, cols)


def to_device(arr):
    """(tensor that owns the memory, device address) of a host array's bytes"""
    import torch
    t = torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint8).copy()).cuda()
    return t, t.data_ptr()


def make_context(rows=ROWS, cols=COLS, n_pairs=4, n_rigs=4):
    from rgbd_odometry_amd import DvoContext
    ctx = DvoContext(n_pairs)
    for p, g in enumerate(rigs_for(rows, cols)[:n_rigs]):
        ctx.set_pair_depth_rig(p, c_rig(g), rows, cols)
    return ctx


def check(ctx, rows, cols, first_pair, seeds, f32=False):
    for i, seed in enumerate(seeds):
        got = ctx.get_registered_depth(first_pair + i)
        w = want(rows, cols, first_pair + i, seed, f32)
        assert got.shape == (rows, cols) and np.array_equal(got, w), (first_pair + i, seed, int((got != w).sum()))


def test_host_and_device_sources_then_more_calls():
    import torch
    from rgbd_odometry_amd import DvoError, capi
    rigs = rigs_for(ROWS, COLS)
    for p in range(4):                                         # the cases mean something: holes, a shadow, several depths
        w = want(ROWS, COLS, p, 10 + p)
        assert 0.02 < (w == 0).mean() < 0.5 and len(np.unique(w)) > 50
    with make_context() as ctx:
        with pytest.raises(DvoError) as ei:                    # nothing registered yet
            ctx.get_registered_depth(0)
        assert ei.value.code == capi.DVO_ERR_STATE
        # host sources, 16-bit
        ptrs = ctx.register_depth([raw_image(rigs[p], 10 + p) for p in range(4)])
        assert len(ptrs) == 4 and all(a % 16 == 0 for a in ptrs) and len(set(ptrs)) == 4
        check(ctx, ROWS, COLS, 0, [10, 11, 12, 13])
        # device sources, 16-bit
        dev = [to_device(raw_image(rigs[p], 20 + p)) for p in range(4)]
        ptrs = ctx.register_depth([a for _, a in dev], flags=capi.DVO_UPLOAD_DEVICE, depth_format=capi.DVO_DEPTH_U16)
        assert all(a % 16 == 0 for a in ptrs)
        check(ctx, ROWS, COLS, 0, [20, 21, 22, 23])
        # count 2 with other images, on pairs 1 and 2: a z-buffer that was not re-armed would keep the minima of the calls before
        ctx.register_depth([raw_image(rigs[p], 30 + p) for p in (1, 2)], first_pair=1, flags=capi.DVO_UPLOAD_ASYNC)
        check(ctx, ROWS, COLS, 1, [31, 32])
        for p in (0, 3):                                       # ... and only the pairs of the last call have an image
            with pytest.raises(DvoError) as ei:
                ctx.get_registered_depth(p)
            assert ei.value.code == capi.DVO_ERR_STATE
        # count 4 again, float metres from the device: a stale pool would show the images of the call before
        dev32 = [to_device(dr.as_f32(raw_image(rigs[p], 40 + p))) for p in range(4)]
        ctx.register_depth([a for _, a in dev32], flags=capi.DVO_UPLOAD_DEVICE | capi.DVO_UPLOAD_ASYNC, depth_format=capi.DVO_DEPTH_F32)
        check(ctx, ROWS, COLS, 0, [40, 41, 42, 43], f32=True)
        # host float metres
        ctx.register_depth([dr.as_f32(raw_image(rigs[p], 50 + p)) for p in range(4)])
        check(ctx, ROWS, COLS, 0, [50, 51, 52, 53], f32=True)
        torch.cuda.synchronize()
        del dev, dev32


def test_odd_colour_geometry_on_a_fresh_context():
    """75 x 101 = 7575 pixels: no multiple of the eight pixels one thread of the resolve launch stores"""
    rows, cols = 75, 101
    rigs = rigs_for(rows, cols)
    with make_context(rows, cols) as ctx:
        ptrs = ctx.register_depth([raw_image(rigs[p], 60 + p) for p in range(4)])
        assert all(a % 16 == 0 for a in ptrs)
        check(ctx, rows, cols, 0, [60, 61, 62, 63])
        ctx.register_depth([raw_image(rigs[p], 70 + p) for p in range(4)])
        check(ctx, rows, cols, 0, [70, 71, 72, 73])


def test_registered_images_upload_in_place():
    """dvo_frames_upload_cameras_fmt(DVO_UPLOAD_DEVICE, DVO_DEPTH_U16) on the registered images stores the levels the host-registered
    images give through a host upload"""
    from rgbd_odometry_amd import DvoContext, capi
    rigs = rigs_for(ROWS, COLS)
    bgr = [frame_gen.camera_frame(80 + p, ROWS, COLS)[0] for p in range(4)]
    with DvoContext(4) as ref:
        ref.frames_upload_cameras(bgr, [want(ROWS, COLS, p, 80 + p) for p in range(4)], n_levels=NL, first_shift=SHIFT)
        want_levels = [[ref.frame_level(p, l) for l in range(NL)] for p in range(4)]
    with make_context() as ctx:
        dev = [to_device(b) for b in bgr]
        ptrs = ctx.register_depth([raw_image(rigs[p], 80 + p) for p in range(4)], flags=capi.DVO_UPLOAD_ASYNC)
        ctx.frames_upload_cameras_device([a for _, a in dev], ptrs, ROWS, COLS, n_levels=NL, first_shift=SHIFT,
                                         depth_format=capi.DVO_DEPTH_U16)
        for p in range(4):
            for l in range(NL):
                g, d, e, n = ctx.frame_level(p, l)
                wg, wd, we, wn = want_levels[p][l]
                assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)), (p, l)
                assert np.array_equal(g, wg) and np.array_equal(e, we) and n == wn, (p, l)
        assert (want_levels[0][0][1] == 1.0).any()             # holes are there, as the publisher's 1 mm
        del dev
        # colour images one byte off a 4-byte boundary are not read in place: the upload gathers both sources on its copy streams, and
        # that gather must come after the registration that is writing the depth images on the context stream
        import torch
        off = []
        for b in bgr:
            t = torch.zeros(b.size + 16, dtype=torch.uint8, device="cuda")
            t[1:1 + b.size] = torch.from_numpy(b.reshape(-1)).cuda()
            off.append(t)
        torch.cuda.synchronize()
        for rep in range(3):                                   # other images in between, so that a stale read would show
            ctx.register_depth([raw_image(rigs[p], 85 + rep + p) for p in range(4)], flags=capi.DVO_UPLOAD_ASYNC)
            ptrs = ctx.register_depth([raw_image(rigs[p], 80 + p) for p in range(4)], flags=capi.DVO_UPLOAD_ASYNC)
            ctx.frames_upload_cameras_device([t.data_ptr() + 1 for t in off], ptrs, ROWS, COLS, n_levels=NL, first_shift=SHIFT,
                                             depth_format=capi.DVO_DEPTH_U16)
            for p in range(4):
                for l in range(NL):
                    g, d, e, n = ctx.frame_level(p, l)
                    wg, wd, we, wn = want_levels[p][l]
                    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)) and np.array_equal(g, wg) and np.array_equal(e, we), (rep, p, l)
        del off


def test_refusals_change_nothing():
    from rgbd_odometry_amd import DvoError, capi
    rigs = rigs_for(ROWS, COLS)
    images = [raw_image(rigs[p], 90 + p) for p in range(4)]
    with make_context(n_pairs=5) as ctx:                       # pair 4 has no rig
        ctx.register_depth(images)

        def refused(code, fn):
            with pytest.raises(DvoError) as ei:
                fn()
            assert ei.value.code == code
            check(ctx, ROWS, COLS, 0, [90, 91, 92, 93])         # the previous images stay readable, as they were

        refused(capi.DVO_ERR_STATE, lambda: ctx.register_depth(images[3:] + images[:1], first_pair=3))
        refused(capi.DVO_ERR_INVALID, lambda: ctx.register_depth(images, flags=capi.DVO_UPLOAD_MAPPED))
        refused(capi.DVO_ERR_INVALID, lambda: ctx.register_depth(images, flags=capi.DVO_UPLOAD_DIRECT))
        refused(capi.DVO_ERR_INVALID, lambda: ctx.register_depth(images, flags=capi.DVO_UPLOAD_DEPTH_RAW))
        refused(capi.DVO_ERR_INVALID, lambda: ctx.register_depth([images[2], images[3]] * 2, first_pair=2))     # beyond the context's pairs
        refused(capi.DVO_ERR_INVALID, lambda: ctx.register_depth([1, 2, 3, 4], flags=capi.DVO_UPLOAD_DEVICE, depth_format=7))
        refused(capi.DVO_ERR_INVALID, lambda: ctx.set_pair_depth_rig(5, c_rig(rigs[0]), ROWS, COLS))
        bad = c_rig(rigs[0])
        bad.Kc4[1] = 0.0
        refused(capi.DVO_ERR_INVALID, lambda: ctx.set_pair_depth_rig(0, bad, ROWS, COLS))
        refused(capi.DVO_ERR_INVALID, lambda: ctx.set_pair_depth_rig(0, c_rig(rigs[0]), 0, COLS))
        # mixed colour geometries among the listed pairs
        ctx.set_pair_depth_rig(2, c_rig(rigs[2]), 75, 101)
        refused(capi.DVO_ERR_INVALID, lambda: ctx.register_depth(images))
        ctx.set_pair_depth_rig(2, c_rig(rigs[2]), ROWS, COLS)
        # a removed rig is gone
        ctx.set_pair_depth_rig(1, None)
        refused(capi.DVO_ERR_STATE, lambda: ctx.register_depth(images))
        ctx.set_pair_depth_rig(1, c_rig(rigs[1]), ROWS, COLS)
        ctx.register_depth([raw_image(rigs[p], 95 + p) for p in range(4)])
        check(ctx, ROWS, COLS, 0, [95, 96, 97, 98])
