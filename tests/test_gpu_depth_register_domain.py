"""Depth registration on the device over the definition's whole domain: every case of depth_register_reference.all_cases() -- the
edges of rules 3 and 4 (a corner at 2^31, corners that are not finite, pixels that straddle the colour camera's plane, rint's ties,
q < 1), contended z-buffer words, depth images of one pixel, one row and one column, has_Dc5 = 0 over numbers left in place -- in
one context with a pair per case, so that one launch mixes depth geometries from 1 x 1 to rows x cols under a grid sized by the
largest; sub-ranges of pairs on pools that grow; colour geometries that change on a live context; colour images smaller than the
eight pixels one resolve thread stores.  Every comparison is byte equality with the host builder (dvo_depth_register_host, pinned to
the numpy restatement and to a ray-cast plane by tests/test_depth_register_cpu.py): the device compiles the same splat() with another
compiler, and its casts, rint, ceil and x - x == 0.0 are what would differ."""
import functools

import numpy as np
import pytest

import depth_register_reference as dr
from test_gpu_depth_register import c_rig, raw_image, rigs_for, to_device

pytestmark = pytest.mark.gpu


def host(g, d, rows, cols):
    from rgbd_odometry_amd import capi
    return capi.depth_register_host(c_rig(g), d, rows, cols)


@functools.lru_cache(maxsize=None)
def ordered_cases(rows, cols):
    """the cases of one colour geometry, those with a 16-bit image first (a contiguous range of pairs for the 16-bit call):
    ([(name, rig, raw image)], number of 16-bit ones)"""
    cs = sorted(dr.cases(rows, cols), key=lambda c: c[2].dtype != np.uint16)          # stable
    return cs, sum(1 for c in cs if c[2].dtype == np.uint16)


def fresh(d, k):
    """another image of the same case: rolled by k pixels along both axes (k = 0: the case's own)"""
    return np.ascontiguousarray(np.roll(d, (k, 3 * k), (0, 1)))


@functools.lru_cache(maxsize=None)
def want(rows, cols, name, k, f32):
    """the host builder's image of a case of ordered_cases(rows, cols) for fresh(image, k): computed once"""
    g, d = next((g, d) for n, g, d in ordered_cases(rows, cols)[0] if n == name)
    return host(g, dr.as_f32(fresh(d, k)) if f32 else fresh(d, k), rows, cols)


def register(ctx, images, first_pair, device):
    """one registration of host arrays, as they are or from device memory"""
    import torch
    from rgbd_odometry_amd import capi
    if not device:
        return ctx.register_depth(images, first_pair=first_pair)
    dev = [to_device(a) for a in images]
    fmt = capi.DVO_DEPTH_U16 if images[0].dtype == np.uint16 else capi.DVO_DEPTH_F32
    ptrs = ctx.register_depth([a for _, a in dev], first_pair=first_pair, flags=capi.DVO_UPLOAD_DEVICE, depth_format=fmt)
    torch.cuda.synchronize()                                   # the sources stay alive until the launches that read them are done
    return ptrs


def compare(ctx, pairs, rows, cols, tag, kind):
    """pairs: [(pair, case name, expected image)]; all differences of the call are reported, as (name, format, source, differing pixels)"""
    bad = []
    for p, name, w in pairs:
        got = ctx.get_registered_depth(p)
        assert got.shape == (rows, cols) and got.dtype == np.uint16, (name, tag, kind, got.shape)
        if not np.array_equal(got, w):
            bad.append((name, tag, kind, int((got != w).sum())))
    assert not bad, bad


def case_context(rows, cols):
    from rgbd_odometry_amd import DvoContext
    cs, n16 = ordered_cases(rows, cols)
    ctx = DvoContext(len(cs))
    for p, (name, g, d) in enumerate(cs):
        ctx.set_pair_depth_rig(p, c_rig(g), rows, cols)
    return ctx, cs, n16


def run_every_case(rows, cols):
    ctx, cs, n16 = case_context(rows, cols)
    with ctx:
        for tag, n in (("f32", len(cs)), ("u16", n16)):
            images = [dr.as_f32(d) if tag == "f32" else d for _, _, d in cs[:n]]
            for kind in ("host", "device"):
                register(ctx, images, 0, kind == "device")
                compare(ctx, [(p, cs[p][0], want(rows, cols, cs[p][0], 0, tag == "f32")) for p in range(n)], rows, cols, tag, kind)


@pytest.mark.parametrize("rows,cols", [(96, 128), (75, 101)])
def test_every_case_on_the_device(rows, cols):
    """a pair per case, one float call over all of them and one 16-bit call over those that have a 16-bit image, each from host and
    from device sources; then many_to_one, whose colour geometry is its own: four pairs, four random images, one call"""
    from rgbd_odometry_amd import DvoContext
    cs, n16 = ordered_cases(rows, cols)
    shapes = {g["depth_shape"] for _, g, _ in cs}
    assert {(1, 1), (rows, cols)} <= shapes and len(shapes) >= 7 and 4 <= n16 < len(cs)         # one launch, many depth geometries
    run_every_case(rows, cols)
    mr, mc = dr.MANY_SHAPE
    many = [dr.many_to_one(rows, cols, seed) for seed in range(4)]
    with DvoContext(4) as ctx:
        for p, (g, d) in enumerate(many):
            ctx.set_pair_depth_rig(p, c_rig(g), mr, mc)
        for tag in ("u16", "f32"):
            images = [dr.as_f32(d) if tag == "f32" else d for _, d in many]
            for kind in ("host", "device"):
                register(ctx, images, 0, kind == "device")
                compare(ctx, [(p, "many_to_one[%d]" % p, host(many[p][0], images[p], mr, mc)) for p in range(4)], mr, mc, tag, kind)
    assert len({host(g, d, mr, mc).tobytes() for g, d in many}) == 4


def test_sub_ranges_and_growth():
    """count 1, then 3 from pair 2, then 2, then every pair, then 1 again, with other images each time: the pools start at one image
    and grow twice, a z-buffer that was not re-armed would keep the minima of the call before, and only the pairs of the last call
    have an image"""
    from rgbd_odometry_amd import DvoError, capi
    rows, cols = 96, 128
    ctx, cs, n16 = case_context(rows, cols)
    assert n16 >= 5
    with ctx:
        for k, (first, count, tag) in enumerate([(0, 1, "u16"), (2, 3, "u16"), (0, 2, "f32"), (0, len(cs), "f32"), (n16 - 1, 1, "u16")]):
            f32 = tag == "f32"
            images = [dr.as_f32(fresh(cs[p][2], k + 1)) if f32 else fresh(cs[p][2], k + 1) for p in range(first, first + count)]
            register(ctx, images, first, device=bool(k % 2))
            compare(ctx, [(p, cs[p][0], want(rows, cols, cs[p][0], k + 1, f32)) for p in range(first, first + count)], rows, cols, tag,
                    "device" if k % 2 else "host")
            for p in [q for q in (0, 1, first - 1, first + count, len(cs) - 1) if 0 <= q < len(cs) and not first <= q < first + count]:
                with pytest.raises(DvoError) as ei:
                    ctx.get_registered_depth(p)
                assert ei.value.code == capi.DVO_ERR_STATE, (k, p)


def test_colour_geometry_changes_on_one_context():
    """four pairs set for 96 x 128, then 24 x 32, then 75 x 101, then 96 x 128 again, two registrations each with other images: the
    pools are reused at another stride, and the second registration of a geometry finds the z-buffer as the first left it"""
    from rgbd_odometry_amd import DvoContext
    seed = 100
    with DvoContext(4) as ctx:
        for rows, cols in ((96, 128), (24, 32), (75, 101), (96, 128)):
            rigs = rigs_for(rows, cols)
            for p, g in enumerate(rigs):
                ctx.set_pair_depth_rig(p, c_rig(g), rows, cols)
            for rep in range(2):
                images = [raw_image(g, seed + p) for p, g in enumerate(rigs)]
                if rep:
                    images = [dr.as_f32(d) for d in images]
                register(ctx, images, 0, device=bool(rep))
                compare(ctx, [(p, "rig %d at %dx%d" % (p, rows, cols), host(rigs[p], images[p], rows, cols)) for p in range(4)], rows, cols,
                        "f32" if rep else "u16", "device" if rep else "host")
                seed += 4


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 9), (3, 3), (6, 8)])
def test_tiny_colour_images(rows, cols):
    """colour images of 1, 9, 9 and 48 pixels: the first below the eight pixels one thread of the resolve launch stores, the next two
    no multiple of them.  Every case of the list can be built for them (the depth geometries that do not follow the colour image
    stay as they are); what the cases are there for mostly does not happen at these sizes, the equality with the host does"""
    cs, n16 = ordered_cases(rows, cols)
    assert sum(1 for name, _, _ in cs if want(rows, cols, name, 0, True).any()) >= len(cs) // 3
    run_every_case(rows, cols)
