"""Depth registration on the CPU (include/dvo_amd.h, "depth registration"): dvo_depth_register_host against the numpy restatement of
the definition (tests/depth_register_reference.py) on every case, for 16-bit and float input, the properties the definition promises,
every refusal, and the builder's own code (rgbd_odometry_amd/csrc/dvo_depth_register.h) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/host/depth_register_main.cpp).  No GPU: the builder needs neither a device nor a context.
All comparisons are byte equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_register_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(96, 128), (75, 101), (60, 80)]          # 75 x 101: an odd pixel count


def c_rig(g):
    from rgbd_odometry_amd import capi
    r = capi.DvoDepthRig.make(g["depth_shape"], g["Kd4"], g["Kc4"], R=g["R"], t=g["t"], Dc5=g["Dc5"])
    r.has_Dc5 = int(g["has_Dc5"])                              # 0 with the numbers in place: the rig of the case dc5_ignored
    return r


def formats_of(depth):
    """the inputs one case stands for: (tag, image)"""
    return [("f32", depth)] if depth.dtype == np.float32 else [("u16", depth), ("f32", dr.as_f32(depth))]


@pytest.mark.parametrize("rows,cols", SIZES)
def test_host_builder_equals_the_restatement(rows, cols):
    from rgbd_odometry_amd import capi
    for name, g, depth, (cr, cc) in dr.all_cases(rows, cols):
        for tag, d in formats_of(depth):
            got = capi.depth_register_host(c_rig(g), d, cr, cc)
            want = dr.register(g, d, cr, cc)
            assert got.shape == (cr, cc) and got.dtype == np.uint16
            assert np.array_equal(got, want), (name, tag, int((got != want).sum()))


@pytest.mark.parametrize("rows,cols", SIZES)
def test_cases_mean_something(rows, cols):
    """Each case of the definition's edges reaches the rule it is there for.  Every condition is computed from the restatement's own
    intermediate results (depth_register_reference.steps / writers), nothing from the library.

    The z-buffer's contention, three cases.  pile_up: every written colour pixel has at least 100 writers (a whole depth row each).
    contended: over a quarter of the written pixels have two to six writers at unrelated depths.  many_to_one: a depth image far
    finer than the colour image, where a depth pixel, a sixteenth of a colour pixel wide, writes only across a colour pixel's
    corner -- about one writer per colour pixel, so this recipe brings no contention.  The writers of one word lie along an epipolar
    line, where depth is monotonic: the minimum is the first or the last of them in raster order, never one between.  Both
    contended cases make it the first, and assert that it is not the last, which a plain store would most likely leave"""
    by = {name: (g, d, shape) for name, g, d, shape in dr.all_cases(rows, cols)}
    inside = lambda c, n: (c >= 0) & (c < n)
    with np.errstate(all="ignore"):
        g, d, _ = by["limit_corner_inside"]
        s = dr.steps(g, d)
        far_a, far_b = np.abs(s["ua"]) >= 2.0 ** 30, np.abs(s["ub"]) >= 2.0 ** 30
        one_in_one_far = (inside(s["ua"], cols) & far_b) | (inside(s["ub"], cols) & far_a)
        assert int(one_in_one_far.sum()) >= rows
        assert int((inside(s["ua"], cols) & (s["ub"] >= 2.0 ** 31)).sum()) >= rows    # ... and beyond the range of int on the b side
        assert np.all(s["front"] & s["front_a"] & s["front_b"]) and not s["ok"].any()
        assert not dr.register(g, d, rows, cols).any()

        g, d, _ = by["not_finite"]
        s = dr.steps(g, d)
        not_finite = ~(np.isfinite(s["ua"]) & np.isfinite(s["va"]) & np.isfinite(s["ub"]) & np.isfinite(s["vb"]))
        print("not_finite %dx%d: %d of %d pixels with a corner that is not finite" % (rows, cols, not_finite.sum(), d.size))
        assert int(not_finite.sum()) >= 1000 and np.all(s["front"] & s["front_a"] & s["front_b"])
        assert not dr.register(g, d, rows, cols).any()

        g, d, _ = by["straddle"]
        s = dr.steps(g, d)
        straddlers = s["front"] & ~(s["front_a"] & s["front_b"])
        written = int((dr.register(g, d, rows, cols) != 0).sum())
        print("straddle %dx%d: %d straddlers, %d with the centre behind, %d pixels written" % (rows, cols, straddlers.sum(), (~s["front"]).sum(), written))
        assert int(straddlers.sum()) >= 20 and written >= 1000 and int((~s["front"]).sum()) >= 1000
        # one of them would be seen if it were kept: its corners' coordinates, the one behind the camera included, span a footprint
        # inside the image, and its q is in range (the others project far outside)
        x0, y0 = np.ceil(np.minimum(s["ua"], s["ub"])), np.ceil(np.minimum(s["va"], s["vb"]))
        x1, y1 = np.minimum(np.ceil(np.maximum(s["ua"], s["ub"])), x0 + dr.SPLAT_MAX), np.minimum(np.ceil(np.maximum(s["va"], s["vb"])), y0 + dr.SPLAT_MAX)
        area = np.clip(np.minimum(x1, cols) - np.maximum(x0, 0), 0, None) * np.clip(np.minimum(y1, rows) - np.maximum(y0, 0), 0, None)
        assert int((straddlers & (area >= 32) & (s["q"] >= 1) & (s["q"] <= 65535)).sum()) >= 1

    g, d, _ = by["ties"]
    x = d.astype(np.float64) * 1000.0
    assert d.dtype == np.float32 and np.all(x - np.floor(x) == 0.5)             # every value a tie, exactly
    g, d, _ = by["tiny"]
    assert d.dtype == np.float32 and set(np.unique(dr.register(g, d, rows, cols))) == {0, 1}
    for value in dr.TINY:
        assert (d == np.float32(value)).mean() >= 0.05, value
    assert 0 < float(np.float32(1e-40)) < float(np.finfo(np.float32).tiny)      # a subnormal

    g, d, shape = by["many_to_one"]
    assert shape == dr.MANY_SHAPE != (rows, cols) and g["depth_shape"] == (rows, cols)
    w = dr.writers(g, d, *shape)
    n_writing = sum(len(v) for v in w.values())
    print("many_to_one %dx%d: %d colour pixels written by %d footprint pixels, at most %d writers" % (rows, cols, len(w), n_writing, max(map(len, w.values()))))
    # 48 colour pixels' worth of surface: 48 footprint pixels expected, and a depth pixel writes with probability 48 / (rows * cols)
    assert 30 <= len(w) <= 48 and 24 <= n_writing <= 96 and n_writing <= 0.02 * d.size

    g, d, _ = by["contended"]
    w = dr.writers(g, d, rows, cols)
    multi = [v for v in w.values() if len(v) > 1]
    print("contended %dx%d: %d pixels written, %d by more than one depth pixel, at most %d" % (rows, cols, len(w), len(multi), max(map(len, w.values()))))
    assert len(multi) >= 1000 and len(multi) >= 0.25 * len(w) and max(map(len, w.values())) >= 4
    assert all(v[-1] != min(v) for v in multi)                                  # the last writer in raster order never holds the minimum
    assert sum(1 for v in multi if len(set(v)) == len(v)) >= 0.9 * len(multi)   # and the values differ

    g, d, _ = by["pile_up"]
    for tag, image in formats_of(d):
        w = dr.writers(g, image, rows, cols)
        print("pile_up %dx%d %s: %d pixels written, %d to %d writers each" % (rows, cols, tag, len(w), min(map(len, w.values())), max(map(len, w.values()))))
        assert len(w) == rows and len({y for y, x in w}) == rows                # one word per colour row
        assert all(len(v) >= 100 for v in w.values())                           # more than a wave of 64 on each
        assert all(v[0] == min(v) and v[-1] > 10 * min(v) and len(set(v)) >= 100 for v in w.values())

    for shape in dr.SHAPES:
        g, d, _ = by["shape_%dx%d" % shape]
        assert g["depth_shape"] == shape and dr.register(g, d, rows, cols).any()
    assert {(1, 1), (1, 300), (17, 15), (257, 1)} == set(dr.SHAPES)

    g, d, _ = by["dc5_ignored"]
    g0, d0, _ = by["rot_dist_ramp"]
    assert g["Dc5"] == g0["Dc5"] and g["Dc5"] is not None and not g["has_Dc5"] and g0["has_Dc5"] and d is d0
    plain = dr.register(dr.rig(g0["depth_shape"], g0["Kd4"], g0["Kc4"], R=g0["R"], t=g0["t"]), d, rows, cols)
    assert np.array_equal(dr.register(g, d, rows, cols), plain)
    assert int((plain != dr.register(g0, d0, rows, cols)).sum()) >= 1000


@pytest.mark.parametrize("rows,cols", SIZES)
def test_properties(rows, cols):
    """what the definition promises, on the host builder's output"""
    from rgbd_odometry_amd import capi
    by_name = {name: (g, d) for name, g, d in dr.cases(rows, cols)}

    def run(name, depth=None):
        g, d = by_name[name]
        return capi.depth_register_host(c_rig(g), d if depth is None else depth, rows, cols)

    g, d = by_name["identity"]
    assert np.array_equal(run("identity"), d)                                   # byte for byte, holes included
    assert np.array_equal(run("identity", dr.as_f32(d)), d)                     # millimetre-valued metres come back as they were
    assert 0.05 < (d == 0).mean() < 0.15
    for name in ("plane_60x80", "plane_96x128"):                                # up- and down-scaled: no hole
        out = run(name)
        assert np.all(out == 1500), (name, int((out == 0).sum()))
    # a 50 mm baseline: the box wins where both land, and leaves an occlusion shadow
    g, d = by_name["baseline_box"]
    _, box = dr.box_scene((rows, cols))
    only_box, only_back = np.where(box, d, 0).astype(np.uint16), np.where(box, 0, d).astype(np.uint16)
    out, ob, ok = run("baseline_box"), run("baseline_box", only_box), run("baseline_box", only_back)
    both = (ob != 0) & (ok != 0)
    assert both.any() and np.array_equal(out[both], ob[both]) and np.all(ob[both] < ok[both])
    assert np.array_equal(out, np.where(ob != 0, ob, ok))
    share = (out == 0).mean()
    print("baseline_box %dx%d: hole share %.4f" % (rows, cols, share))
    assert 0 < share < 0.05
    # the clamp: four pixels, 12 colour pixels wide each, write 8 x 8 each
    out = run("clamp_12x")
    assert int((out != 0).sum()) == 4 * dr.SPLAT_MAX * dr.SPLAT_MAX and np.all(out[out != 0] == 2000)
    for name in ("behind", "f32_far", "outside", "all_zero"):
        assert not run(name).any(), name
    # NaN, +-inf, 0 and negative values are no measurements: the same image with zeros in their place registers alike
    g, d = by_name["f32_specials"]
    bad = ~(np.isfinite(d) & (d > 0))
    assert np.isnan(d).any() and np.isposinf(d).any() and (d == 0).any() and (d < 0).any() and bad.mean() > 0.2
    assert np.array_equal(run("f32_specials"), run("f32_specials", np.where(bad, np.float32(0), d)))
    assert run("f32_specials").any()
    # 65.535 m + 1 m does not fit 16 bits, 64 m + 1 m does
    out = run("q_beyond")
    assert set(np.unique(out)) == {0, 65000}
    out = run("partly_outside")
    assert 0.1 < (out == 0).mean() < 0.9
    # a corner at or beyond 2^30, or not finite, drops the pixel
    for name in ("limit_corner_inside", "not_finite"):
        assert not run(name).any(), name
    assert run("straddle").any()
    # rint rounds half to even: 62.5 -> 62, 187.5 -> 188, 312.5 -> 312, ... where half away from zero gives 63, 188, 313, ...
    g, d = by_name["ties"]
    out = run("ties")
    assert out.reshape(-1)[:8].tolist() == [62, 188, 312, 438, 562, 688, 812, 938]
    assert (out != np.floor(d.astype(np.float64) * 1000.0 + 0.5)).mean() >= 1.0 / 3.0
    # q = 0 is no measurement: 0.0005f (a little above 0.0005) is the smallest that is kept, a subnormal is not
    g, d = by_name["tiny"]
    out = run("tiny")
    assert np.array_equal(out, (d == np.float32(0.0005)).astype(np.uint16)) and out.any()
    # has_Dc5 = 0 with the numbers in place: as without them, and not as with them
    g, d = by_name["dc5_ignored"]
    g0 = by_name["rot_dist_ramp"][0]
    assert c_rig(g).has_Dc5 == 0 and list(c_rig(g).Dc5) == g0["Dc5"]
    plain = capi.depth_register_host(c_rig(dr.rig(g0["depth_shape"], g0["Kd4"], g0["Kc4"], R=g0["R"], t=g0["t"])), d, rows, cols)
    assert np.array_equal(run("dc5_ignored"), plain) and not np.array_equal(plain, run("rot_dist_ramp"))
    # depth images of one pixel, one row, one column: a plane stays that plane wherever it lands
    for shape in dr.SHAPES:
        out = run("shape_%dx%d" % shape)
        assert out.any() and np.all(out[out != 0] == 1500), shape
    # a depth image 16 x 16 times finer than the colour image: the nearest of the few that write
    g, d = dr.many_to_one(rows, cols)
    out = capi.depth_register_host(c_rig(g), d, *dr.MANY_SHAPE)
    w = dr.writers(g, d, *dr.MANY_SHAPE)
    assert all(out[y, x] == min(v) for (y, x), v in w.items()) and int((out != 0).sum()) == len(w)
    for name in ("contended", "pile_up"):                                       # a few and a hundred and more writers on one pixel
        g, d = by_name[name]
        out, w = run(name), dr.writers(g, d, rows, cols)
        assert all(out[y, x] == min(v) for (y, x), v in w.items()) and int((out != 0).sum()) == len(w), name


PLANE_N = np.array([0.25, -0.15, 1.0]) / np.linalg.norm([0.25, -0.15, 1.0])
PLANE_D = 1.8                                                                    # the plane n . X = 1.8 in the depth camera's frame
TRUTH_ROLLS = (None, 0.0, 0.01, 0.03)                                            # None: no rotation at all
TRUTH_SHAPES = ((96, 128), (60, 80), (72, 96), (192, 256))


def plane_rig(depth_shape, roll, rows=96, cols=128):
    Kc = dr.colour_K(rows, cols)
    R = np.eye(3) if roll is None else dr.rot("z", roll) @ dr.rot("y", 0.03) @ dr.rot("x", -0.02)
    return dr.rig(depth_shape, dr.scaled_K(Kc, (rows, cols), depth_shape), Kc, R=R, t=[0.05, -0.01, 0.005])


def plane_scene(g, rows=96, cols=128):
    """(raw 16-bit image of the plane as the depth camera of rig g sees it, the depth in millimetres along each colour pixel's ray,
    the colour pixels whose surface point the depth camera sees more than one pixel inside its image): analytic, nothing of the
    definition in it"""
    fxd, fyd, cxd, cyd = g["Kd4"]
    fxc, fyc, cxc, cyc = g["Kc4"]
    dr_, dc_ = g["depth_shape"]
    v, u = np.mgrid[0:dr_, 0:dc_].astype(np.float64)
    raw = np.rint(1000.0 * PLANE_D / (PLANE_N[0] * (u - cxd) / fxd + PLANE_N[1] * (v - cyd) / fyd + PLANE_N[2]))
    assert raw.min() >= 1 and raw.max() <= 65535
    # X_colour = R X_depth + t: the plane is (R n) . X_colour = d + (R n) . t there
    nc = g["R"] @ PLANE_N
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ray = np.stack([(u - cxc) / fxc, (v - cyc) / fyc, np.ones_like(u)], -1)
    Zc = (PLANE_D + nc @ g["t"]) / (ray @ nc)
    Xd = (ray * Zc[..., None] - g["t"]) @ g["R"]                                 # R^T (X_colour - t), row-wise
    ud, vd = fxd * Xd[..., 0] / Xd[..., 2] + cxd, fyd * Xd[..., 1] / Xd[..., 2] + cyd
    seen = (Zc > 0) & (Xd[..., 2] > 0) & (ud > 0.5) & (ud < dc_ - 1.5) & (vd > 0.5) & (vd < dr_ - 1.5)      # pixels span -0.5 .. n - 0.5
    return raw.astype(np.uint16), Zc * 1000.0, seen


def neighbour_step(raw):
    """the largest difference between 8-neighbours of a raw image"""
    r = raw.astype(np.int64)
    return int(max(np.abs(r[1:] - r[:-1]).max(), np.abs(r[:, 1:] - r[:, :-1]).max(), np.abs(r[1:, 1:] - r[:-1, :-1]).max(),
                   np.abs(r[1:, :-1] - r[:-1, 1:]).max()))


def test_registered_depth_against_a_ray_cast_plane():
    """Registration against geometry it did not write itself: a slanted plane, the raw image its analytic depth per depth pixel
    (rounded to millimetres), the truth the analytic intersection of every colour pixel's ray with that plane.  Every covered colour
    pixel the depth camera sees is within S + 1 mm of the truth, S the largest step between 8-neighbours of the raw image (from the
    input, not from any output): a colour pixel inside a footprint sees a surface point of that depth pixel's cell or of a direct
    neighbour's, half a millimetre of rounding goes in and half comes out.  At least 90 % of the seen pixels are covered.

    Measured (host builder = restatement; worst error in mm / S / hole share of the seen pixels), depth geometry by rotation:

                   none               yaw, pitch         + roll 0.01        + roll 0.03
        96 x 128   3.1 /  9 / 1.3 %   3.9 /  9 / 0.8 %   4.3 /  9 / 1.7 %   4.3 /  9 / 3.7 %
        60 x 80    6.3 / 14 / 0.8 %   6.8 / 14 / 1.0 %   6.8 / 14 / 1.6 %   6.2 / 14 / 3.7 %
        72 x 96    4.8 / 12 / 0.7 %   5.4 / 12 / 0.9 %   5.5 / 12 / 1.7 %   5.4 / 12 / 3.6 %
        192 x 256  2.0 /  5 / 0.7 %   2.4 /  5 / 1.0 %   2.5 /  5 / 1.4 %   2.6 /  5 / 3.5 %

    and the hole share of the 96 x 128 rig by roll (with the yaw and pitch above), which is about the roll in radians -- the two
    corners of a rolled pixel span a box that loses width: 0.8 % at 0, 1.7 % at 0.01, 3.7 % at 0.03, 10.8 % at 0.1, 28.6 % at 0.3,
    98.6 % at pi / 4 (the table of INTEGRATION.md).  Printed below, asserted only to grow with the roll."""
    from rgbd_odometry_amd import capi
    rows, cols = 96, 128
    for shape in TRUTH_SHAPES:
        for roll in TRUTH_ROLLS:
            g = plane_rig(shape, roll)
            raw, truth, seen = plane_scene(g)
            S = neighbour_step(raw)
            out = capi.depth_register_host(c_rig(g), raw, rows, cols)
            assert np.array_equal(out, dr.register(g, raw, rows, cols))
            m = seen & (out != 0)
            err = np.abs(out.astype(np.float64) - truth)[m]
            holes = 1.0 - m.sum() / seen.sum()
            print("plane %dx%d roll %s: %d seen, worst error %.1f mm, S = %d, hole share %.1f %%" % (shape + (roll, seen.sum(), err.max(), S, 100 * holes)))
            assert seen.mean() > 0.5 and 1 <= S <= 20
            assert err.max() <= S + 1, (shape, roll, float(err.max()), S)
            assert holes <= 0.10, (shape, roll, holes)
    shares = []
    for roll in (0.0, 0.01, 0.03, 0.1, 0.3, np.pi / 4):
        g = plane_rig((96, 128), roll)
        raw, truth, seen = plane_scene(g)
        out = capi.depth_register_host(c_rig(g), raw, rows, cols)
        shares.append(1.0 - (seen & (out != 0)).sum() / seen.sum())
        print("plane 96x128 roll %.4f: hole share of the seen pixels %.1f %%" % (roll, 100 * shares[-1]))
    assert all(a < b for a, b in zip(shares, shares[1:])), shares


def test_refusals_of_the_host_builder():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    rows, cols = 24, 32
    K = dr.colour_K(rows, cols)
    depth = np.full((rows, cols), 1000, np.uint16)
    out = np.full((rows, cols), 0xABCD, np.uint16)

    def call(rig_edit=None, rig_null=False, depth_null=False, out_null=False, fmt=capi.DVO_DEPTH_U16, r=rows, c=cols):
        g = capi.DvoDepthRig.make((rows, cols), K, K, Dc5=[0.1, 0, 0, 0, 0])
        if rig_edit:
            rig_edit(g)
        return lib.dvo_depth_register_host(None if rig_null else C.byref(g), None if depth_null else capi._ptr(depth), fmt, r, c,
                                           None if out_null else capi._ptr(out))

    def setter(field, index, value):
        def edit(g):
            if index is None:
                setattr(g, field, value)
            else:
                getattr(g, field)[index] = value
        return edit

    assert call() == capi.DVO_OK and out[12, 16] == 1000
    out[:] = 0xABCD
    bad = [dict(rig_null=True), dict(depth_null=True), dict(out_null=True), dict(r=0), dict(c=0), dict(r=-3), dict(fmt=2), dict(fmt=-1),
           dict(rig_edit=setter("depth_rows", None, 0)), dict(rig_edit=setter("depth_cols", None, -1)),
           dict(rig_edit=setter("has_Dc5", None, 2)), dict(rig_edit=setter("has_Dc5", None, -1))]
    for field, index in (("Kd4", 0), ("Kd4", 1), ("Kc4", 0), ("Kc4", 1)):
        bad += [dict(rig_edit=setter(field, index, 0.0)), dict(rig_edit=setter(field, index, -100.0))]
    for field, n in (("Kd4", 4), ("R", 9), ("t", 3), ("Kc4", 4), ("Dc5", 5)):
        for index in range(n):
            for value in (float("nan"), float("inf"), float("-inf")):
                bad.append(dict(rig_edit=setter(field, index, value)))
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
    assert np.all(out == 0xABCD), "a refused call must write nothing"
    with pytest.raises(capi.DvoError) as ei:
        capi.depth_register_host(capi.DvoDepthRig.make((rows, cols), [0, 1, 0, 0], K), depth, rows, cols)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.depth_register_host(capi.DvoDepthRig.make((rows, cols + 1), K, K), depth, rows, cols)
    # R is taken as given: a matrix that is no rotation is not refused
    assert call(rig_edit=setter("R", 0, 2.0)) == capi.DVO_OK


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in ("dvo_depth_register_host", "dvo_frames_set_pair_depth_rig", "dvo_frames_register_depth", "dvo_frames_get_registered_depth",
                 "dvo_tracker_set_stream_depth_rig", "dvo_tracker_step_raw_depth"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    for macro, value in (("DVO_DEPTH_SPLAT_MAX", capi.DVO_DEPTH_SPLAT_MAX), ("DVO_DEPTH_REGISTER_LAUNCHES", capi.DVO_DEPTH_REGISTER_LAUNCHES)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == value
    assert capi.DVO_DEPTH_SPLAT_MAX == dr.SPLAT_MAX
    # the rig is declared twice under one guard (the public header and the definition's own): the two texts must be the same
    own = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_depth_register.h")).read(), flags=re.S)
    pat = r"typedef struct dvo_depth_rig \{.*?\} dvo_depth_rig;"
    assert re.search(pat, text, re.S).group(0).split() == re.search(pat, own, re.S).group(0).split()


def test_rig_layout_matches_header(tmp_path):
    """the ctypes mirror must have the layout the C compiler gives dvo_depth_rig"""
    from rgbd_odometry_amd import capi
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu", '
                   'sizeof(dvo_depth_rig), offsetof(dvo_depth_rig, Kd4), offsetof(dvo_depth_rig, t), offsetof(dvo_depth_rig, has_Dc5), '
                   'offsetof(dvo_depth_rig, Dc5));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, kd, t, has, dc = (int(x) for x in subprocess.check_output([exe]).split())
    R = capi.DvoDepthRig
    assert (C.sizeof(R), R.Kd4.offset, R.t.offset, R.has_Dc5.offset, R.Dc5.offset) == (size, kd, t, has, dc)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_register")
    exe = str(d / "depth_register_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "depth_register_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/depth_register_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def run_program(host_program, rig, depth, fmt, rows, cols):
    d, exe = host_program
    rig_path, depth_path = str(d / "rig.bin"), str(d / "depth.bin")
    open(rig_path, "wb").write(bytes(rig))
    np.ascontiguousarray(depth).tofile(depth_path)
    run = subprocess.run([exe, rig_path, depth_path, str(fmt), str(rows), str(cols)], capture_output=True, text=True, timeout=60)
    if run.returncode == 3:
        assert run.stdout.strip() == "refused"
        return None
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    tag, r, c = lines[0].split()
    assert tag == "image" and (int(r), int(c)) == (rows, cols)
    return np.frombuffer(bytes.fromhex(lines[1]), ">u2").astype(np.uint16).reshape(rows, cols)


@pytest.mark.parametrize("rows,cols", SIZES)
def test_builder_under_sanitizers(host_program, rows, cols):
    """the same code the library compiles, with the depth image and the output allocated to their exact sizes: byte-equal to the
    restatement and clean under -fsanitize=address,undefined"""
    from rgbd_odometry_amd import capi
    for name, g, depth, (cr, cc) in dr.all_cases(rows, cols):
        for tag, d in formats_of(depth):
            got = run_program(host_program, c_rig(g), d, capi.DVO_DEPTH_U16 if tag == "u16" else capi.DVO_DEPTH_F32, cr, cc)
            assert got is not None and np.array_equal(got, dr.register(g, d, cr, cc)), (name, tag)


def test_program_refuses_what_the_builder_refuses(host_program):
    from rgbd_odometry_amd import capi
    rows, cols = 24, 32
    K = dr.colour_K(rows, cols)
    depth = np.full((rows, cols), 1000, np.uint16)
    mk = lambda **kw: capi.DvoDepthRig.make((rows, cols), kw.get("Kd", K), kw.get("Kc", K), t=kw.get("t"), Dc5=kw.get("Dc5"))
    assert run_program(host_program, mk(), depth, 1, rows, cols) is not None
    for rig in (mk(Kd=[0, 1, 0, 0]), mk(Kc=[1, -1, 0, 0]), mk(t=[float("nan"), 0, 0]), mk(Dc5=[0, 0, float("inf"), 0, 0])):
        assert run_program(host_program, rig, depth, 1, rows, cols) is None
    g = mk()
    g.has_Dc5 = 3
    assert run_program(host_program, g, depth, 1, rows, cols) is None
    g = mk()
    g.depth_rows = 0
    assert run_program(host_program, g, depth, 1, rows, cols) is None
    for fmt, r, c in ((2, rows, cols), (1, 0, cols), (1, rows, -1)):
        assert run_program(host_program, mk(), depth, fmt, r, c) is None
