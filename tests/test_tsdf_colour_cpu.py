"""Colour in the map on the CPU (include/dvo_amd.h, "colour in the map"): the three host definitions against the numpy restatement
(tests/tsdf_colour_reference.py) on every case and in every image format, their uncoloured results against the uncoloured definitions,
rounding and limits, conditions that keep the cases from being vacuous, capacities with guard values, every refusal, the symbols, the
PLY writer, and the definition's own code (rgbd_odometry_amd/csrc/dvo_tsdf_colour.h) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/host/tsdf_colour_main.cpp) and the C++ mirror (tests/host/tsdf_colour_hpp_main.cpp).  No GPU.
Comparisons are byte equality unless a bound is stated."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_colour_reference as cr
import tsdf_map_reference as tr
import tsdf_mesh_reference as mr
import tsdf_raycast_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_FORMATS = ["bgr8", "rgb8", "mono8"]
NEW_SYMBOLS = ["dvo_colour_integrate_host", "dvo_colour_raycast_host", "dvo_colour_mesh_host", "dvo_colour_enable", "dvo_colour_integrate",
               "dvo_colour_get_words", "dvo_colour_set_words", "dvo_colour_raycast_views", "dvo_colour_mesh_extract"]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def frames_of(vi, depth="u16"):
    imgs, poses = tr.frame_list(depth)
    idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
    return idx, [imgs[i] for i in idx], poses[idx]


def host_integrate(vol, words, colours, depths, images, fmt, K, poses, **params):
    """dvo_colour_integrate_host with the restatement's signature"""
    from rgbd_odometry_amd import capi
    p = capi.DvoTsdfParams.default(**params)
    return capi.tsdf_integrate_colour_host(c_volume(vol), words, colours, depths, images, K, poses, image_format=fmt, params=p)


# ---- 1, 2: the host definitions, the restatement and the uncoloured definitions ----

@pytest.mark.parametrize("depth", ["u16", "f32"])
@pytest.mark.parametrize("fmt", IMAGE_FORMATS)
@pytest.mark.parametrize("kind", ["random", "gradient"])
def test_fusion_equals_the_restatement(kind, fmt, depth):
    from rgbd_odometry_amd import capi
    cols = cr.images(kind, fmt)
    for vi, (vol, w, c) in enumerate(cr.fused(kind, fmt, depth)):
        idx, imgs, poses = frames_of(vi, depth)
        hw, hc = capi.tsdf_integrate_colour_host(c_volume(vol), None, None, imgs, [cols[i] for i in idx], tr.K4, poses, image_format=fmt)
        assert same_bits(hw, w) and same_bits(hc, c), vi
        assert same_bits(hw, capi.tsdf_integrate_host(c_volume(vol), None, imgs, tr.K4, poses)), vi
        # one call per frame from the state of the last gives the same words
        sw, sc = None, None
        for k, i in enumerate(idx):
            sw, sc = capi.tsdf_integrate_colour_host(c_volume(vol), sw, sc, [imgs[k]], [cols[i]], tr.K4, poses[k:k + 1], image_format=fmt)
        assert same_bits(sw, w) and same_bits(sc, c), vi


@pytest.mark.parametrize("depth", ["u16", "f32"])
@pytest.mark.parametrize("fmt", IMAGE_FORMATS)
def test_fusion_equals_the_restatement_at_37_x_53(fmt, depth):
    """an odd image size: 1961 bytes of mono8 and 5883 of rgb8 or bgr8 beside 3922 or 7844 of depth, a row pitch that is no power of
    two.  Every volume takes colour"""
    from rgbd_odometry_amd import capi
    rows, cols = tr.ODD_SIZE
    imgs, poses = tr.frame_list(depth, tr.ODD_SIZE)
    cols8 = cr.images("random" if depth == "u16" else "gradient", fmt, tr.ODD_SIZE)
    K = tr.k4_for(rows, cols)
    assert cols8[0].shape == (tr.ODD_SIZE if fmt == "mono8" else tr.ODD_SIZE + (3,)) and cols8[0].nbytes % 16
    for vi, vol in enumerate(tr.VOLUMES):
        idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
        w, c = cr.integrate(vol, None, None, [imgs[i] for i in idx], [cols8[i] for i in idx], cr.FORMATS[fmt], K, poses[idx])
        hw, hc = capi.tsdf_integrate_colour_host(c_volume(vol), None, None, [imgs[i] for i in idx], [cols8[i] for i in idx], K, poses[idx], image_format=fmt)
        assert same_bits(hw, w) and same_bits(hc, c), (vi, int((hw != w).sum()), int((hc != c).sum()))
        assert same_bits(hw, tr.integrate(vol, None, [imgs[i] for i in idx], K, poses[idx])), vi
        coloured = int((cr.colour_wc(c) > 0).sum())
        print("volume %d: %d of %d voxels coloured" % (vi, coloured, c.size))
        assert coloured >= (200, 2000, 5, 1)[vi] and len(np.unique(c)) > min(coloured, 100) // 2, (vi, coloured)


_views = {}


def view_reference(key, vol, words, colours, pose, rows=tr.ROWS, cols=tr.COLS, **settings):
    if key not in _views:
        _views[key] = cr.raycast_view(vol, words, colours, rr.k4_for(rows, cols), pose, rows, cols, **settings)
    return _views[key]


def check_views(tag, vol, words, colours, views, rows=tr.ROWS, cols=tr.COLS, **settings):
    """every view, both depth formats, the three image formats: image, depth and normals; returns (hit pixels, coloured hit pixels)"""
    from rgbd_odometry_amd import capi
    p = capi.DvoRaycastParams.default(**settings)
    hits = coloured = 0
    for name, pose in views:
        ref = view_reference((tag, name, rows, cols, tuple(sorted(settings.items()))), vol, words, colours, pose, rows, cols, **settings)
        hits += int((ref["kind"] == rr.HIT).sum())
        coloured += int((ref["levels_f32"].sum(axis=-1) > 0).sum())
        for dfmt in ("u16", "f32"):
            plain_d, plain_n = capi.tsdf_raycast_host(c_volume(vol), words, rr.k4_for(rows, cols), pose[None], rows, cols, params=p, fmt=dfmt, normals=True)
            for ifmt in IMAGE_FORMATS:
                d, n, img = capi.tsdf_raycast_colour_host(c_volume(vol), words, colours, rr.k4_for(rows, cols), pose[None], rows, cols, params=p, fmt=dfmt,
                                                          image_format=ifmt, normals=True)
                assert same_bits(img[0], cr.image_of_levels(ref["levels_" + dfmt], cr.FORMATS[ifmt])), (tag, name, dfmt, ifmt)
                assert same_bits(d[0], ref[dfmt]) and same_bits(n[0], ref["normals_" + dfmt]), (tag, name, dfmt, ifmt)
                assert same_bits(d, plain_d) and same_bits(n, plain_n), (tag, name, dfmt, ifmt)
            d, img = capi.tsdf_raycast_colour_host(c_volume(vol), words, colours, rr.k4_for(rows, cols), pose[None], rows, cols, params=p, fmt=dfmt)
            assert same_bits(d, plain_d) and same_bits(img[0], cr.image_of_levels(ref["levels_" + dfmt], cr.BGR8))
    return hits, coloured


@pytest.mark.parametrize("vi", [0, 1, 2, 3])
def test_raycast_equals_the_restatement(vi):
    vol, w, c = cr.fused()[vi]
    check_views("fused%d" % vi, vol, w, c, rr.view_list(vol))


def test_raycast_of_other_states():
    """gradient images; random words with random colour words (corners without colour inside valid samples); min_weight 2 and another
    step; an image size of its own"""
    vol, w, c = cr.fused("gradient", "rgb8")[1]
    check_views("gradient1", vol, w, c, rr.view_list(vol)[:3])
    vol = tr.VOLUMES[1]
    w, c = rr.random_words(vol), cr.random_colours(vol)
    hits, coloured = check_views("random1", vol, w, c, rr.view_list(vol)[:3], step_trunc=0.25, min_weight=2)
    assert 0 < coloured < hits
    vol, w, c = cr.fused()[0]
    check_views("fused0", vol, w, c, rr.view_list(vol)[:2], rows=17, cols=19)


def test_several_views_in_one_call():
    from rgbd_odometry_amd import capi
    vol, w, c = cr.fused()[0]
    poses = np.stack([p for _, p in rr.view_list(vol)])
    d, n, img = capi.tsdf_raycast_colour_host(c_volume(vol), w, c, tr.K4, poses, tr.ROWS, tr.COLS, fmt="u16", image_format="rgb8", normals=True)
    for k, (name, pose) in enumerate(rr.view_list(vol)):
        ref = view_reference(("fused0", name, tr.ROWS, tr.COLS, ()), vol, w, c, pose)
        assert same_bits(img[k], cr.image_of_levels(ref["levels_u16"], cr.RGB8)) and same_bits(d[k], ref["u16"]), name


_host_mesh = {}


def host_mesh(name, min_weight):
    from rgbd_odometry_amd import capi
    if (name, min_weight) not in _host_mesh:
        vol, words, colours = cr.mesh_case(name)
        _host_mesh[(name, min_weight)] = capi.tsdf_mesh_colour_host(c_volume(vol), words, colours, min_weight)
    return _host_mesh[(name, min_weight)]


@pytest.mark.parametrize("name,min_weight", cr.MESH_CASES)
def test_mesh_equals_the_restatement(name, min_weight):
    from rgbd_odometry_amd import capi
    vol, words, colours = cr.mesh_case(name)
    v, t, rgb = host_mesh(name, min_weight)
    rv, rt, rrgb, ends = cr.mesh_reference(name, min_weight)
    print("%s at min_weight %d: %d vertices, coloured ends %s" % (name, min_weight, len(v), np.bincount(ends, minlength=3)))
    assert same_bits(rgb, rrgb), int((rgb != rrgb).any(axis=1).sum())
    assert same_bits(v, rv) and same_bits(t, rt)
    pv, pt = capi.tsdf_mesh_host(c_volume(vol), words, min_weight)
    assert same_bits(v, pv) and same_bits(t, pt)


# ---- 3: rounding and limits ----

def test_rounding_and_limits():
    cr.check_rounding_and_limits(host_integrate)


# ---- 3b: the packed pool of tests/tsdf_map_reference.py, with colour words ----

def test_restatement_on_the_packed_volumes():
    """tr.PACKED_FRAMES into every packed volume, from cleared and from random words and colour words: host definition = restatement"""
    from rgbd_odometry_amd import capi
    imgs, poses = tr.frame_list("u16")
    idx = list(tr.PACKED_FRAMES)
    for fmt in IMAGE_FORMATS:
        pics = cr.images("random", fmt)
        for vi, vol in enumerate(tr.PACKED_VOLUMES):
            rng = np.random.RandomState(100 + vi)
            for w0, c0 in ((None, None), (tr.random_pool_words(rng, tr.voxels_of(vol)), tr.random_pool_colours(rng, tr.voxels_of(vol)))):
                hw, hc = capi.tsdf_integrate_colour_host(c_volume(vol), w0, c0, [imgs[i] for i in idx], [pics[i] for i in idx], tr.K4, poses[idx],
                                                         image_format=fmt)
                w, c = cr.integrate(vol, w0, c0, [imgs[i] for i in idx], [pics[i] for i in idx], cr.FORMATS[fmt], tr.K4, poses[idx])
                assert same_bits(hw, w) and same_bits(hc, c), (fmt, vi, w0 is None)
            assert cr.colour_wc(c).any() or w0 is None, vi


def test_random_pool_colours_are_colour_words():
    c = tr.random_pool_colours(np.random.RandomState(1), 4000)
    assert cr.colour_wc(c).max() == tr.MAX_WEIGHT and (cr.colour_wc(c) == 0).any() and np.all(c[cr.colour_wc(c) == 0] == 0)
    assert all(0 <= cr.colour_channel(c, ch).min() and 65000 < cr.colour_channel(c, ch).max() <= 65280 for ch in range(3))


@pytest.mark.parametrize("fmt", IMAGE_FORMATS)
def test_packed_pool(fmt):
    """tr.check_packed_pool with integrate_colour against a Python stand-in that applies the host definition per volume"""
    tr.check_packed_pool(lambda vols: tr.FakePool(vols, colour=True), image_format=fmt, formats=("u16",) if fmt != "bgr8" else ("u16", "f32"))


@pytest.mark.parametrize("fault, assertion", [("whole_groups", r"unlisted volume \d+ changed"),
                                              ("no_wrap", r"listed volume \d+ differs from the host definition"),
                                              ("reversed", r"listed volume \d+ differs from the host definition")])
def test_packed_pool_sees_a_wrong_handle(fault, assertion):
    """the three wrong stand-ins of tests/test_tsdf_map_cpu.py with colour words, and the assertion each one fails"""
    with pytest.raises(AssertionError, match="^" + assertion):
        tr.check_packed_pool(lambda vols: tr.FakePool(vols, colour=True, fault=fault), image_format="rgb8")


def test_packed_pool_sees_wrong_colour_words_alone():
    """a stand-in whose depth words are right and whose colour words alone are stored in whole groups"""
    with pytest.raises(AssertionError, match=r"^unlisted volume \d+: colour words changed"):
        tr.check_packed_pool(lambda vols: tr.FakePool(vols, colour=True, fault="whole_colour_groups"), image_format="bgr8")


# ---- 4: the cases are not vacuous ----

def test_cases_are_not_vacuous():
    """the figures of a CPU prototype of the band rule on these volumes and frames: 436 of 436 and 2339 of 2356 axis crossings with colour
    at both ends, 17 with one end, 33 of 2083 surface cells with a corner without colour"""
    both = {}
    for name in ("volume0", "volume1"):
        ends = cr.mesh_reference(name, 1)[3]
        axis = mr.reference(name, 1)[2] < 3
        both[name] = (int((ends[axis] == 2).sum()), int((ends[axis] == 1).sum()), int(axis.sum()))
        print(name, both[name])
        assert both[name][0] >= 0.95 * both[name][2]
    assert both["volume0"][2] == 436 and both["volume1"][2] == 2356
    assert both["volume1"][1] >= 1
    vol, w, c = cr.fused()[1]
    nx, ny, nz = vol["dims"]
    W, Cw = w.reshape(nz, ny, nx), c.reshape(nz, ny, nx)
    cell = lambda a, k: a[(k >> 2) & 1:nz - 1 + ((k >> 2) & 1), (k >> 1) & 1:ny - 1 + ((k >> 1) & 1), (k & 1):nx - 1 + (k & 1)]
    valid = np.all([cell(tr.word_w(W) >= 1, k) for k in range(8)], axis=0)
    neg = np.array([cell(tr.word_q(W) < 0, k) for k in range(8)])
    surface = valid & neg.any(axis=0) & ~neg.all(axis=0)
    uncoloured = surface & ~np.all([cell(cr.colour_wc(Cw) >= 1, k) for k in range(8)], axis=0)
    print("volume1: %d surface cells, %d with a corner without colour" % (surface.sum(), uncoloured.sum()))
    assert surface.sum() > 1000 and uncoloured.sum() >= 1
    hits = coloured = 0
    for vi in (0, 1):
        vol, w, c = cr.fused()[vi]
        for name, pose in rr.view_list(vol):
            ref = view_reference(("fused%d" % vi, name, tr.ROWS, tr.COLS, ()), vol, w, c, pose)
            hits += int((ref["kind"] == rr.HIT).sum())
            coloured += int((ref["levels_f32"].sum(axis=-1) > 0).sum())
    print("ray cast: %d hit pixels, %d with colour" % (hits, coloured))
    assert hits > 5000 and coloured >= 0.90 * hits
    # random1: vertices with no, one and two coloured ends all occur
    assert np.all(np.bincount(cr.mesh_reference("random1", 1)[3], minlength=3) >= 1000)


# ---- 5: capacities ----

@pytest.mark.parametrize("name,min_weight", [("volume0", 1), ("random1", 2), ("volume2", 1), ("SPHERE", 1)])
def test_capacities(name, min_weight):
    """zero, exact, one short and short on one side only: the written prefix is the full result's, nothing beyond it is touched, the
    counts are always the full counts"""
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol, words, colours = cr.mesh_case(name)
    v, t, rgb = host_mesh(name, min_weight)
    nv, nt = len(v), len(t)
    guard = 3
    for vcap, tcap in [(0, 0), (nv, nt), (max(nv - 1, 0), max(nt - 1, 0)), (max(nv - 1, 0), nt), (nv, max(nt - 1, 0)), (nv // 2, nt), (0, nt), (nv, 0),
                       (nv + 2, nt + 2)]:
        xyz = np.full((vcap + guard, 3), -7.5, np.float32)
        col = np.full((vcap + guard, 3), 0xA5, np.uint8)
        tri = np.full((tcap + guard, 3), -77, np.int32)
        gv, gt = C.c_longlong(-5), C.c_longlong(-6)
        rc = lib.dvo_colour_mesh_host(C.byref(c_volume(vol)), capi._ptr(words), capi._ptr(colours), min_weight, capi._ptr(xyz) if vcap else None,
                                      capi._ptr(col) if vcap else None, vcap, capi._ptr(tri) if tcap else None, tcap, C.byref(gv), C.byref(gt))
        assert rc == capi.DVO_OK and (gv.value, gt.value) == (nv, nt), (vcap, tcap)
        kv, kt = min(vcap, nv), min(tcap, nt)
        assert same_bits(xyz[:kv], v[:kv]) and same_bits(col[:kv], rgb[:kv]) and same_bits(tri[:kt], t[:kt]), (vcap, tcap)
        assert np.all(xyz[kv:] == -7.5) and np.all(col[kv:] == 0xA5) and np.all(tri[kt:] == -77), (vcap, tcap)


# ---- 6: refusals ----

def setter(field, value, index=None):
    def edit(o):
        if index is None:
            setattr(o, field, value)
        else:
            getattr(o, field)[index] = value
    return edit


NAN, INF = float("nan"), float("inf")


def bad_volumes():
    from rgbd_odometry_amd import capi
    bad = []
    for field in ("nx", "ny", "nz"):
        bad += [setter(field, 0), setter(field, -1), setter(field, capi.DVO_TSDF_MAX_DIM + 1)]
    for field in ("voxel_size", "trunc"):
        bad += [setter(field, value) for value in (0.0, -0.1, NAN, INF)]
    return bad + [setter("origin", value, k) for k in range(3) for value in (NAN, INF, -INF)]


def test_refusals_of_the_fusion():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol = tr.VOLUMES[2]
    n = tr.voxels_of(vol)
    words, colours = np.full(n, 7, np.uint32), np.full(n, 9, np.uint64)
    depth = [tr.scene_u16(0), tr.scene_u16(1)]
    image = cr.images("random", "bgr8")[:2]
    K = np.tile(np.array(tr.K4), (2, 1))
    P = np.stack(tr.POSES[:2])

    def call(null=(), count=2, dfmt=capi.DVO_DEPTH_U16, ifmt=capi.DVO_CAM_BGR8, rows=tr.ROWS, cols=tr.COLS, vol_edit=None, p_edit=None, K_=K, P_=P):
        v, p = c_volume(vol), capi.DvoTsdfParams.default()
        if vol_edit:
            vol_edit(v)
        if p_edit:
            p_edit(p)
        dp = (C.c_void_p * 2)(depth[0].ctypes.data, None if "depth1" in null else depth[1].ctypes.data)
        ip = (C.c_void_p * 2)(image[0].ctypes.data, None if "image1" in null else image[1].ctypes.data)
        K_, P_ = np.ascontiguousarray(K_), np.ascontiguousarray(P_)
        return lib.dvo_colour_integrate_host(None if "vol" in null else C.byref(v), None if "voxels" in null else capi._ptr(words),
                                             None if "colours" in null else capi._ptr(colours), None if "params" in null else C.byref(p), count,
                                             None if "depth" in null else dp, dfmt, None if "image" in null else ip, ifmt, rows, cols,
                                             None if "K4" in null else capi._ptr(K_), None if "poses" in null else capi._ptr(P_))

    bad = [dict(null=(k,)) for k in ("vol", "voxels", "colours", "params", "depth", "image", "depth1", "image1", "K4", "poses")]
    bad += [dict(count=0), dict(count=-1), dict(rows=0), dict(cols=0), dict(dfmt=2), dict(dfmt=-1), dict(ifmt=3), dict(ifmt=-1)]
    bad += [dict(vol_edit=e) for e in bad_volumes()]
    bad += [dict(p_edit=setter("z_near", 0.0)), dict(p_edit=setter("z_far", 0.05)), dict(p_edit=setter("z_near", NAN)), dict(p_edit=setter("max_weight", 0)),
            dict(p_edit=setter("max_weight", 65536))]
    Kb, Pb = K.copy(), P.copy()
    Kb[1, 0] = 0.0
    Pb[1, 4] = NAN
    bad += [dict(K_=Kb), dict(P_=Pb)]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
        assert np.all(words == 7) and np.all(colours == 9), kw
    assert call() == capi.DVO_OK and not np.all(words == 7)
    with pytest.raises(capi.DvoError) as ei:
        capi.tsdf_integrate_colour_host(c_volume(dict(vol, trunc=0.0)), None, None, depth, image, tr.K4, P)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.tsdf_integrate_colour_host(c_volume(vol), None, None, depth, image[:1], tr.K4, P)
    with pytest.raises(ValueError):
        capi.tsdf_integrate_colour_host(c_volume(vol), None, None, depth, image, tr.K4, P, image_format="mono8")     # three channels given
    with pytest.raises(ValueError):
        capi.tsdf_integrate_colour_host(c_volume(vol), None, np.zeros(n - 1, np.uint64), depth, image, tr.K4, P)
    with pytest.raises(ValueError):
        capi.tsdf_integrate_colour_host(c_volume(vol), None, None, depth, image, tr.K4, P, image_format="yuv")


def test_refusals_of_the_ray_cast():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol, words, colours = cr.fused()[0]
    rows, cols = 5, 6
    depth = np.full((2, rows, cols), 7, np.uint16)
    nrm = np.full((2, rows, cols, 3), 7.0, np.float32)
    img = np.full((2, rows, cols, 3), 7, np.uint8)
    K = np.tile(np.array(tr.K4), (2, 1))
    P = np.stack(tr.POSES[:2])

    def call(null=(), count=2, dfmt=capi.DVO_DEPTH_U16, ifmt=capi.DVO_CAM_RGB8, rows_=rows, cols_=cols, vol_edit=None, p_edit=None, K_=K, P_=P):
        v, p = c_volume(vol), capi.DvoRaycastParams.default()
        if vol_edit:
            vol_edit(v)
        if p_edit:
            p_edit(p)
        dp = (C.c_void_p * 2)(depth[0].ctypes.data, None if "depth1" in null else depth[1].ctypes.data)
        np_ = (C.c_void_p * 2)(nrm[0].ctypes.data, None if "normals1" in null else nrm[1].ctypes.data)
        ip = (C.c_void_p * 2)(img[0].ctypes.data, None if "image1" in null else img[1].ctypes.data)
        K_, P_ = np.ascontiguousarray(K_), np.ascontiguousarray(P_)
        return lib.dvo_colour_raycast_host(None if "vol" in null else C.byref(v), None if "voxels" in null else capi._ptr(words),
                                           None if "colours" in null else capi._ptr(colours), None if "params" in null else C.byref(p), count, dfmt,
                                           rows_, cols_, None if "K4" in null else capi._ptr(K_), None if "poses" in null else capi._ptr(P_),
                                           None if "depth" in null else dp, None if "normals" in null else np_, None if "image" in null else ip, ifmt)

    bad = [dict(null=(k,)) for k in ("vol", "voxels", "colours", "params", "depth", "image", "depth1", "normals1", "image1", "K4", "poses")]
    bad += [dict(count=0), dict(rows_=0), dict(cols_=-1), dict(dfmt=2), dict(ifmt=3), dict(ifmt=-1)]
    bad += [dict(vol_edit=e) for e in bad_volumes()]
    bad += [dict(p_edit=setter("z_near", 0.0)), dict(p_edit=setter("step_trunc", 0.0)), dict(p_edit=setter("step_trunc", 1.5)),
            dict(p_edit=setter("min_weight", 0)), dict(p_edit=setter("step_trunc", 1e-7))]
    Kb, Pb = K.copy(), P.copy()
    Kb[0, 1] = -1.0
    Pb[0, 11] = INF
    bad += [dict(K_=Kb), dict(P_=Pb)]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
        assert np.all(depth == 7) and np.all(nrm == 7.0) and np.all(img == 7), kw
    assert call(null=("normals",)) == capi.DVO_OK and np.all(nrm == 7.0) and not np.all(img == 7) and not np.all(depth == 7)
    with pytest.raises(capi.DvoError) as ei:
        capi.tsdf_raycast_colour_host(c_volume(dict(vol, trunc=-1.0)), words, colours, tr.K4, P, rows, cols)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.tsdf_raycast_colour_host(c_volume(vol), words, colours[:-1], tr.K4, P, rows, cols)


def test_refusals_of_the_mesh():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol, words, colours = cr.mesh_case("volume0")
    xyz = np.full((8, 3), 7.0, np.float32)
    rgb = np.full((8, 3), 7, np.uint8)
    tri = np.full((8, 3), -9, np.int32)
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)

    def call(null=(), min_weight=1, vcap=8, tcap=8, vol_edit=None):
        v = c_volume(vol)
        if vol_edit:
            vol_edit(v)
        return lib.dvo_colour_mesh_host(None if "vol" in null else C.byref(v), None if "voxels" in null else capi._ptr(words),
                                        None if "colours" in null else capi._ptr(colours), min_weight, None if "xyz" in null else capi._ptr(xyz),
                                        None if "rgb" in null else capi._ptr(rgb), vcap, None if "tri" in null else capi._ptr(tri), tcap,
                                        None if "nv" in null else C.byref(nv), None if "nt" in null else C.byref(nt))

    bad = [dict(null=(k,)) for k in ("vol", "voxels", "colours", "xyz", "rgb", "tri", "nv", "nt")]
    bad += [dict(min_weight=0), dict(min_weight=-3), dict(vcap=-1), dict(tcap=-1), dict(null=("xyz", "rgb", "tri"), vcap=0), dict(null=("colours",), vcap=0, tcap=0)]
    bad += [dict(vol_edit=e) for e in bad_volumes()]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
        assert (nv.value, nt.value) == (-5, -6) and np.all(xyz == 7.0) and np.all(rgb == 7) and np.all(tri == -9), kw
    assert call(null=("xyz", "rgb", "tri"), vcap=0, tcap=0) == capi.DVO_OK and (nv.value, nt.value) == (1333, 2420)
    assert call(null=("xyz", "rgb"), vcap=0) == capi.DVO_OK and np.all(xyz == 7.0) and np.all(rgb == 7) and not np.all(tri == -9)
    with pytest.raises(capi.DvoError) as ei:
        capi.tsdf_mesh_colour_host(c_volume(dict(vol, trunc=0.0)), words, colours)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.tsdf_mesh_colour_host(c_volume(vol), words, colours[:-1])


def test_handle_calls_without_a_handle():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)
    assert lib.dvo_colour_enable(None) == capi.DVO_ERR_INVALID
    assert lib.dvo_colour_integrate(None, None, 0, None, None, 0, None, 0, 0, 0, None, None, 0) == capi.DVO_ERR_INVALID
    assert lib.dvo_colour_get_words(None, 0, None) == capi.DVO_ERR_INVALID and lib.dvo_colour_set_words(None, 0, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_colour_raycast_views(None, None, 0, None, 0, 0, 0, None, None, None, None, None, 0, 0) == capi.DVO_ERR_INVALID
    assert lib.dvo_colour_mesh_extract(None, 0, 1, None, None, 0, None, 0, C.byref(nv), C.byref(nt), 0) == capi.DVO_ERR_INVALID
    assert (nv.value, nt.value) == (-5, -6)


# ---- 7: the symbols ----

def test_symbols_headers_and_launches():
    from rgbd_odometry_amd import capi
    full = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", full, flags=re.S)
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    assert sorted(n for n in capi.C_ABI_SYMBOLS if n.startswith("dvo_colour_")) == sorted(NEW_SYMBOLS)
    csrc = lambda f: open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", f)).read()
    own, launch = csrc("dvo_tsdf_colour.h"), csrc("dvo_tsdf_launch.h")
    for header in ("dvo_tsdf_map.h", "dvo_tsdf_raycast.h", "dvo_tsdf_mesh.h"):
        assert '#include "%s"' % header in own
    assert '#include "dvo_tsdf_colour.h"' in launch
    # the colour launches issue what the constants say
    for fn, hip, want in (("launch_tsdf_integrate_colour", "dvo_tsdf_map.hip", capi.DVO_TSDF_INTEGRATE_LAUNCHES),
                          ("launch_tsdf_raycast_colour", "dvo_tsdf_raycast.hip", capi.DVO_RAYCAST_LAUNCHES),
                          ("launch_tsdf_mesh_colour", "dvo_tsdf_mesh.hip", capi.DVO_MESH_LAUNCHES)):
        body = csrc(hip).split("int %s(" % fn)[1].split("\n}\n")[0]
        assert body.count("hipLaunchKernelGGL(") == want, fn
    # no atomics, no environment switch and no float in the definition
    code = re.sub(r"/\*.*?\*/", " ", own, flags=re.S)
    assert "atomic" not in code and "getenv" not in code
    # colour is no longer out of scope in the fusion and the mesh sections; the new section follows the mesh section
    fusion = full.split("---- depth fusion:")[1].split("#ifndef DVO_TSDF_TYPES_DEFINED_")[0]
    meshes = full.split("---- the surface as a triangle mesh:")[1].split("#define DVO_MESH_LAUNCHES")[0]
    for section in (fusion, meshes):
        assert "OUT OF SCOPE" in section and "colour" not in section.split("OUT OF SCOPE")[1]
    assert full.index("---- the surface as a triangle mesh:") < full.index("---- colour in the map:") < full.index("---- the legacy photometric")


# ---- 8: the PLY writer ----

def test_save_ply(tmp_path):
    from rgbd_odometry_amd import capi
    v, t, rgb = host_mesh("volume0", 1)
    plain, again, coloured = tmp_path / "plain.ply", tmp_path / "again.ply", tmp_path / "coloured.ply"
    capi.save_ply(str(plain), v, t)
    capi.save_ply(str(again), v, t, colours=None)
    capi.save_ply(str(coloured), v, t, rgb)
    assert plain.read_bytes() == again.read_bytes()
    raw = plain.read_bytes()
    assert b"red" not in raw[:raw.index(b"end_header\n")] and len(raw) == raw.index(b"end_header\n") + 11 + 12 * len(v) + 13 * len(t)
    raw = coloured.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0" and header[-1] == "end_header"
    rest = [line for line in header[2:-1] if not line.startswith("comment")]
    assert rest == ["element vertex %d" % len(v), "property float x", "property float y", "property float z", "property uchar red",
                    "property uchar green", "property uchar blue", "element face %d" % len(t), "property list uchar int vertex_indices"]
    rec = np.frombuffer(raw[end:end + 15 * len(v)], dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
    assert same_bits(np.ascontiguousarray(rec["p"]), v) and same_bits(np.ascontiguousarray(rec["c"]), rgb)
    faces = np.frombuffer(raw[end + 15 * len(v):], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert len(faces) == len(t) and np.all(faces["n"] == 3) and np.array_equal(faces["i"], t)
    with pytest.raises(ValueError):
        capi.save_ply(str(coloured), v, t, rgb[:-1])


# ---- 9: the definition's own code under sanitizers, and the C++ mirror ----

def fnv1a(*blocks):
    """the 64-bit FNV-1a of the blocks' bytes, as the programs compute it"""
    h = 0xCBF29CE484222325
    data = np.frombuffer(b"".join(np.ascontiguousarray(b).tobytes() for b in blocks), np.uint8)
    for byte in data.tolist():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


#: (volume, image format, min_weight): the small volumes, whose bytes the checksum in Python can walk
PROGRAM_CASES = [(0, "bgr8", 1), (0, "mono8", 2), (2, "rgb8", 1), (3, "bgr8", 1)]
_expected = {}


def expected(vi, fmt, mw):
    """what the programs print, from the library's host functions; computed once"""
    from rgbd_odometry_amd import capi
    if (vi, fmt, mw) not in _expected:
        vol = tr.VOLUMES[vi]
        idx, imgs, poses = frames_of(vi)
        cols = [cr.images("random", fmt)[i] for i in idx]
        w, c = capi.tsdf_integrate_colour_host(c_volume(vol), None, None, imgs, cols, tr.K4, poses, image_format=fmt)
        v, t, rgb = capi.tsdf_mesh_colour_host(c_volume(vol), w, c, mw)
        d, n, img = capi.tsdf_raycast_colour_host(c_volume(vol), w, c, tr.K4, poses, tr.ROWS, tr.COLS, fmt="u16", image_format=fmt, normals=True)
        _expected[(vi, fmt, mw)] = dict(words="%016x" % fnv1a(w), colours="%016x" % fnv1a(c), vertices=str(len(v)), triangles=str(len(t)),
                                        mesh="%016x" % fnv1a(v, rgb, t), views="%016x" % fnv1a(d, n, img))
    return _expected[(vi, fmt, mw)]


def program_args(d, vi, fmt, mw, vol=None):
    idx, imgs, poses = frames_of(vi)
    cols = [cr.images("random", fmt)[i] for i in idx]
    paths = {k: str(d / ("%s_%d_%s.bin" % (k, vi, fmt))) for k in ("volume", "depth", "image", "poses")}
    open(paths["volume"], "wb").write(bytes(c_volume(vol or tr.VOLUMES[vi])))
    np.stack(imgs).tofile(paths["depth"])
    np.stack(cols).tofile(paths["image"])
    np.ascontiguousarray(poses).tofile(paths["poses"])
    return [paths["volume"], paths["depth"], paths["image"], paths["poses"], str(len(idx)), str(tr.ROWS), str(tr.COLS), str(cr.FORMATS[fmt]), str(mw)] + \
           [repr(float(k)) for k in tr.K4]


def parse(stdout):
    return dict(line.split(" ", 1) for line in stdout.splitlines() if " " in line)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_colour")
    exe = str(d / "tsdf_colour_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tsdf_colour_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/tsdf_colour_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


@pytest.mark.parametrize("vi,fmt,mw", PROGRAM_CASES)
def test_definition_under_sanitizers(host_program, vi, fmt, mw):
    """the same code the library compiles, with every buffer allocated to its exact size: clean under -fsanitize=address,undefined, and
    words, colour words, mesh and views have the library's bytes"""
    d, exe = host_program
    run = subprocess.run([exe] + program_args(d, vi, fmt, mw), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = parse(run.stdout)
    assert got == expected(vi, fmt, mw)


def test_program_refuses_what_the_definition_refuses(host_program):
    d, exe = host_program
    for vol, fmt_code, mw in ((dict(tr.VOLUMES[2], trunc=0.0), None, 1), (dict(tr.VOLUMES[2], voxel_size=float("nan")), None, 1), (None, "3", 1),
                              (None, None, 0)):
        args = program_args(d, 2, "rgb8", mw, vol=vol)
        if fmt_code:
            args[7] = fmt_code
        run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert run.returncode == 3 and run.stdout.splitlines()[-1] == "refused", run.stdout + run.stderr


def test_cpp_mirror(tmp_path):
    """include/dvo_amd.hpp's colour functions and the colour methods of TsdfVolumes: tests/host/tsdf_colour_hpp_main.cpp compiles with
    plain g++ and every warning on and links against the library; the host functions give the library's bytes on every small case, and
    on two cases TsdfVolumes is asked too: the same bytes where there is a device, a loud refusal where there is none"""
    import torch
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "tsdf_colour_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tsdf_colour_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    DEVICE_CASES = {(0, "mono8", 2), (2, "rgb8", 1)}
    for vi, fmt, mw in PROGRAM_CASES:
        on_device = (vi, fmt, mw) in DEVICE_CASES                     # every process that asks for the device initialises it: a few are enough
        run = subprocess.run([exe] + program_args(tmp_path, vi, fmt, mw) + (["device"] if on_device else []), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        got = parse(run.stdout)
        device = got.pop("device", None)
        assert got == expected(vi, fmt, mw), (vi, fmt, mw)
        if on_device and torch.cuda.is_available():
            assert device == "equal 1", (vi, fmt, mw, device)
        elif on_device:
            assert device.startswith("none") and "no CPU fallback" in device
    bad = program_args(tmp_path, 2, "rgb8", 1, vol=dict(tr.VOLUMES[2], trunc=-1.0))
    run = subprocess.run([exe] + bad, capture_output=True, text=True, timeout=120)
    assert run.returncode == 3 and run.stdout.splitlines()[-1] == "refused"
