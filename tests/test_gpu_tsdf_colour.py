"""Colour in the map on the device (include/dvo_amd.h, "colour in the map"): dvo_colour_integrate, dvo_colour_raycast_views and
dvo_colour_mesh_extract against the host definitions, which tests/test_tsdf_colour_cpu.py pins to the numpy restatement.  One handle
whose pools are exactly the sum of the four volumes of tests/tsdf_map_reference.py, set in order: a read or write past one volume lands
in its neighbour and shows; volumes 2 and 3 (5 x 3 x 2 and 1 x 1 x 1) make every 16-byte group a shared one.  SPHERE and TORUS
(83 x 81 x 79: 260 tiles) sit in a handle of their own.  All comparisons are byte equality; every test runs the definition's ordinary
inputs only."""
import ctypes as C

import numpy as np
import pytest

import tsdf_colour_reference as cr
import tsdf_map_reference as tr
import tsdf_mesh_reference as mr
import tsdf_raycast_reference as rr

pytestmark = pytest.mark.gpu
IMAGE_FORMATS = ["bgr8", "rgb8", "mono8"]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def new_handle(colour=True, volumes=tr.VOLUMES):
    """the volumes, cleared, in pools that are exactly their sum"""
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(len(volumes), sum(tr.voxels_of(v) for v in volumes))
    if colour:
        h.enable_colour()
    for i, vol in enumerate(volumes):
        h.set_volume(i, c_volume(vol))
    return h


_host = {}


def host_fused(kind, fmt, depth):
    """[(words, colours)] of the four volumes by the host definition; computed once"""
    from rgbd_odometry_amd import capi
    key = (kind, fmt, depth)
    if key not in _host:
        imgs, poses = tr.frame_list(depth)
        cols = cr.images(kind, fmt)
        out = []
        for vi, vol in enumerate(tr.VOLUMES):
            idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
            out.append(capi.tsdf_integrate_colour_host(c_volume(vol), None, None, [imgs[i] for i in idx], [cols[i] for i in idx], tr.K4, poses[idx],
                                                       image_format=fmt))
        _host[key] = out
    return _host[key]


def check_state(h, want, tag):
    for vi, (w, c) in enumerate(want):
        assert same_bits(h.voxels(vi), w), (tag, vi, int((h.voxels(vi) != w).sum()))
        assert same_bits(h.get_colours(vi), c), (tag, vi, int((h.get_colours(vi) != c).sum()))


def fill(h, kind="random", fmt="bgr8"):
    """the host definition's state into the handle"""
    for vi, (w, c) in enumerate(host_fused(kind, fmt, "u16")):
        h.set_voxels(vi, w)
        h.set_colours(vi, c)


@pytest.fixture(scope="module")
def handle():
    h = new_handle()
    yield h
    h.close()


# ---- 1: fusion ----

@pytest.mark.parametrize("depth", ["u16", "f32"])
@pytest.mark.parametrize("fmt", IMAGE_FORMATS)
def test_fusion_equals_the_host_definition(handle, fmt, depth):
    """all seven frames in one call; one call per frame; the list reversed by volume; host images and device images"""
    import torch
    from rgbd_odometry_amd import capi
    imgs, poses = tr.frame_list(depth)
    kind = "random" if depth == "u16" else "gradient"
    cols = cr.images(kind, fmt)
    want = host_fused(kind, fmt, depth)
    order = sorted(range(7), key=lambda i: (-tr.FRAME_VOLUMES[i], i))             # volumes 3, 2, 1, 0; each volume's frames in list order

    def clear():
        for vi in range(4):
            handle.clear(vi)

    clear()
    handle.integrate_colour(tr.FRAME_VOLUMES, imgs, cols, tr.K4, poses, image_format=fmt)
    assert handle.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1)
    check_state(handle, want, "one call")
    clear()
    for i in range(7):
        handle.integrate_colour([tr.FRAME_VOLUMES[i]], [imgs[i]], [cols[i]], tr.K4, poses[i:i + 1], image_format=fmt)
    check_state(handle, want, "one call per frame")
    clear()
    handle.integrate_colour([tr.FRAME_VOLUMES[i] for i in order], [imgs[i] for i in order], [cols[i] for i in order], tr.K4, poses[order], image_format=fmt)
    check_state(handle, want, "reversed by volume")
    clear()
    d_dev = [torch.from_numpy(d.view(np.int16) if d.dtype == np.uint16 else d).cuda() for d in imgs]
    c_dev = [torch.from_numpy(c).cuda() for c in cols]
    torch.cuda.synchronize()
    handle.integrate_colour(tr.FRAME_VOLUMES, d_dev, c_dev, tr.K4, poses, image_format=fmt, device=True)
    assert handle.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1)
    check_state(handle, want, "device images")


def host_colour_after(state, imgs, cols, fmt, K, poses):
    """the host definition: the seven frames on top of `state` ([(words, colours)] per volume, None: cleared)"""
    from rgbd_odometry_amd import capi
    out = []
    for vi, vol in enumerate(tr.VOLUMES):
        idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
        w, c = (None, None) if state is None else state[vi]
        out.append(capi.tsdf_integrate_colour_host(c_volume(vol), w, c, [imgs[i] for i in idx], [cols[i] for i in idx], K, poses[idx], image_format=fmt))
    return out


@pytest.mark.parametrize("fmt", IMAGE_FORMATS)
def test_fusion_at_37_x_53(handle, fmt):
    """an odd image size: 3922 or 7844 bytes of depth, 1961 or 5883 of image, none a multiple of 16 -- every staged image after the
    first starts at a padded offset, and the colour images start behind seven padded depth images.  Host images and device images"""
    import torch
    rows, cols = tr.ODD_SIZE
    depth = "f32" if fmt == "rgb8" else "u16"
    imgs, poses = tr.frame_list(depth, tr.ODD_SIZE)
    cols8 = cr.images("random", fmt, tr.ODD_SIZE)
    K = tr.k4_for(rows, cols)
    assert imgs[0].nbytes % 16 and cols8[0].nbytes % 16
    want = host_colour_after(None, imgs, cols8, fmt, K, poses)
    assert all(int((cr.colour_wc(c) > 0).sum()) >= least for (w, c), least in zip(want, (200, 2000, 5, 1)))
    for vi in range(4):
        handle.clear(vi)
    handle.integrate_colour(tr.FRAME_VOLUMES, imgs, cols8, K, poses, image_format=fmt)
    check_state(handle, want, "host images")
    for vi in range(4):
        handle.clear(vi)
    d_dev = [torch.from_numpy(d.view(np.int16) if d.dtype == np.uint16 else d).cuda() for d in imgs]
    c_dev = [torch.from_numpy(c).cuda() for c in cols8]
    torch.cuda.synchronize()
    handle.integrate_colour(tr.FRAME_VOLUMES, d_dev, c_dev, K, poses, image_format=fmt, device=True)
    check_state(handle, want, "device images")
    assert all(t.cpu().numpy().tobytes() == a.tobytes() for t, a in zip(d_dev + c_dev, imgs + cols8))


def test_image_sizes_on_one_handle():
    """a 24 x 32 call, a 37 x 53 call -- the staging buffer grows --, a 24 x 32 call in other formats -- it is reused: the words and
    the colour words of the host definition applied in the same order"""
    state = None
    h = new_handle()
    try:
        for size, depth, fmt in (((tr.ROWS, tr.COLS), "u16", "bgr8"), (tr.ODD_SIZE, "u16", "mono8"), ((tr.ROWS, tr.COLS), "f32", "rgb8")):
            imgs, poses = tr.frame_list(depth, size)
            cols8 = cr.images("gradient", fmt, size)
            K = tr.k4_for(*size)
            state = host_colour_after(state, imgs, cols8, fmt, K, poses)
            h.integrate_colour(tr.FRAME_VOLUMES, imgs, cols8, K, poses, image_format=fmt)
            check_state(h, state, (size, depth, fmt))
    finally:
        h.close()


# ---- 2: rounding and limits ----

def test_rounding_and_limits():
    from rgbd_odometry_amd import capi
    n = tr.voxels_of(tr.EDGE_VOLUME)
    guard_w, guard_c = np.full(5, 0x00030007, np.uint32), np.full(5, 0x0001000200030004, np.uint64)
    h = new_handle(volumes=[tr.volume((5, 1, 1), 0.1, (50.0, 0.0, 0.0), 0.1), tr.EDGE_VOLUME, tr.volume((5, 1, 1), 0.1, (60.0, 0.0, 0.0), 0.1)])
    try:
        def on_device(vol, words, colours, depths, images, fmt, K, poses, **params):
            h.set_volume(1, c_volume(vol))                                          # the same voxel count: it keeps its place
            for g in (0, 2):
                h.set_voxels(g, guard_w)
                h.set_colours(g, guard_c)
            h.set_voxels(1, words)
            h.set_colours(1, colours)
            h.integrate_colour([1] * len(depths), depths, images, K, poses, image_format=fmt, params=capi.DvoTsdfParams.default(**params))
            for g in (0, 2):
                assert same_bits(h.voxels(g), guard_w) and same_bits(h.get_colours(g), guard_c)
            return h.voxels(1), h.get_colours(1)

        cr.check_rounding_and_limits(on_device)
    finally:
        h.close()
    assert n == 27


# ---- 3: what touches the colour words and what does not ----

def test_plain_calls_and_clears(handle):
    imgs, poses = tr.frame_list("u16")
    fill(handle)
    want = host_fused("random", "bgr8", "u16")
    handle.integrate(tr.FRAME_VOLUMES, imgs, tr.K4, poses)                           # depth only: colour words untouched
    for vi, (w, c) in enumerate(want):
        assert same_bits(handle.get_colours(vi), c) and not same_bits(handle.voxels(vi), w), vi
    handle.set_voxels(1, want[1][0])
    assert same_bits(handle.get_colours(1), want[1][1])
    fill(handle)
    handle.clear(1)
    assert not handle.voxels(1).any() and not handle.get_colours(1).any()
    for vi in (0, 2, 3):
        assert same_bits(handle.voxels(vi), want[vi][0]) and same_bits(handle.get_colours(vi), want[vi][1]), vi
    fill(handle)
    handle.set_volume(2, c_volume(tr.VOLUMES[2]))
    assert not handle.voxels(2).any() and not handle.get_colours(2).any()
    for vi in (0, 1, 3):
        assert same_bits(handle.voxels(vi), want[vi][0]) and same_bits(handle.get_colours(vi), want[vi][1]), vi


# ---- 4: ray cast ----

def host_views(volumes, poses, rows, cols, dfmt, ifmt, state):
    from rgbd_odometry_amd import capi
    out = []
    for v, pose in zip(volumes, poses):
        d, n, img = capi.tsdf_raycast_colour_host(c_volume(tr.VOLUMES[v]), state[v][0], state[v][1], rr.k4_for(rows, cols), pose[None], rows, cols,
                                                  fmt=dfmt, image_format=ifmt, normals=True)
        out.append((d[0], n[0], img[0]))
    return out


@pytest.mark.parametrize("ifmt", IMAGE_FORMATS)
def test_ray_cast_equals_the_host_definition(handle, ifmt):
    """all views in one call, one call per view, device and host outputs, both depth formats, and 17 x 19 with partial 16 x 16 tiles"""
    from rgbd_odometry_amd import capi
    fill(handle)
    state = host_fused("random", "bgr8", "u16")
    volumes = [0, 1, 1, 0, 2, 3, 1]
    poses = np.stack([tr.POSES[0], tr.POSES[1], tr.POSES[4], tr.POSES[5], tr.POSES[3], tr.POSES[6], rr.extra_views(tr.VOLUMES[1])[3][1]])
    for (rows, cols), dfmt in (((tr.ROWS, tr.COLS), "u16"), ((17, 19), "f32")):
        want = host_views(volumes, poses, rows, cols, dfmt, ifmt, state)
        K = rr.k4_for(rows, cols)
        d, n, img = handle.raycast(volumes, K, poses, rows, cols, fmt=dfmt, normals=True, image_format=ifmt)
        assert handle.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
        pd, pn = handle.raycast(volumes, K, poses, rows, cols, fmt=dfmt, normals=True)
        assert same_bits(d, pd) and same_bits(n, pn)
        for k, (wd, wn, wi) in enumerate(want):
            assert same_bits(img[k], wi), (k, int((img[k] != wi).sum()))
            assert same_bits(d[k], wd) and same_bits(n[k], wn), k
            d1, i1 = handle.raycast(volumes[k:k + 1], K, poses[k:k + 1], rows, cols, fmt=dfmt, image_format=ifmt)
            assert same_bits(d1[0], wd) and same_bits(i1[0], wi), k
        td, tn, ti = handle.raycast(volumes, K, poses, rows, cols, fmt=dfmt, normals=True, image_format=ifmt, device=True)
        assert handle.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
        td = td.cpu().numpy()
        assert same_bits(td.view(np.uint16) if dfmt == "u16" else td, d) and same_bits(tn.cpu().numpy(), n) and same_bits(ti.cpu().numpy(), img)
    assert sum(int((w[2] != 0).sum()) for w in want) > 0


# ---- 5: mesh ----

_mesh = {}


def host_mesh(name, min_weight):
    from rgbd_odometry_amd import capi
    if (name, min_weight) not in _mesh:
        vol, words, colours = cr.mesh_case(name)
        _mesh[(name, min_weight)] = capi.tsdf_mesh_colour_host(c_volume(vol), words, colours, min_weight)
    return _mesh[(name, min_weight)]


def check_mesh(h, volume, name, min_weight, device=False):
    from rgbd_odometry_amd import capi
    v, t, rgb = h.extract_mesh(volume, min_weight, device=device, colours=True)
    assert h.stats() == (capi.DVO_MESH_LAUNCHES, 1)
    if device:
        v, t, rgb = v.cpu().numpy(), t.cpu().numpy(), rgb.cpu().numpy()
    hv, ht, hrgb = host_mesh(name, min_weight)
    assert len(v) == len(hv) and len(t) == len(ht), (name, min_weight, len(v), len(hv), len(t), len(ht))
    assert same_bits(rgb, hrgb), (name, min_weight, int((rgb != hrgb).any(axis=1).sum()))
    assert same_bits(v, hv) and same_bits(t, ht), (name, min_weight)
    pv, pt = h.extract_mesh(volume, min_weight)
    assert same_bits(pv, hv) and same_bits(pt, ht), (name, min_weight)


@pytest.mark.parametrize("min_weight", [1, 2])
def test_mesh_equals_the_host_definition(handle, min_weight):
    """the four fused volumes, then volume 1 with random words and random colour words in the same layout"""
    fill(handle)
    for i in range(4):
        check_mesh(handle, i, "volume%d" % i, min_weight, device=(i == 1))
    vol, words, colours = cr.mesh_case("random1")
    handle.set_voxels(1, words)
    handle.set_colours(1, colours)
    check_mesh(handle, 1, "random1", min_weight)
    check_mesh(handle, 1, "random1", min_weight, device=True)
    check_mesh(handle, 0, "volume0", min_weight)
    check_mesh(handle, 2, "volume2", min_weight)


@pytest.fixture(scope="module")
def analytic():
    """volume 0: volume 1's fused state; volumes 1 and 2: SPHERE and TORUS; the pools are exactly their sum"""
    h = new_handle(volumes=[tr.VOLUMES[1], mr.ANALYTIC_VOLUME, mr.ANALYTIC_VOLUME])
    for i, name in enumerate(("volume1", "SPHERE", "TORUS")):
        vol, words, colours = cr.mesh_case(name)
        h.set_voxels(i, words)
        h.set_colours(i, colours)
    yield h
    h.close()


def test_closed_surfaces(analytic):
    check_mesh(analytic, 1, "SPHERE", 1)
    check_mesh(analytic, 2, "TORUS", 1, device=True)
    check_mesh(analytic, 0, "volume1", 1)


def test_mesh_capacities(handle, analytic):
    """zero, exact and one short, host and device outputs: the written prefix is the full result's, nothing beyond it is touched"""
    import torch
    from rgbd_odometry_amd import capi
    fill(handle)
    guard = 3
    for h, volume, name in ((handle, 0, "volume0"), (handle, 2, "volume2"), (analytic, 1, "SPHERE")):
        v, t, rgb = host_mesh(name, 1)
        nv, nt = len(v), len(t)
        for vcap, tcap in [(0, 0), (nv, nt), (max(nv - 1, 0), max(nt - 1, 0)), (nv, max(nt - 1, 0)), (max(nv - 1, 0), nt)]:
            xyz = np.full((vcap + guard, 3), -7.5, np.float32)
            col = np.full((vcap + guard, 3), 0xA5, np.uint8)
            tri = np.full((tcap + guard, 3), -77, np.int32)
            gv, gt = C.c_longlong(-5), C.c_longlong(-6)
            rc = h.lib.dvo_colour_mesh_extract(h._h, volume, 1, capi._ptr(xyz) if vcap else None, capi._ptr(col) if vcap else None, vcap,
                                               capi._ptr(tri) if tcap else None, tcap, C.byref(gv), C.byref(gt), 0)
            assert rc == capi.DVO_OK and (gv.value, gt.value) == (nv, nt), (name, vcap, tcap)
            kv, kt = min(vcap, nv), min(tcap, nt)
            assert same_bits(xyz[:kv], v[:kv]) and same_bits(col[:kv], rgb[:kv]) and same_bits(tri[:kt], t[:kt]), (name, vcap, tcap)
            assert np.all(xyz[kv:] == -7.5) and np.all(col[kv:] == 0xA5) and np.all(tri[kt:] == -77), (name, vcap, tcap)
        # device outputs one short, with guards behind them
        vcap, tcap = max(nv - 1, 0), max(nt - 1, 0)
        if vcap and tcap:
            xyz = torch.full((vcap + guard, 3), -7.5, dtype=torch.float32, device="cuda")
            col = torch.full((vcap + guard, 3), 0xA5, dtype=torch.uint8, device="cuda")
            tri = torch.full((tcap + guard, 3), -77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            gv, gt = C.c_longlong(-5), C.c_longlong(-6)
            rc = h.lib.dvo_colour_mesh_extract(h._h, volume, 1, int(xyz.data_ptr()), int(col.data_ptr()), vcap, int(tri.data_ptr()), tcap, C.byref(gv),
                                               C.byref(gt), capi.DVO_UPLOAD_DEVICE)
            assert rc == capi.DVO_OK and (gv.value, gt.value) == (nv, nt)
            xyz, col, tri = xyz.cpu().numpy(), col.cpu().numpy(), tri.cpu().numpy()
            assert same_bits(xyz[:vcap], v[:vcap]) and same_bits(col[:vcap], rgb[:vcap]) and same_bits(tri[:tcap], t[:tcap]), name
            assert np.all(xyz[vcap:] == -7.5) and np.all(col[vcap:] == 0xA5) and np.all(tri[tcap:] == -77), name


# ---- 6: without enable_colour; refusals ----

def test_colour_calls_need_the_colour_pool():
    from rgbd_odometry_amd import capi
    imgs, poses = tr.frame_list("u16")
    cols = cr.images("random", "bgr8")
    h = new_handle(colour=False)
    try:
        state = host_fused("random", "bgr8", "u16")
        for vi in range(4):
            h.set_voxels(vi, state[vi][0])
        calls = [lambda: h.integrate_colour(tr.FRAME_VOLUMES, imgs, cols, tr.K4, poses),
                 lambda: h.get_colours(0),
                 lambda: h.set_colours(0, state[0][1]),
                 lambda: h.raycast([0], tr.K4, poses[:1], tr.ROWS, tr.COLS, image_format="bgr8"),
                 lambda: h.extract_mesh(0, colours=True)]
        for call in calls:
            with pytest.raises(capi.DvoError) as ei:
                call()
            assert ei.value.code == capi.DVO_ERR_STATE and "dvo_colour_enable" in str(ei.value)
        for vi in range(4):
            assert same_bits(h.voxels(vi), state[vi][0])
        # the uncoloured calls do what they did
        v, t = h.extract_mesh(0)
        assert same_bits(v, host_mesh("volume0", 1)[0]) and same_bits(t, host_mesh("volume0", 1)[1])
        # enabling is idempotent and leaves the words alone; the colour words start at zero
        h.enable_colour()
        h.enable_colour()
        for vi in range(4):
            assert same_bits(h.voxels(vi), state[vi][0]) and not h.get_colours(vi).any()
    finally:
        h.close()


def test_refusals_change_nothing(handle):
    from rgbd_odometry_amd import capi
    fill(handle)
    state = host_fused("random", "bgr8", "u16")
    imgs, poses = tr.frame_list("u16")
    cols = cr.images("random", "bgr8")
    lib, p = handle.lib, capi.DvoTsdfParams.default()
    K = np.ascontiguousarray(np.tile(np.array(tr.K4), (7, 1)))
    v = (C.c_int * 7)(*tr.FRAME_VOLUMES)
    dp = (C.c_void_p * 7)(*[d.ctypes.data for d in imgs])
    ip = (C.c_void_p * 7)(*[c.ctypes.data for c in cols])
    ip_null = (C.c_void_p * 7)(*[c.ctypes.data for c in cols[:6]], None)

    def integrate(count=7, volumes=v, depth=dp, image=ip, ifmt=capi.DVO_CAM_BGR8, flags=0):
        return lib.dvo_colour_integrate(handle._h, C.byref(p), count, volumes, depth, capi.DVO_DEPTH_U16, image, ifmt, tr.ROWS, tr.COLS, capi._ptr(K),
                                        capi._ptr(poses), flags)

    assert integrate(image=None) == capi.DVO_ERR_INVALID
    assert integrate(image=ip_null) == capi.DVO_ERR_INVALID
    assert integrate(ifmt=3) == capi.DVO_ERR_INVALID and integrate(ifmt=-1) == capi.DVO_ERR_INVALID
    assert integrate(depth=None) == capi.DVO_ERR_INVALID and integrate(count=0) == capi.DVO_ERR_INVALID and integrate(flags=7) == capi.DVO_ERR_INVALID
    assert integrate(volumes=(C.c_int * 7)(0, 1, 0, 2, 1, 0, 4)) == capi.DVO_ERR_INVALID
    assert lib.dvo_colour_get_words(handle._h, 0, None) == capi.DVO_ERR_INVALID and lib.dvo_colour_set_words(handle._h, 9, None) == capi.DVO_ERR_INVALID
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)
    xyz = np.full((4, 3), 7.0, np.float32)
    assert lib.dvo_colour_mesh_extract(handle._h, 0, 1, capi._ptr(xyz), None, 4, None, 0, C.byref(nv), C.byref(nt), 0) == capi.DVO_ERR_INVALID
    assert (nv.value, nt.value) == (-5, -6) and np.all(xyz == 7.0)
    rp = capi.DvoRaycastParams.default()
    depth = np.full((1, tr.ROWS, tr.COLS), 7, np.uint16)
    one = (C.c_void_p * 1)(depth.ctypes.data)
    for image_out, ifmt in ((None, capi.DVO_CAM_BGR8), ((C.c_void_p * 1)(None), capi.DVO_CAM_BGR8), (one, 5)):
        rc = lib.dvo_colour_raycast_views(handle._h, C.byref(rp), 1, (C.c_int * 1)(0), capi.DVO_DEPTH_U16, tr.ROWS, tr.COLS, capi._ptr(K), capi._ptr(poses),
                                          one, None, image_out, ifmt, 0)
        assert rc == capi.DVO_ERR_INVALID and np.all(depth == 7)
    check_state(handle, state, "after refusals")
