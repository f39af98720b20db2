"""The triangle mesh of fused volumes on the device (include/dvo_amd.h, "the surface as a triangle mesh"): dvo_mesh_extract against the
host definition (dvo_mesh_host), which tests/test_tsdf_mesh_cpu.py pins to the numpy restatement.  One handle whose pool is exactly the
sum of the four volumes of tests/tsdf_map_reference.py, set in order: a read past one volume lands in the next one's words and shows.
SPHERE and TORUS (83 x 81 x 79: 260 tiles, so every thread of the scan has more than one) sit in a handle of their own.  All
comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import tsdf_map_reference as tr
import tsdf_mesh_reference as mr
import tsdf_raycast_reference as rr

pytestmark = pytest.mark.gpu
TILE = 2048                                   # voxels of one workgroup's walk (kExtractTile)


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_host = {}


def host_mesh(name, min_weight):
    """the host definition's mesh of a case of tests/tsdf_mesh_reference.py; computed once, read-only"""
    from rgbd_odometry_amd import capi
    if (name, min_weight) not in _host:
        vol, words = mr.case(name)
        v, t = capi.tsdf_mesh_host(c_volume(vol), words, min_weight)
        v.setflags(write=False)
        t.setflags(write=False)
        _host[(name, min_weight)] = (v, t)
    return _host[(name, min_weight)]


def new_handle(random1=False):
    """the four fused volumes in a pool that is exactly their sum (random1: volume 1 holds the random words instead)"""
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(len(tr.VOLUMES), sum(tr.voxels_of(v) for v in tr.VOLUMES))
    for i, vol in enumerate(tr.VOLUMES):
        h.set_volume(i, c_volume(vol))
        h.set_voxels(i, mr.case("random1" if random1 and i == 1 else "volume%d" % i)[1])
    return h


@pytest.fixture(scope="module")
def fused():
    h = new_handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def analytic():
    """volume 0: volume 1's fused words; volumes 1 and 2: SPHERE and TORUS; the pool is exactly their sum"""
    from rgbd_odometry_amd import capi
    n = tr.voxels_of(mr.ANALYTIC_VOLUME)
    h = capi.DvoTsdfVolumes(3, tr.voxels_of(tr.VOLUMES[1]) + 2 * n)
    h.set_volume(0, c_volume(tr.VOLUMES[1]))
    h.set_voxels(0, mr.case("volume1")[1])
    for i, name in ((1, "SPHERE"), (2, "TORUS")):
        h.set_volume(i, c_volume(mr.ANALYTIC_VOLUME))
        h.set_voxels(i, mr.case(name)[1])
    yield h
    h.close()


def check(h, volume, name, min_weight, device=False):
    v, t = h.extract_mesh(volume, min_weight, device=device)
    if device:
        v, t = v.cpu().numpy(), t.cpu().numpy()
    hv, ht = host_mesh(name, min_weight)
    assert len(v) == len(hv) and len(t) == len(ht), (name, min_weight, len(v), len(hv), len(t), len(ht))
    assert same_bits(v, hv), (name, min_weight, int((v.view(np.uint32) != hv.view(np.uint32)).any(axis=1).sum()))
    assert same_bits(t, ht), (name, min_weight, int((t != ht).any(axis=1).sum()))


def raw_call(h, volume, min_weight, vcap, tcap, flags=0, guard=3, null=()):
    """dvo_mesh_extract into host buffers of vcap and tcap entries followed by `guard` entries of guard values: (rc, xyz, tri, nv, nt)"""
    from rgbd_odometry_amd import capi
    xyz = np.full((vcap + guard, 3), -7.5, np.float32)
    tri = np.full((tcap + guard, 3), -77, np.int32)
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)
    rc = h.lib.dvo_mesh_extract(h._h, volume, min_weight, capi._ptr(xyz) if vcap and "xyz" not in null else None, vcap,
                                capi._ptr(tri) if tcap and "tri" not in null else None, tcap, None if "nv" in null else C.byref(nv),
                                None if "nt" in null else C.byref(nt), flags)
    return rc, xyz, tri, nv.value, nt.value


@pytest.mark.parametrize("min_weight", [1, 2])
def test_device_equals_the_host_definition(fused, min_weight):
    """the four fused volumes, then volume 1 with random words in a handle of the same layout"""
    for i in range(len(tr.VOLUMES)):
        check(fused, i, "volume%d" % i, min_weight)
    h = new_handle(random1=True)
    try:
        check(h, 1, "random1", min_weight)
        check(h, 0, "volume0", min_weight)
        check(h, 2, "volume2", min_weight)
    finally:
        h.close()


@pytest.mark.parametrize("volume,name", [(1, "SPHERE"), (2, "TORUS")])
def test_closed_surfaces(analytic, volume, name):
    check(analytic, volume, name, 1)


def interesting_capacities(name, min_weight):
    """zero, exact, one short, short on one side only, a vertex capacity that ends inside a tile's vertices and a triangle capacity that
    ends inside a cell's triangles"""
    v, t = host_mesh(name, min_weight)
    nv, nt = len(v), len(t)
    cell = mr.reference(name, min_weight)[3]
    inside = np.flatnonzero(cell[1:] == cell[:-1]) + 1                # a capacity k with triangles k - 1 and k of one cell
    assert len(inside) > 0
    mid_cell = int(inside[len(inside) // 2])
    # vertices are in voxel order: the tile of the vertex in the middle also holds its neighbour unless a tile boundary falls there;
    # a capacity of 1 ends inside the first tile that has a vertex whenever that tile has two
    caps = [(0, 0), (nv, nt), (nv - 1, nt - 1), (nv - 1, nt), (nv, nt - 1), (nv // 2 + 1, nt), (1, nt), (nv, mid_cell), (nv // 3, mid_cell),
            (0, nt), (nv, 0), (nv + 2, nt + 2)]
    return nv, nt, caps


@pytest.mark.parametrize("name,volume,min_weight", [("volume1", 1, 1), ("volume0", 0, 2), ("SPHERE", 1, 1)])
def test_capacities(fused, analytic, name, volume, min_weight):
    from rgbd_odometry_amd import capi
    h = analytic if name == "SPHERE" else fused
    v, t = host_mesh(name, min_weight)
    nv, nt, caps = interesting_capacities(name, min_weight)
    for vcap, tcap in caps:
        rc, xyz, tri, gv, gt = raw_call(h, volume, min_weight, vcap, tcap)
        assert rc == capi.DVO_OK and (gv, gt) == (nv, nt), (vcap, tcap, gv, gt)
        kv, kt = min(vcap, nv), min(tcap, nt)
        assert same_bits(xyz[:kv], v[:kv]) and same_bits(tri[:kt], t[:kt]), (vcap, tcap)
        assert np.all(xyz[kv:] == -7.5) and np.all(tri[kt:] == -77), (vcap, tcap)
        assert h.stats() == (capi.DVO_MESH_LAUNCHES, 1)


def test_device_buffers(fused, analytic):
    """DVO_UPLOAD_DEVICE: torch tensors written in place equal the host-buffer outputs; short device buffers keep their guard values"""
    import torch
    from rgbd_odometry_amd import capi
    for i in range(len(tr.VOLUMES)):
        check(fused, i, "volume%d" % i, 1, device=True)
    check(analytic, 1, "SPHERE", 1, device=True)
    assert analytic.stats() == (capi.DVO_MESH_LAUNCHES, 1)
    v, t = host_mesh("SPHERE", 1)
    nv, nt, caps = interesting_capacities("SPHERE", 1)
    for vcap, tcap in caps[2:9]:
        xyz = torch.full((vcap + 3, 3), -7.5, dtype=torch.float32, device="cuda")
        tri = torch.full((tcap + 3, 3), -77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gv, gt = C.c_longlong(-5), C.c_longlong(-6)
        rc = analytic.lib.dvo_mesh_extract(analytic._h, 1, 1, int(xyz.data_ptr()), vcap, int(tri.data_ptr()), tcap, C.byref(gv), C.byref(gt),
                                           capi.DVO_UPLOAD_DEVICE)
        assert rc == capi.DVO_OK and (gv.value, gt.value) == (nv, nt)
        xyz, tri = xyz.cpu().numpy(), tri.cpu().numpy()
        kv, kt = min(vcap, nv), min(tcap, nt)
        assert same_bits(xyz[:kv], v[:kv]) and same_bits(tri[:kt], t[:kt]), (vcap, tcap)
        assert np.all(xyz[kv:] == -7.5) and np.all(tri[kt:] == -77), (vcap, tcap)


def test_scratch_is_reused_after_growing():
    """a fresh handle: the scratch is allocated for a tiny volume, grows twice, and is reused by smaller volumes afterwards; meshing twice
    in a row gives the same bytes"""
    h = new_handle()
    try:
        for i in (2, 0, 1, 0, 2, 3, 1, 1):
            check(h, i, "volume%d" % i, 1)
        check(h, 1, "volume1", 2)
        check(h, 1, "volume1", 1)
    finally:
        h.close()


def test_volume_1_before_and_after_a_larger_volume(analytic):
    check(analytic, 0, "volume1", 1)
    check(analytic, 1, "SPHERE", 1)
    check(analytic, 0, "volume1", 1)
    check(analytic, 2, "TORUS", 1)
    check(analytic, 0, "volume1", 2)


def test_after_points_and_raycast_on_the_same_handle(fused):
    from rgbd_odometry_amd import capi
    vol, words = mr.case("volume1")
    pts, n = fused.points(1)
    assert n > 0 and same_bits(pts, capi.tsdf_extract_host(c_volume(vol), words, 1)[0])
    check(fused, 1, "volume1", 1)
    rows, cols = rr.SIZES[0]
    depth = fused.raycast([1, 0], tr.K4, np.stack([tr.POSES[0], tr.POSES[1]]), rows, cols, normals=False)
    assert depth.any()
    check(fused, 1, "volume1", 1)
    check(fused, 0, "volume0", 2)
    pts2, n2 = fused.points(1)
    assert n2 == n and same_bits(pts, pts2)


def test_words_are_unchanged_and_stats(fused):
    from rgbd_odometry_amd import capi
    before = [fused.voxels(i) for i in range(len(tr.VOLUMES))]
    for i in range(len(tr.VOLUMES)):
        fused.extract_mesh(i, 1)
        assert fused.stats() == (capi.DVO_MESH_LAUNCHES, 1)
        fused.extract_mesh(i, 2, device=True)
        assert fused.stats() == (capi.DVO_MESH_LAUNCHES, 1)
    for i, w in enumerate(before):
        assert same_bits(fused.voxels(i), w) and same_bits(w, mr.case("volume%d" % i)[1])


def test_refusals_write_nothing():
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(3, tr.voxels_of(tr.VOLUMES[0]) + 8)
    try:
        h.set_volume(0, c_volume(tr.VOLUMES[0]))
        h.set_voxels(0, mr.case("volume0")[1])
        nv, nt = len(host_mesh("volume0", 1)[0]), len(host_mesh("volume0", 1)[1])

        def refused(code, volume=0, min_weight=1, vcap=8, tcap=8, flags=0, null=()):
            rc, xyz, tri, gv, gt = raw_call(h, volume, min_weight, vcap, tcap, flags, null=null)
            assert rc == code, (rc, code, volume, min_weight, vcap, tcap, flags, null)
            assert (gv, gt) == (-5, -6) and np.all(xyz == -7.5) and np.all(tri == -77)
            assert h.lib.dvo_tsdf_last_error(h._h)

        for kw in (dict(min_weight=0), dict(min_weight=-1), dict(vcap=-1), dict(tcap=-1), dict(null=("xyz",)), dict(null=("tri",)), dict(null=("nv",)),
                   dict(null=("nt",)), dict(flags=2), dict(flags=-1), dict(flags=capi.DVO_UPLOAD_DEVICE | 2), dict(volume=-1), dict(volume=3)):
            refused(capi.DVO_ERR_INVALID, **kw)
        refused(capi.DVO_ERR_STATE, volume=1)
        refused(capi.DVO_ERR_STATE, volume=2, flags=capi.DVO_UPLOAD_DEVICE)
        with pytest.raises(capi.DvoError) as ei:
            h.extract_mesh(1)
        assert ei.value.code == capi.DVO_ERR_STATE
        # the handle still works, and either buffer may be NULL with capacity 0
        rc, xyz, tri, gv, gt = raw_call(h, 0, 1, 0, nt)
        assert rc == capi.DVO_OK and (gv, gt) == (nv, nt) and same_bits(tri[:nt], host_mesh("volume0", 1)[1])
        assert same_bits(h.voxels(0), mr.case("volume0")[1])
    finally:
        h.close()
