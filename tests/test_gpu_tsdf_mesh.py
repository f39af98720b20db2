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


def corner_words():
    """a sphere in SPHERE's volume around its last voxel, so the last rows -- the tiles from the 256th on -- hold crossings; weights 1 .. 3"""
    x, y, z = mr._analytic_grid()
    dx, dy, dz = x - x.max() - 0.0031, y - y.max() + 0.0017, z - z.max() - 0.0023
    q = np.clip(np.rint((np.sqrt(dx * dx + dy * dy + dz * dz) - 0.1953) / mr.ANALYTIC_VOLUME["trunc"] * 32767.0), -32767, 32767).astype(np.int64)
    return tr.make_words(q.reshape(-1), np.random.RandomState(77).randint(1, 4, size=q.size))


POINT_CASES = [("SPHERE", 1), ("TORUS", 1), ("CORNER", 1), ("CORNER", 2)]     # SPHERE's and TORUS's words all have weight 1


@pytest.mark.parametrize("name,min_weight", POINT_CASES)
def test_points_through_the_multi_count_scan(name, min_weight):
    """Point extraction over 260 tiles: threads 0 .. 129 of the scan own two counts each, the rest none (the point tests of
    test_gpu_tsdf_map.py stop at 60 tiles).  Byte-equal to the host definition at capacities zero, exact, one short and one that ends
    behind the first point of the tiles from the 256th on.  SPHERE and TORUS end well inside the volume (|z| <= 0.3 and 0.09 of 0.39):
    their last tile with a crossing is below the 256th, so CORNER, a sphere around the last voxel, stands beside them."""
    from rgbd_odometry_amd import capi
    vol = mr.ANALYTIC_VOLUME
    words = corner_words() if name == "CORNER" else mr.case(name)[1]
    want, n_want = capi.tsdf_extract_host(c_volume(vol), words, min_weight)
    # the conditions on the inputs, from the host definition alone: a voxel's crossings are with neighbours of higher index, so what
    # is left with the first 256 tiles emptied is exactly what the tiles from the 256th on hold
    assert tr.voxels_of(vol) > 256 * TILE and n_want > 0
    tail = words.copy()
    tail[:256 * TILE] = 0
    n_tail = capi.tsdf_extract_host(c_volume(vol), tail, min_weight)[1]
    odd = words.copy()
    odd[:258 * TILE].reshape(258, TILE)[0::2] = 0                   # tiles 0, 2, .. emptied: what remains is owned by an odd tile
    assert capi.tsdf_extract_host(c_volume(vol), odd, min_weight)[1] > 0, "no thread's second count is positive"
    caps = [0, n_want, n_want - 1]
    if name == "CORNER":
        assert n_tail >= 2, "no crossing in a tile with index >= 256"
        from_tile = [n_tail]                                            # the points of the tiles from 256 + k on, by the same emptying
        for t in range(257, (tr.voxels_of(vol) + TILE - 1) // TILE + 1):
            tail[:min(t * TILE, len(tail))] = 0
            from_tile.append(capi.tsdf_extract_host(c_volume(vol), tail, min_weight)[1])
        first = next(a - b for a, b in zip(from_tile, from_tile[1:]) if a > b)
        assert from_tile[-1] == 0 and first >= 2, "the first tile from the 256th on with a point has no second one"
        caps.append(n_want - n_tail + 1)                                # ends behind the first point of that tile, inside it
    with capi.DvoTsdfVolumes(1, tr.voxels_of(vol)) as h:
        h.set_volume(0, c_volume(vol))
        h.set_voxels(0, words)
        got, n = h.points(0, min_weight)
        assert h.stats() == (capi.DVO_TSDF_EXTRACT_LAUNCHES, 1)
        assert n == n_want and same_bits(got, want), (name, min_weight, n, n_want)
        for capacity in caps:
            buf = np.full((n_want + 8, 3), -777.25, np.float32)
            n = C.c_longlong(0)
            assert h.lib.dvo_tsdf_extract_points(h._h, 0, min_weight, capi._ptr(buf), capacity, C.byref(n)) == capi.DVO_OK
            assert n.value == n_want and same_bits(buf[:capacity], want[:capacity]) and np.all(buf[capacity:] == -777.25), (name, capacity)
        assert same_bits(h.voxels(0), words)


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

        def refused(code, msg, volume=0, min_weight=1, vcap=8, tcap=8, flags=0, null=()):
            rc, xyz, tri, gv, gt = raw_call(h, volume, min_weight, vcap, tcap, flags, null=null)
            assert rc == code, (rc, code, volume, min_weight, vcap, tcap, flags, null)
            assert (gv, gt) == (-5, -6) and np.all(xyz == -7.5) and np.all(tri == -77)
            assert h.lib.dvo_tsdf_last_error(h._h).decode() == msg

        # the words of every refusal, as dvo_capi_tsdf.cpp has had them since the mesh was added
        ARGS = "min_weight < 1, a negative capacity, a NULL buffer with capacity > 0, or a NULL count"
        FLAGS, RANGE, NEVER = "unknown flags (0 or DVO_UPLOAD_DEVICE)", "volume outside [0, max_volumes)", "volume %d was never set (dvo_tsdf_set_volume)"
        for kw in (dict(min_weight=0), dict(min_weight=-1), dict(vcap=-1), dict(tcap=-1), dict(null=("xyz",)), dict(null=("tri",)), dict(null=("nv",)),
                   dict(null=("nt",)), dict(min_weight=0, flags=2, volume=3)):
            refused(capi.DVO_ERR_INVALID, ARGS, **kw)
        for kw in (dict(flags=2), dict(flags=-1), dict(flags=capi.DVO_UPLOAD_DEVICE | 2), dict(flags=2, volume=3)):
            refused(capi.DVO_ERR_INVALID, FLAGS, **kw)
        for kw in (dict(volume=-1), dict(volume=3)):
            refused(capi.DVO_ERR_INVALID, RANGE, **kw)
        refused(capi.DVO_ERR_STATE, NEVER % 1, volume=1)
        refused(capi.DVO_ERR_STATE, NEVER % 2, volume=2, flags=capi.DVO_UPLOAD_DEVICE)
        with pytest.raises(capi.DvoError) as ei:
            h.extract_mesh(1)
        assert ei.value.code == capi.DVO_ERR_STATE and str(ei.value) == "dvo error 4: " + NEVER % 1
        # the handle still works, and either buffer may be NULL with capacity 0
        rc, xyz, tri, gv, gt = raw_call(h, 0, 1, 0, nt)
        assert rc == capi.DVO_OK and (gv, gt) == (nv, nt) and same_bits(tri[:nt], host_mesh("volume0", 1)[1])
        assert same_bits(h.voxels(0), mr.case("volume0")[1])
    finally:
        h.close()
