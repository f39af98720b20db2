"""Distance fields on the device (include/dvo_amd.h, "distance fields"): dvo_esdf_update, dvo_esdf_get_words, dvo_esdf_get_distances and
dvo_esdf_query against the host definition, which tests/test_esdf_cpu.py pins to the numpy restatement (tests/esdf_reference.py).  Every
handle's pools are exactly the sum of its volumes, set in order: a read or write past one volume lands in its neighbour and shows.  All
comparisons are byte equality."""
import os
import re

import numpy as np
import pytest

import esdf_reference as er
import tsdf_map_reference as tr
import tsdf_mesh_reference as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def params(mw=1, sites=0):
    from rgbd_odometry_amd import capi
    return capi.DvoEsdfParams.default(min_weight=mw, sites=sites)


def host_words(vol, tw, mw=1, sites=0):
    from rgbd_odometry_amd import capi
    return capi.esdf_host(c_volume(vol), tw, params(mw, sites))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def new_handle(volumes, esdf=True, words=None):
    """the volumes in pools that are exactly their sum, cleared or holding `words`"""
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(len(volumes), sum(tr.voxels_of(v) for v in volumes))
    if esdf:
        h.enable_esdf()
    for i, vol in enumerate(volumes):
        h.set_volume(i, c_volume(vol))
        if words is not None:
            h.set_voxels(i, words[i])
    return h


def launch_constants():
    text = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_esdf_launch.h")).read()
    return (int(re.search(r"constexpr int kEsdfRowChunk = (\d+);", text).group(1)), int(re.search(r"constexpr int kEsdfColumnTile = (\d+);", text).group(1)))


def state_error(call):
    from rgbd_odometry_amd import capi
    with pytest.raises(capi.DvoError) as ei:
        call()
    return ei.value.code == capi.DVO_ERR_STATE


# ---- 1, 3: the words on every case ----

def check_cases_on_one_handle(case_list, combos=er.COMBOS):
    """all cases in one handle, one update of all volumes per (min_weight, sites); every volume byte-equal to the host definition"""
    from rgbd_odometry_amd import capi
    h = new_handle([v for _, v, _ in case_list], words=[w for _, _, w in case_list])
    try:
        for mw, sites in combos:
            h.update_esdf(list(range(len(case_list))), params(mw, sites))
            assert h.stats() == (capi.DVO_ESDF_UPDATE_LAUNCHES, 1)
            for i, (name, vol, tw) in enumerate(case_list):
                got, want = h.esdf_words(i), host_words(vol, tw, mw, sites)
                assert same_bits(got, want), "%s (min_weight %d, sites %d): %d words differ" % (name, mw, sites, int((got != want).sum()))
    finally:
        h.close()


def test_words_of_fused_and_random_volumes():
    check_cases_on_one_handle(er.fused_cases())


def test_words_of_constructed_volumes():
    cases = er.constructed_cases()
    check_cases_on_one_handle(cases)
    name, vol, tw = next(c for c in cases if c[0] == "corner")
    w = host_words(vol, tw, 1, 1).reshape(65, 67, 70)
    assert int(w[64, 66, 69] & er.NO_SITE) == 69 ** 2 + 66 ** 2 + 64 ** 2 and int(w[0, 0, 0]) == er.UNKNOWN


def test_shapes_around_the_tiling():
    B, C = launch_constants()
    cases = er.tiling_cases(B, C)
    assert sorted(v["dims"][0] for n, v, _ in cases if n.startswith("x")) == [B - 1, B, B + 1, 2 * B + 1]
    check_cases_on_one_handle(cases, combos=[(1, 0), (1, 1)])
    # the site's distance reaches the near end from another chunk or tile
    for name, vol, tw in cases:
        d2 = host_words(vol, tw) & er.NO_SITE
        assert d2[0] != er.NO_SITE and d2[0] >= (max(vol["dims"]) - 2) ** 2, name


# ---- 2: the packed pool ----

def test_packed_pool_any_batch_and_unlisted_volumes():
    from rgbd_odometry_amd import capi
    vols = tr.PACKED_VOLUMES
    rng = np.random.RandomState(21)
    words = [tr.random_pool_words(rng, tr.voxels_of(v)) for v in vols]
    want = [host_words(v, w, 1, 1) for v, w in zip(vols, words)]
    n = len(vols)
    got = {}
    for tag, calls in (("one call", [list(range(n))]), ("one per volume", [[i] for i in range(n)]), ("reversed", [list(range(n))[::-1]])):
        h = new_handle(vols, words=words)
        for listed in calls:
            h.update_esdf(listed, params(1, 1))
            assert h.stats() == (capi.DVO_ESDF_UPDATE_LAUNCHES, 1)
        got[tag] = [h.esdf_words(i) for i in range(n)]
        h.close()
        for i in range(n):
            assert same_bits(got[tag][i], want[i]), (tag, i)
    # a volume that is not listed: its words untouched, its flag as it was (current stays current, stale stays stale)
    h = new_handle(vols, words=words)
    h.update_esdf(list(range(n)), params(1, 1))
    h.set_voxels(5, words[5])                                       # volume 5 is stale now
    listed = [i for i in range(n) if i not in (1, 5, 18)]
    other = [tr.random_pool_words(rng, tr.voxels_of(v)) for v in vols]
    for i in listed:
        h.set_voxels(i, other[i])
    h.update_esdf(listed[::-1], params(1, 0))
    for i in range(n):
        if i == 5:
            assert state_error(lambda: h.esdf_words(5))
        elif i in (1, 18):
            assert same_bits(h.esdf_words(i), want[i]), i
        else:
            assert same_bits(h.esdf_words(i), host_words(vols[i], other[i], 1, 0)), i
    h.close()


# ---- 4: staleness, and fusion as without the feature ----

def test_staleness_in_sequence():
    from rgbd_odometry_amd import capi
    vol = tr.VOLUMES[0]
    imgs, poses = tr.frame_list("u16")
    h = new_handle([vol, tr.VOLUMES[2]])
    readers = (lambda: h.esdf_words(0), lambda: h.esdf_distances(0), lambda: h.esdf_query(0, np.zeros((1, 3))))
    assert all(state_error(r) for r in readers)                      # never updated
    h.update_esdf([0, 1])
    h.integrate([0], [imgs[0]], tr.K4, poses[:1])
    assert all(state_error(r) for r in readers)
    h.esdf_words(1)                                                  # the other volume's field stays current
    h.update_esdf([0])
    assert same_bits(h.esdf_words(0), host_words(vol, h.voxels(0)))
    for change in (lambda: h.clear(0), lambda: h.set_voxels(0, h.voxels(0)), lambda: h.set_volume(0, c_volume(vol))):
        change()
        assert all(state_error(r) for r in readers)
        h.update_esdf([0])
        h.esdf_words(0)
    # a volume listed twice, a bad parameter, a volume that was never set: refused, the flags as they were
    for bad in (lambda: h.update_esdf([0, 0]), lambda: h.update_esdf([0], params(0, 0)), lambda: h.update_esdf([0], params(1, 2)),
                lambda: h.update_esdf([]), lambda: h.update_esdf([2])):
        with pytest.raises(capi.DvoError) as ei:
            bad()
        assert ei.value.code == capi.DVO_ERR_INVALID
    h.esdf_words(0)
    h.close()
    plain = new_handle([vol], esdf=False)
    assert state_error(lambda: plain.update_esdf([0])) and state_error(lambda: plain.esdf_words(0))
    assert state_error(lambda: plain.esdf_distances(0)) and state_error(lambda: plain.esdf_query(0, np.zeros((1, 3))))
    plain.close()


def test_fusion_is_what_it_was_on_an_enabled_handle():
    """words after dvo_tsdf_integrate, points, ray cast and mesh of VOLUMES[0]: the same bytes, launches and synchronisations with and
    without the distance-field pool"""
    vol = tr.VOLUMES[0]
    imgs, poses = tr.frame_list("u16")
    idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == 0]
    out = []
    for esdf in (False, True):
        h = new_handle([vol], esdf=esdf)
        if esdf:
            h.update_esdf([0])
        res, st = [], []
        h.integrate([0] * len(idx), [imgs[i] for i in idx], tr.K4, poses[idx]); st.append(h.stats())
        res.append(h.voxels(0))
        res.extend(h.points(0)[:1]); st.append(h.stats())
        res.extend(h.raycast([0, 0], tr.K4, poses[idx][:2], tr.ROWS, tr.COLS, normals=True)); st.append(h.stats())
        res.extend(h.extract_mesh(0)); st.append(h.stats())
        out.append((res, st))
        h.close()
    assert out[0][1] == out[1][1]
    assert len(out[0][0]) == len(out[1][0]) == 6 and all(same_bits(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert len(out[0][0][1]) > 0 and len(out[0][0][5]) > 0


# ---- 5, 6, 7: distances, queries and their stats ----

@pytest.fixture(scope="module")
def sphere():
    """SPHERE behind a volume with unknown voxels and one without a site, fields current"""
    from rgbd_odometry_amd import capi
    vols = [tr.VOLUMES[2], mr.ANALYTIC_VOLUME, tr.VOLUMES[0], tr.volume((7, 5, 3), 0.05, (0, 0, 0.5), 0.15)]
    words = [mr.case("volume2")[1], mr.case("SPHERE")[1], mr.case("volume0")[1], tr.make_words(np.full(105, 50), np.ones(105, np.int64))]
    h = new_handle(vols, words=words)
    h.update_esdf([0, 1, 2, 3])
    ew = [host_words(v, w) for v, w in zip(vols, words)]
    for i in range(4):
        assert same_bits(h.esdf_words(i), ew[i])
    yield h, vols, ew
    h.close()


def test_get_distances(sphere):
    import torch
    from rgbd_odometry_amd import capi
    h, vols, ew = sphere
    for i, vol in enumerate(vols):
        nx, ny, nz = vol["dims"]
        want = capi.esdf_distances_host(c_volume(vol), ew[i])
        for iz0, n in ((0, nz), (nz // 2, 1), (nz - 1, 1)):
            sl = slice(iz0 * nx * ny, (iz0 + n) * nx * ny)
            assert same_bits(h.esdf_distances(i, iz0, n), want[sl]), (i, iz0, n)
            assert h.stats() == (1, 1)
            dev = h.esdf_distances(i, iz0, n, device=True)
            assert h.stats() == (1, 1)
            assert same_bits(dev.cpu().numpy(), want[sl]), (i, iz0, n)
    assert np.all(np.isinf(capi.esdf_distances_host(c_volume(vols[3]), ew[3])))
    # refused ranges write nothing: guard words around the output
    nx, ny, nz = vols[1]["dims"]
    lib, handle = h.lib, h._h
    guard = np.full(nx * ny + 64, -7.5, np.float32)
    dguard = torch.full((nx * ny + 64,), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for iz0, n in ((-1, 1), (0, 0), (nz, 1), (nz - 1, 2), (0, nz + 1), (2 ** 31 - 1, 2)):
        assert lib.dvo_esdf_get_distances(handle, 1, iz0, n, guard[32:].ctypes.data, 0) == capi.DVO_ERR_INVALID
        assert lib.dvo_esdf_get_distances(handle, 1, iz0, n, dguard[32:].data_ptr(), capi.DVO_UPLOAD_DEVICE) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_get_distances(handle, 1, 0, 1, guard[32:].ctypes.data, 3) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_get_distances(handle, 1, 0, 1, None, 0) == capi.DVO_ERR_INVALID
    assert np.all(guard == -7.5) and bool((dguard == -7.5).all())
    # one plane lands inside the guards
    assert lib.dvo_esdf_get_distances(handle, 1, 3, 1, guard[32:].ctypes.data, 0) == capi.DVO_OK
    assert np.all(guard[:32] == -7.5) and np.all(guard[32 + nx * ny:] == -7.5)
    assert same_bits(guard[32:32 + nx * ny], capi.esdf_distances_host(c_volume(vols[1]), ew[1])[3 * nx * ny:4 * nx * ny])


def test_query(sphere):
    import torch
    from rgbd_odometry_amd import capi
    h, vols, ew = sphere
    for i, vol in enumerate(vols):
        P = er.query_points(vol, ew[i])
        want = capi.esdf_query_host(c_volume(vol), ew[i], P)
        got = h.esdf_query(i, P)
        assert h.stats() == (1, 1)
        assert got.tobytes() == want.tobytes(), (i, int((got != want).sum()))
        dev = h.esdf_query(i, torch.from_numpy(P).cuda(), device=True)
        assert h.stats() == (1, 1)
        assert dev.cpu().numpy().tobytes() == want.tobytes(), i
    seen = set(int(s) for i in range(4) for s in capi.esdf_query_host(c_volume(vols[i]), ew[i], er.query_points(vols[i], ew[i]))["status"])
    assert seen == {er.FOUND, er.OUTSIDE, er.NO_DISTANCE}
    # count = 1, 63, 64, 65 and 4097
    vol, words = vols[1], ew[1]
    rng = np.random.RandomState(5)
    o, vs, dims = np.array(vol["origin"]), vol["voxel_size"], np.array(vol["dims"], np.float64)
    for count in (1, 63, 64, 65, 4097):
        P = o + vs * rng.uniform(-0.05, 1.05, size=(count, 3)) * (dims - 1.0)
        want = capi.esdf_query_host(c_volume(vol), words, P)
        assert h.esdf_query(1, P).tobytes() == want.tobytes(), count
        assert h.esdf_query(1, torch.from_numpy(P).cuda(), device=True).cpu().numpy().tobytes() == want.tobytes(), count
    # a point that is not finite in host memory: refused, nothing written
    bad = np.array([[0.0, 0.0, 0.0], [0.0, np.nan, 0.0]])
    out = np.full(2, 7, dtype=capi.ESDF_SAMPLE_DTYPE)
    keep = out.tobytes()
    assert h.lib.dvo_esdf_query(h._h, 1, 2, bad.ctypes.data, out.ctypes.data, 0) == capi.DVO_ERR_INVALID and out.tobytes() == keep
    assert h.lib.dvo_esdf_query(h._h, 1, 0, bad.ctypes.data, out.ctypes.data, 0) == capi.DVO_ERR_INVALID and out.tobytes() == keep


def test_stats_of_one_and_five_volumes():
    from rgbd_odometry_amd import capi
    cases = er.fused_cases()[:5]
    h = new_handle([v for _, v, _ in cases], words=[w for _, _, w in cases])
    h.update_esdf([3])
    assert h.stats() == (capi.DVO_ESDF_UPDATE_LAUNCHES, 1)
    h.update_esdf([4, 2, 0, 1, 3])
    assert h.stats() == (capi.DVO_ESDF_UPDATE_LAUNCHES, 1)
    for i, (name, vol, tw) in enumerate(cases):
        assert same_bits(h.esdf_words(i), host_words(vol, tw)), name
    h.close()


# ---- 8: the scratch block ----

def test_scratch_is_reused_after_growing():
    small, large = tr.VOLUMES[0], tr.VOLUMES[1]
    ws, wl = mr.case("volume0")[1], mr.case("volume1")[1]
    h = new_handle([small, large], words=[ws, wl])
    for listed in ([0], [1], [0], [1, 0]):
        h.update_esdf(listed, params(1, 1))
        assert same_bits(h.esdf_words(0), host_words(small, ws, 1, 1)), listed
        if 1 in listed:
            assert same_bits(h.esdf_words(1), host_words(large, wl, 1, 1)), listed
    h.close()
