"""Ray casting of fused volumes on the device (include/dvo_amd.h, "from the map back to depth"): dvo_raycast_views against the host
definition (dvo_raycast_host), which tests/test_tsdf_raycast_cpu.py pins to the numpy restatement.  One handle whose pool is exactly the
sum of the four volumes of tests/tsdf_map_reference.py, set in order: a read past one volume lands in the next one's words and shows as
a wrong pixel.  Images are 24 x 32 and 37 x 53 (no multiple of the 16 x 16 pixel tile of a workgroup: partial tiles on two borders, more
than one workgroup per view).  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import tsdf_map_reference as tr
import tsdf_raycast_reference as rr

pytestmark = pytest.mark.gpu
FORMATS = ["u16", "f32"]
COMBOS = [(rr.SIZES[0], s) for s in rr.SETTINGS] + [(rr.SIZES[1], rr.SETTINGS[0])]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_state = {}


def host_words():
    """the words of the four volumes after their frames, by the host definition (computed once)"""
    from rgbd_odometry_amd import capi
    if "words" not in _state:
        imgs, poses = tr.frame_list("u16")
        out = []
        for vi, vol in enumerate(tr.VOLUMES):
            idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
            w = capi.tsdf_integrate_host(c_volume(vol), None, [imgs[i] for i in idx], tr.K4, poses[idx])
            w.setflags(write=False)
            out.append(w)
        _state["words"] = out
    return _state["words"]


def view_table():
    """(volume index of each view, poses (n, 12)): every view of tests/tsdf_raycast_reference.py of every volume, volumes interleaved"""
    per = [rr.view_list(vol) for vol in tr.VOLUMES]
    vols, poses = [], []
    for k in range(len(per[0])):
        for vi in range(len(tr.VOLUMES)):
            vols.append(vi)
            poses.append(per[vi][k][1])
    return vols, np.stack(poses)


def host_images(words, size, setting, fmt):
    """the host definition's (depth, normals) of the view table, for the given words of the four volumes"""
    from rgbd_odometry_amd import capi
    vols, poses = view_table()
    rows, cols = size
    p = capi.DvoRaycastParams.default(**setting)
    depth = np.zeros((len(vols), rows, cols), np.uint16 if fmt == "u16" else np.float32)
    nrm = np.zeros((len(vols), rows, cols, 3), np.float32)
    for vi, vol in enumerate(tr.VOLUMES):
        idx = [i for i, v in enumerate(vols) if v == vi]
        d, n = capi.tsdf_raycast_host(c_volume(vol), words[vi], rr.k4_for(rows, cols), poses[idx], rows, cols, p, fmt, True)
        depth[idx], nrm[idx] = d, n
    return depth, nrm


def fused_host_images(size, setting, fmt):
    key = (size, tuple(sorted(setting.items())), fmt)
    if key not in _state:
        d, n = host_images(host_words(), size, setting, fmt)
        d.setflags(write=False)
        n.setflags(write=False)
        _state[key] = (d, n)
    return _state[key]


def new_handle(words=None, extra_volumes=0):
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(len(tr.VOLUMES) + extra_volumes, sum(tr.voxels_of(v) for v in tr.VOLUMES))
    for i, vol in enumerate(tr.VOLUMES):
        h.set_volume(i, c_volume(vol))
        h.set_voxels(i, (host_words() if words is None else words)[i])
    return h


@pytest.fixture(scope="module")
def fused():
    """a handle that holds the four fused volumes, for the tests that only read it"""
    h = new_handle()
    yield h
    h.close()


def all_voxels(h):
    return [h.voxels(i) for i in range(len(tr.VOLUMES))]


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_equals_the_host_definition(fused, fmt):
    """every view of every volume in one call per size and setting; then volume 1 with random words, put in through dvo_tsdf_set_voxels"""
    from rgbd_odometry_amd import capi
    vols, poses = view_table()
    for size, setting in COMBOS:
        rows, cols = size
        p = capi.DvoRaycastParams.default(**setting)
        want_d, want_n = fused_host_images(size, setting, fmt)
        depth, nrm = fused.raycast(vols, rr.k4_for(rows, cols), poses, rows, cols, p, fmt, normals=True)
        assert fused.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
        assert same_bits(depth, want_d), (size, setting, fmt, int((depth != want_d).sum()))
        assert same_bits(nrm, want_n), (size, setting, fmt)
        assert same_bits(fused.raycast(vols, rr.k4_for(rows, cols), poses, rows, cols, p, fmt), want_d)
        assert depth.any() and nrm.any()
    words = list(host_words())
    words[1] = rr.random_words(tr.VOLUMES[1])
    with new_handle(words) as h:
        for size, setting in COMBOS:
            rows, cols = size
            want_d, want_n = host_images(words, size, setting, fmt)
            depth, nrm = h.raycast(vols, rr.k4_for(rows, cols), poses, rows, cols, capi.DvoRaycastParams.default(**setting), fmt, normals=True)
            assert same_bits(depth, want_d) and same_bits(nrm, want_n), (size, setting, fmt)
            idx = [i for i, v in enumerate(vols) if v == 1]
            assert (depth[idx] > 0).sum() >= 100 and (depth[idx] == 0).sum() >= 100


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_independence(fused, fmt):
    """all views in one call, one call per view, a permuted list: the same bytes"""
    vols, poses = view_table()
    size = rr.SIZES[1]
    rows, cols = size
    K = rr.k4_for(rows, cols)
    want_d, want_n = fused_host_images(size, rr.SETTINGS[0], fmt)
    depth, nrm = fused.raycast(vols, K, poses, rows, cols, fmt=fmt, normals=True)
    assert same_bits(depth, want_d) and same_bits(nrm, want_n)
    for i in range(len(vols)):
        d, n = fused.raycast(vols[i:i + 1], K, poses[i:i + 1], rows, cols, fmt=fmt, normals=True)
        assert same_bits(d[0], want_d[i]) and same_bits(n[0], want_n[i]), i
    order = np.random.RandomState(4).permutation(len(vols))
    assert not np.array_equal(order, np.arange(len(vols)))
    d, n = fused.raycast([vols[i] for i in order], K, poses[order], rows, cols, fmt=fmt, normals=True)
    assert same_bits(d, want_d[order]) and same_bits(n, want_n[order])


@pytest.mark.parametrize("fmt", FORMATS)
def test_partial_tiles_and_device_outputs(fused, fmt):
    """37 x 53 images written in place (DVO_UPLOAD_DEVICE) into one canary-filled device buffer with a guard band in front of, between
    and behind the images: the images are the copied-back ones, the guard bands keep their canary"""
    import torch
    from rgbd_odometry_amd import capi
    vols, poses = view_table()
    n = len(vols)
    rows, cols = rr.SIZES[1]
    K = np.ascontiguousarray(np.broadcast_to(np.array(rr.k4_for(rows, cols)), (n, 4)))
    want_d, want_n = fused_host_images(rr.SIZES[1], rr.SETTINGS[0], fmt)
    guard, px = 64, rows * cols
    dt = torch.int16 if fmt == "u16" else torch.float32
    dbuf = torch.full((n, guard + px + guard), 0x5A5A if fmt == "u16" else -7.5, dtype=dt, device="cuda")
    nbuf = torch.full((n, guard + 3 * px + guard), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dp = (C.c_void_p * n)(*[dbuf[i].data_ptr() + guard * dbuf.element_size() for i in range(n)])
    npp = (C.c_void_p * n)(*[nbuf[i].data_ptr() + guard * 4 for i in range(n)])
    v = (C.c_int * n)(*vols)
    p = capi.DvoRaycastParams.default()
    code = capi.DVO_DEPTH_U16 if fmt == "u16" else capi.DVO_DEPTH_F32
    fused._chk(fused.lib.dvo_raycast_views(fused._h, C.byref(p), n, v, code, rows, cols, capi._ptr(K), capi._ptr(poses), dp, npp, capi.DVO_UPLOAD_DEVICE))
    assert fused.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
    d, nr = dbuf.cpu().numpy(), nbuf.cpu().numpy()
    if fmt == "u16":
        d = d.view(np.uint16)
    canary = 0x5A5A if fmt == "u16" else np.float32(-7.5)
    assert np.all(d[:, :guard] == canary) and np.all(d[:, guard + px:] == canary)
    assert np.all(nr[:, :guard] == -7.5) and np.all(nr[:, guard + 3 * px:] == -7.5)
    assert same_bits(d[:, guard:guard + px].reshape(n, rows, cols), want_d)
    assert same_bits(nr[:, guard:guard + 3 * px].reshape(n, rows, cols, 3), want_n)
    # the mirror's device path: torch tensors
    td, tn = fused.raycast(vols, K, poses, rows, cols, fmt=fmt, normals=True, device=True)
    got = td.cpu().numpy()
    assert td.is_cuda and same_bits(got.view(np.uint16) if fmt == "u16" else got, want_d) and same_bits(tn.cpu().numpy(), want_n)


@pytest.mark.parametrize("fmt", FORMATS)
def test_rendered_depth_into_fusion(fused, fmt):
    """a depth image rendered into device memory goes straight into dvo_tsdf_integrate(..., DVO_UPLOAD_DEVICE): the words are those of
    the host definition fed the host-rendered image"""
    from rgbd_odometry_amd import capi
    vol = tr.VOLUMES[1]
    rows, cols = rr.SIZES[0]
    poses = np.stack(tr.POSES[:3])
    rendered = fused.raycast([1, 1, 1], tr.K4, poses, rows, cols, fmt=fmt, device=True)
    host_rendered = capi.tsdf_raycast_host(c_volume(vol), host_words()[1], tr.K4, poses, rows, cols, None, fmt)
    want = capi.tsdf_integrate_host(c_volume(vol), None, list(host_rendered), tr.K4, poses)
    with capi.DvoTsdfVolumes(1, tr.voxels_of(vol)) as h:
        h.set_volume(0, c_volume(vol))
        h.integrate([0, 0, 0], [rendered[i] for i in range(3)], tr.K4, poses, device=True)
        got = h.voxels(0)
    assert want.any() and np.array_equal(got, want)


def test_stats_and_read_only(fused):
    from rgbd_odometry_amd import capi
    before = all_voxels(fused)
    assert all(np.array_equal(a, b) for a, b in zip(before, host_words()))
    vols, poses = view_table()
    rows, cols = rr.SIZES[0]
    fused.points(0, capacity=10)
    assert fused.stats() == (capi.DVO_TSDF_EXTRACT_LAUNCHES, 1)
    fused.raycast(vols[:1], tr.K4, poses[:1], rows, cols)
    assert fused.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1) == (1, 1)
    fused.raycast(vols, tr.K4, poses, rows, cols, fmt="f32", normals=True)
    assert fused.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
    fused.raycast(vols, tr.K4, poses, rows, cols, fmt="u16", device=True)
    assert fused.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
    assert all(np.array_equal(a, b) for a, b in zip(all_voxels(fused), before)), "a ray cast must change no word"


def test_refusals_change_nothing():
    from rgbd_odometry_amd import capi
    vols, poses = view_table()
    rows, cols = rr.SIZES[0]
    with new_handle(extra_volumes=1) as h:
        lib = h.lib
        before = all_voxels(h)
        depth = np.full((2, rows, cols), 0x5A5A, np.uint16)
        nrm = np.full((2, rows, cols, 3), -7.5, np.float32)
        dp = (C.c_void_p * 2)(depth[0].ctypes.data, depth[1].ctypes.data)
        npp = (C.c_void_p * 2)(nrm[0].ctypes.data, nrm[1].ctypes.data)
        half = (C.c_void_p * 2)(depth[0].ctypes.data, None)
        two = (C.c_int * 2)(0, 1)
        K = np.ascontiguousarray(np.broadcast_to(np.array(tr.K4), (2, 4)))
        P = np.ascontiguousarray(np.stack(tr.POSES[:2]))
        prm = capi.DvoRaycastParams.default()
        INV, STATE = capi.DVO_ERR_INVALID, capi.DVO_ERR_STATE

        def raw(p=prm, count=2, v=two, fmt=capi.DVO_DEPTH_U16, r=rows, c=cols, k=K, q=P, d=dp, n=npp, flags=0):
            return lib.dvo_raycast_views(h._h, None if p is None else C.byref(p), count, v, fmt, r, c, None if k is None else capi._ptr(k),
                                         None if q is None else capi._ptr(q), d, n, flags)

        def untouched():
            return np.all(depth == 0x5A5A) and np.all(nrm == -7.5) and all(np.array_equal(a, b) for a, b in zip(all_voxels(h), before))

        D = capi.DvoRaycastParams.default
        nan, inf = float("nan"), float("inf")
        # the words of every refusal, as dvo_capi_tsdf.cpp has had them since the ray cast was added
        PARAMS = "bad parameters (NULL, 0 < z_near < z_far, step_trunc in (0, 1], all finite, min_weight in [1, 65535])"
        COUNT, SHAPE, FLAGS = "count < 1 or a NULL argument", "rows or cols < 1, or an unknown depth format", "unknown flags (0 or DVO_UPLOAD_DEVICE)"
        LISTED, IMAGE = "a listed volume is outside [0, max_volumes)", "a NULL output image"
        VIEW = "view %d: a K4 or pose that is not finite, or fx / fy not positive"
        MARCH = "view %d: its march would have more than DVO_RAYCAST_MAX_STEPS samples"
        bad = [(PARAMS, dict(p=None)), (COUNT, dict(v=None)), (COUNT, dict(k=None)), (COUNT, dict(q=None)), (COUNT, dict(d=None)), (IMAGE, dict(d=half)),
               (IMAGE, dict(n=half)), (COUNT, dict(count=0)), (COUNT, dict(count=-2)), (SHAPE, dict(r=0)), (SHAPE, dict(c=0)), (SHAPE, dict(c=-5)),
               (SHAPE, dict(fmt=2)), (SHAPE, dict(fmt=-1)), (FLAGS, dict(flags=1)), (FLAGS, dict(flags=capi.DVO_UPLOAD_DEVICE | 1)), (FLAGS, dict(flags=-1)),
               (LISTED, dict(v=(C.c_int * 2)(0, 5))), (LISTED, dict(v=(C.c_int * 2)(-1, 0))),
               (COUNT, dict(count=0, r=0, flags=9)), (SHAPE, dict(r=0, flags=9)), (FLAGS, dict(flags=9, d=half))]      # the order of the checks
        bad += [(PARAMS, dict(p=D(**kw))) for kw in (dict(z_near=0.0), dict(z_near=9.0), dict(z_near=nan), dict(z_far=inf), dict(z_far=nan),
                                                      dict(step_trunc=0.0), dict(step_trunc=1.5), dict(step_trunc=nan), dict(min_weight=0),
                                                      dict(min_weight=65536))]
        bad.append((MARCH % 0, dict(p=D(step_trunc=1e-6))))
        for j in range(4):
            for value in (nan, inf):
                Kb = K.copy()
                Kb[1, j] = value
                bad.append((VIEW % 1, dict(k=Kb)))
        bad += [(VIEW % 1, dict(k=np.array([[30.0, 30.0, 15.5, 11.5], [0.0, 30.0, 15.5, 11.5]]))),
                (VIEW % 0, dict(k=np.array([[30.0, -1.0, 15.5, 11.5], [30.0, 30.0, 15.5, 11.5]])))]
        for j in (0, 8, 9, 11):
            Pb = P.copy()
            Pb[1, j] = nan
            bad.append((VIEW % 1, dict(q=Pb)))
        for msg, kw in bad:
            assert raw(**kw) == INV, kw
            assert lib.dvo_tsdf_last_error(h._h).decode() == msg, kw
            assert untouched(), kw
        for v in ((C.c_int * 2)(0, 4), (C.c_int * 2)(4, 4)):                                          # never set
            assert raw(v=v) == STATE and lib.dvo_tsdf_last_error(h._h).decode() == "volume 4 was never set (dvo_tsdf_set_volume)"
            assert untouched()
        assert raw(v=(C.c_int * 2)(4, 0), q=Pb) == INV and lib.dvo_tsdf_last_error(h._h).decode() == VIEW % 1      # every view before any "never set"
        with pytest.raises(capi.DvoError) as ei:
            h.raycast([4], tr.K4, poses[:1], rows, cols)
        assert ei.value.code == STATE and str(ei.value) == "dvo error 4: volume 4 was never set (dvo_tsdf_set_volume)"
        with pytest.raises(capi.DvoError) as ei:
            h.raycast([0], tr.K4, poses[:1], rows, cols, D(step_trunc=2.0))
        assert ei.value.code == INV and str(ei.value) == "dvo error 1: " + PARAMS
        assert untouched()
        # the handle still works
        assert raw() == capi.DVO_OK and h.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
        want = capi.tsdf_raycast_host(c_volume(tr.VOLUMES[0]), host_words()[0], tr.K4, P[:1], rows, cols, None, "u16", True)
        assert same_bits(depth[0], want[0][0]) and same_bits(nrm[0], want[1][0]) and depth[1].any()
        assert all(np.array_equal(a, b) for a, b in zip(all_voxels(h), before))


def test_clip_domain():
    """the views of rr.domain_views -- where clip(), which only the kernel's march uses, is nearest to cutting a sample off -- against
    the whole march of the host definition, depth and normals.  Every case has a volume of its own in one handle whose pool is exactly
    their sum; the cases that share parameters and a depth format go into one call"""
    from rgbd_odometry_amd import capi
    cases = rr.domain_views(0)
    rows, cols = rr.DOMAIN_SIZE
    groups = rr.domain_groups(cases)
    assert len(groups) <= 36
    hits = 0
    with capi.DvoTsdfVolumes(len(cases), sum(tr.voxels_of(c["vol"]) for c in cases)) as h:
        for i, c in enumerate(cases):
            h.set_volume(i, c_volume(c["vol"]))
            h.set_voxels(i, c["words"])
        for (z_near, z_far, step_trunc, min_weight, fmt), idx in sorted(groups.items()):
            p = capi.DvoRaycastParams.default(z_near=z_near, z_far=z_far, step_trunc=step_trunc, min_weight=min_weight)
            depth, nrm = h.raycast(idx, np.array([cases[i]["K4"] for i in idx]), np.stack([cases[i]["pose"] for i in idx]), rows, cols, p, fmt,
                                   normals=True)
            assert h.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
            for k, i in enumerate(idx):
                c = cases[i]
                want_d, want_n = capi.tsdf_raycast_host(c_volume(c["vol"]), c["words"], c["K4"], c["pose"][None], rows, cols, p, fmt, True)
                where = (i, c["category"], c["params"], fmt)
                assert same_bits(depth[k], want_d[0]), where + (int((depth[k] != want_d[0]).sum()),)
                assert same_bits(nrm[k], want_n[0]), where
                hits += int((want_d[0] != 0).sum())
        for i in (0, len(cases) // 2, len(cases) - 1):
            assert np.array_equal(h.voxels(i), cases[i]["words"])
    assert 100 * hits >= 15 * len(cases) * rows * cols
