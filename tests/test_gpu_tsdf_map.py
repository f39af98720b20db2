"""Depth fusion on the device (include/dvo_amd.h, "depth fusion"): dvo_tsdf_integrate and dvo_tsdf_extract_points against the host
definition (dvo_tsdf_integrate_host, dvo_tsdf_extract_host), which tests/test_tsdf_map_cpu.py pins to the numpy restatement.  One handle
whose pool is exactly the sum of the four volumes of tests/tsdf_map_reference.py, set in order: an overrun of one volume lands in the next
one's bytes and is seen.  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import tsdf_map_reference as tr

pytestmark = pytest.mark.gpu
FORMATS = ["u16", "f32"]
LIST = tr.FRAME_VOLUMES                          # [0, 1, 0, 2, 1, 0, 3]
PERMUTED = [6, 3, 1, 0, 4, 2, 5]                 # another order of the frames that keeps each volume's own order


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_points(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def new_handle(extra_volumes=0):
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(len(tr.VOLUMES) + extra_volumes, sum(tr.voxels_of(v) for v in tr.VOLUMES))
    for i, vol in enumerate(tr.VOLUMES):
        h.set_volume(i, c_volume(vol))
    return h


def all_voxels(h):
    return [h.voxels(i) for i in range(len(tr.VOLUMES))]


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


_host = {}


def host_state(fmt):
    """the host definition applied in list order: the words of every volume after the seven frames (computed once per format)"""
    from rgbd_odometry_amd import capi
    if fmt not in _host:
        imgs, poses = tr.frame_list(fmt)
        state = []
        for vi, vol in enumerate(tr.VOLUMES):
            idx = [i for i, v in enumerate(LIST) if v == vi]
            w = capi.tsdf_integrate_host(c_volume(vol), None, [imgs[i] for i in idx], tr.K4, poses[idx])
            w.setflags(write=False)
            state.append(w)
        _host[fmt] = state
    return _host[fmt]


@pytest.fixture(scope="module")
def fused():
    """a handle that holds the seven 16-bit frames, for the tests that only read it"""
    h = new_handle()
    imgs, poses = tr.frame_list("u16")
    h.integrate(LIST, imgs, tr.K4, poses)
    yield h
    h.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_equals_the_host_definition(fmt):
    from rgbd_odometry_amd import capi
    imgs, poses = tr.frame_list(fmt)
    with new_handle() as h:
        assert all(not w.any() for w in all_voxels(h))
        h.integrate(LIST, imgs, tr.K4, poses)
        assert h.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1)
        got = all_voxels(h)
    for vi, (g, w) in enumerate(zip(got, host_state(fmt))):
        assert g.any() and np.array_equal(g, w), (vi, fmt, int((g != w).sum()))


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_independence(fmt):
    """one call of seven frames, seven calls of one frame, a call with the volumes permuted (each volume's own order kept), and the
    first again: the same bytes"""
    imgs, poses = tr.frame_list(fmt)
    assert all([LIST[i] for i in PERMUTED if LIST[i] == v] == [v] * LIST.count(v) and
               [i for i in PERMUTED if LIST[i] == v] == sorted(i for i in PERMUTED if LIST[i] == v) for v in set(LIST))
    states = []
    with new_handle() as h:
        h.integrate(LIST, imgs, tr.K4, poses)
        states.append(all_voxels(h))
    with new_handle() as h:
        for i in range(len(LIST)):
            h.integrate([LIST[i]], [imgs[i]], tr.K4, poses[i:i + 1])
        states.append(all_voxels(h))
    with new_handle() as h:
        h.integrate([LIST[i] for i in PERMUTED], [imgs[i] for i in PERMUTED], tr.K4, poses[PERMUTED])
        states.append(all_voxels(h))
        for i in range(len(tr.VOLUMES)):         # the same handle again, after a clear
            h.clear(i)
        h.integrate(LIST, imgs, tr.K4, poses)
        states.append(all_voxels(h))
    for s in states:
        assert same_state(s, host_state(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_resident_images(fmt):
    import torch
    imgs, poses = tr.frame_list(fmt)
    dev = [torch.from_numpy(i.view(np.int16) if fmt == "u16" else i).cuda().contiguous() for i in imgs]
    torch.cuda.synchronize()
    with new_handle() as h:
        h.integrate(LIST, dev, tr.K4, poses, device=True)
        assert same_state(all_voxels(h), host_state(fmt))


def host_after(state, volumes, imgs, K, poses):
    """the host definition: the listed frames on top of `state` (the words per volume, None: cleared), in list order"""
    from rgbd_odometry_amd import capi
    out = []
    for vi, vol in enumerate(tr.VOLUMES):
        idx = [i for i, v in enumerate(volumes) if v == vi]
        before = None if state is None else state[vi]
        out.append(capi.tsdf_integrate_host(c_volume(vol), before, [imgs[i] for i in idx], K, poses[idx]) if idx else
                   (np.zeros(tr.voxels_of(vol), np.uint32) if before is None else before))
    return out


def as_device(imgs):
    import torch
    dev = [torch.from_numpy(i.view(np.int16) if i.dtype == np.uint16 else i).cuda().contiguous() for i in imgs]
    torch.cuda.synchronize()
    return dev


@pytest.mark.parametrize("fmt", FORMATS)
def test_odd_image_size(fmt):
    """37 x 53: 3922 or 7844 bytes an image, no multiple of 16 -- every staged image after the first starts at a padded offset -- and
    a row pitch that is no power of two.  The seven frames in one call, host images and device images"""
    from rgbd_odometry_amd import capi
    rows, cols = tr.ODD_SIZE
    imgs, poses = tr.frame_list(fmt, tr.ODD_SIZE)
    assert imgs[0].nbytes % 16 and imgs[0].shape == tr.ODD_SIZE
    K = tr.k4_for(rows, cols)
    want = host_after(None, LIST, imgs, K, poses)
    assert all(tr.seen_and_negative(w)[0] >= least for w, least in zip(want, (1500, 20000, 20, 1))) and tr.seen_and_negative(want[0])[1] >= 500
    with new_handle() as h:
        h.integrate(LIST, imgs, K, poses)
        assert h.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1)
        got = all_voxels(h)
        assert same_state(got, want), [int((g != w).sum()) for g, w in zip(got, want)]
        for i in range(len(tr.VOLUMES)):
            h.clear(i)
        dev = as_device(imgs)
        h.integrate(LIST, dev, K, poses, device=True)
        got = all_voxels(h)
        assert same_state(got, want), [int((g != w).sum()) for g, w in zip(got, want)]
        assert all(d.cpu().numpy().tobytes() == i.tobytes() for d, i in zip(dev, imgs))


def test_vga_image_size():
    """480 x 640, three 16-bit frames into each of the volumes 0, 2 and 3: pixel indices beyond 65,535"""
    rows, cols = tr.VGA_SIZE
    frames, poses = tr.frame_list("u16", tr.VGA_SIZE)
    imgs, poses = [frames[f] for f in tr.VGA_FRAMES], poses[tr.VGA_FRAMES]
    K = tr.k4_for(rows, cols)
    want = host_after(None, tr.VGA_VOLUMES, imgs, K, poses)
    assert tr.seen_and_negative(want[0])[0] >= 1500 and tr.seen_and_negative(want[2])[0] >= 20 and want[3].any() and not want[1].any()
    with new_handle() as h:
        h.integrate(tr.VGA_VOLUMES, imgs, K, poses)
        got = all_voxels(h)
        assert same_state(got, want), [int((g != w).sum()) for g, w in zip(got, want)]
        for i in range(len(tr.VOLUMES)):
            h.clear(i)
        h.integrate(tr.VGA_VOLUMES, as_device(imgs), K, poses, device=True)
        assert same_state(all_voxels(h), want)


def test_image_sizes_on_one_handle():
    """a 24 x 32 call, a 37 x 53 call -- the staging buffer grows --, a 24 x 32 call in the other depth format -- it is reused: the
    words of the host definition applied in the same order"""
    state = None
    with new_handle() as h:
        for size, fmt in (((tr.ROWS, tr.COLS), "u16"), (tr.ODD_SIZE, "u16"), ((tr.ROWS, tr.COLS), "f32")):
            imgs, poses = tr.frame_list(fmt, size)
            K = tr.k4_for(*size)
            before = state
            state = host_after(state, LIST, imgs, K, poses)
            assert before is None or not any(np.array_equal(a, b) for a, b in zip(before[:3], state[:3]))
            h.integrate(LIST, imgs, K, poses)
            got = all_voxels(h)
            assert same_state(got, state), (size, fmt, [int((g != w).sum()) for g, w in zip(got, state)])


def test_crafted_states():
    """the rounding and limit cases of the CPU file, put in through dvo_tsdf_set_voxels"""
    from rgbd_odometry_amd import capi

    def device_integrate(vol, words, imgs, K, poses, **params):
        with capi.DvoTsdfVolumes(1, tr.voxels_of(vol)) as h:
            h.set_volume(0, c_volume(vol))
            h.set_voxels(0, words)
            h.integrate([0] * len(imgs), imgs, K, poses, capi.DvoTsdfParams.default(**params) if params else None)
            return h.voxels(0)

    tr.check_rounding_and_limits(device_integrate)


def test_extraction(fused):
    from rgbd_odometry_amd import capi
    before = all_voxels(fused)
    assert same_state(before, host_state("u16"))
    counts = []
    for vi, vol in enumerate(tr.VOLUMES):
        for min_weight in (1, 2):
            want, n_want = capi.tsdf_extract_host(c_volume(vol), host_state("u16")[vi], min_weight)
            got, n = fused.points(vi, min_weight)
            assert fused.stats() == (capi.DVO_TSDF_EXTRACT_LAUNCHES, 1)
            assert n == n_want and same_points(got, want), (vi, min_weight, n, n_want)
            counts.append(n)
    assert counts[0] >= 100 and counts[2] > 2048 // 3, counts          # more than one workgroup's tile holds crossings
    # a capacity below the count: exactly the first `capacity` points, the rest of a canary-filled buffer alone, the full count
    want, n_want = capi.tsdf_extract_host(c_volume(tr.VOLUMES[1]), host_state("u16")[1], 1)
    for capacity in (1, 100, n_want - 1):
        buf = np.full((n_want + 8, 3), -777.25, np.float32)
        n = C.c_longlong(0)
        assert fused.lib.dvo_tsdf_extract_points(fused._h, 1, 1, capi._ptr(buf), capacity, C.byref(n)) == capi.DVO_OK
        assert n.value == n_want and same_points(buf[:capacity], want[:capacity]) and np.all(buf[capacity:] == -777.25), capacity
    pts, n = fused.points(1, 1, capacity=0)
    assert n == n_want and len(pts) == 0
    assert same_state(all_voxels(fused), before), "extraction must change no word"
    with new_handle() as h:                      # cleared volumes give 0
        for vi in range(len(tr.VOLUMES)):
            assert h.points(vi)[1] == 0
        imgs, poses = tr.frame_list("u16")
        h.integrate(LIST, imgs, tr.K4, poses)
        h.clear(1)
        assert h.points(1)[1] == 0 and h.points(0)[1] == counts[0]


@pytest.mark.parametrize("fmt", FORMATS)
def test_degenerate_frames(fmt):
    """looking away, camera inside the volume, all holes, non-finite depth, u and v beyond 2^30: ordinary inputs of the definition"""
    from rgbd_odometry_amd import capi
    with new_handle() as h:
        imgs, poses = tr.frame_list(fmt)
        h.integrate(LIST, imgs, tr.K4, poses)
        ran = 0
        for name, img, pose in tr.degenerate_frames():
            if img.dtype == np.uint16 and fmt == "f32":
                img = tr.as_f32(img)
            elif img.dtype == np.float32 and fmt == "u16":
                continue
            for vi, vol in enumerate(tr.VOLUMES):
                want = capi.tsdf_integrate_host(c_volume(vol), host_state(fmt)[vi], [img], tr.K4, pose[None])
                h.set_voxels(vi, host_state(fmt)[vi])
                h.integrate([vi], [img], tr.K4, pose[None])
                assert np.array_equal(h.voxels(vi), want), (name, vi, fmt)
            ran += 1
        assert ran == (5 if fmt == "f32" else 4)


def test_counts():
    from rgbd_odometry_amd import capi
    imgs, poses = tr.frame_list("u16")
    with new_handle() as h:
        h.integrate([0], imgs[:1], tr.K4, poses[:1])
        assert h.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1) == (1, 1)
        h.integrate(LIST, imgs, tr.K4, poses)
        assert h.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1)
        h.points(0, capacity=10)
        assert h.stats() == (capi.DVO_TSDF_EXTRACT_LAUNCHES, 1) == (3, 1)


def test_refusals_change_nothing(fused):
    from rgbd_odometry_amd import capi
    lib = fused.lib
    imgs, poses = tr.frame_list("u16")
    before = all_voxels(fused)
    with capi.DvoTsdfVolumes(len(tr.VOLUMES) + 1, sum(tr.voxels_of(v) for v in tr.VOLUMES)) as h:
        for i, vol in enumerate(tr.VOLUMES):
            h.set_volume(i, c_volume(vol))
        h.integrate(LIST, imgs, tr.K4, poses)
        assert same_state(all_voxels(h), before)
        P = capi.DvoTsdfParams.default
        K, one = np.array(tr.K4), poses[:1]

        def refused(code, msg, fn):
            with pytest.raises(capi.DvoError) as ei:
                fn()
            assert ei.value.code == code, (ei.value.code, code, str(ei.value))
            assert str(ei.value) == "dvo error %d: %s" % (code, msg)
            assert same_state(all_voxels(h), before)

        INV, STATE = capi.DVO_ERR_INVALID, capi.DVO_ERR_STATE
        # the words of every refusal, as dvo_capi_tsdf.cpp has had them since the depth fusion was added
        LISTED, NEVER4 = "a listed volume is outside [0, max_volumes)", "volume 4 was never set (dvo_tsdf_set_volume)"
        COUNT, SHAPE, FLAGS = "count < 1 or a NULL argument", "rows or cols < 1, or an unknown depth format", "unknown flags (0 or DVO_UPLOAD_DEVICE)"
        PARAMS = "bad parameters (NULL, 0 < z_near < z_far, both finite, max_weight in [1, 65535])"
        FRAME = "frame %d: a K4 or pose that is not finite, or fx / fy not positive"
        RANGE = "volume outside [0, max_volumes)"
        VOLUME = ("bad volume (NULL, a dimension outside [1, DVO_TSDF_MAX_DIM], voxel_size or trunc not positive, a number that is not "
                  "finite)")
        POINTS = "min_weight < 1, a negative capacity, a NULL buffer with capacity > 0, or a NULL n_points"
        refused(INV, LISTED, lambda: h.integrate([4 + 1], imgs[:1], K, one))                           # a volume index out of range
        refused(INV, LISTED, lambda: h.integrate([-1], imgs[:1], K, one))
        refused(STATE, NEVER4, lambda: h.integrate([4], imgs[:1], K, one))                             # never set
        refused(STATE, NEVER4, lambda: h.integrate([0, 4], imgs[:2], K, poses[:2]))
        refused(INV, COUNT, lambda: h.integrate([], [], K, poses[:0]))                                 # count < 1
        for kw in (dict(z_near=0.0), dict(z_near=9.0), dict(z_far=float("inf")), dict(z_near=float("nan")), dict(max_weight=0), dict(max_weight=65536)):
            refused(INV, PARAMS, lambda: h.integrate([0], imgs[:1], K, one, P(**kw)))
        for k in range(4):
            for value in (float("nan"), float("inf")):
                refused(INV, FRAME % 0, lambda: h.integrate([0], imgs[:1], [value if j == k else K[j] for j in range(4)], one))
        refused(INV, FRAME % 0, lambda: h.integrate([0], imgs[:1], [0.0, 30.0, 15.5, 11.5], one))
        refused(INV, FRAME % 0, lambda: h.integrate([0], imgs[:1], [30.0, -1.0, 15.5, 11.5], one))
        for k in (0, 8, 9, 11):
            bad = one.copy()
            bad[0, k] = np.nan
            refused(INV, FRAME % 0, lambda: h.integrate([0], imgs[:1], K, bad))
        bad = poses[:2].copy()
        bad[1, 3] = np.inf                                                                             # the second frame of a list
        refused(INV, FRAME % 1, lambda: h.integrate([0, 1], imgs[:2], K, bad))
        refused(INV, LISTED, lambda: h.integrate([0, 7], imgs[:2], K, bad))                            # the order of the checks: the list first,
        refused(STATE, NEVER4, lambda: h.integrate([4, 0], imgs[:2], K, poses[:2]))                    # every frame before any "never set"
        refused(INV, FRAME % 1, lambda: h.integrate([4, 0], imgs[:2], K, bad))
        # what the Python mirror cannot express goes through the C ABI: NULL arguments, sizes, an unknown format or flag
        vols = (C.c_int * 1)(0)
        img = (C.c_void_p * 1)(imgs[0].ctypes.data)
        null_img = (C.c_void_p * 1)(None)
        p, Kp, Pp = P(), capi._ptr(K), capi._ptr(np.ascontiguousarray(one))

        def raw(prm=C.byref(p), count=1, v=vols, d=img, fmt=capi.DVO_DEPTH_U16, r=tr.ROWS, c=tr.COLS, k=Kp, q=Pp, flags=0):
            return lib.dvo_tsdf_integrate(h._h, prm, count, v, d, fmt, r, c, k, q, flags)

        for msg, kw in ((PARAMS, dict(prm=None)), (COUNT, dict(v=None)), (COUNT, dict(d=None)), ("a NULL depth image", dict(d=null_img)),
                        (COUNT, dict(k=None)), (COUNT, dict(q=None)), (COUNT, dict(count=0)), (COUNT, dict(count=-2)), (SHAPE, dict(r=0)),
                        (SHAPE, dict(c=0)), (SHAPE, dict(c=-5)), (SHAPE, dict(fmt=2)), (SHAPE, dict(fmt=-1)), (FLAGS, dict(flags=1)),
                        (FLAGS, dict(flags=capi.DVO_UPLOAD_DEVICE | 1)), (FLAGS, dict(flags=-1)), (COUNT, dict(count=0, r=0, flags=9)),
                        (SHAPE, dict(r=0, flags=9))):
            assert raw(**kw) == INV, kw
            assert lib.dvo_tsdf_last_error(h._h).decode() == msg, kw
            assert same_state(all_voxels(h), before)
        # volumes: a bad geometry, an index out of range, one that does not fit the pool (which is full), another count for a volume
        # that is not the last placed
        refused(INV, VOLUME, lambda: h.set_volume(0, c_volume(dict(tr.VOLUMES[0], trunc=0.0))))
        refused(INV, VOLUME, lambda: h.set_volume(0, c_volume(dict(tr.VOLUMES[0], dims=(20, 14, 1025)))))
        refused(INV, RANGE, lambda: h.set_volume(5, c_volume(tr.VOLUMES[3])))
        refused(INV, "the set volumes would hold more voxels than the handle was created for", lambda: h.set_volume(4, c_volume(tr.VOLUMES[3])))
        refused(INV, "a set volume keeps its voxel count unless it is the one placed last",
                lambda: h.set_volume(0, c_volume(dict(tr.VOLUMES[0], dims=(20, 14, 10)))))
        assert lib.dvo_tsdf_set_volume(h._h, 0, None) == INV and lib.dvo_tsdf_last_error(h._h).decode() == VOLUME
        word = np.zeros(1, np.uint32)
        for fn in (lambda: h.clear(4), lambda: h._chk(lib.dvo_tsdf_get_voxels(h._h, 4, capi._ptr(word))),
                   lambda: h._chk(lib.dvo_tsdf_set_voxels(h._h, 4, capi._ptr(word))), lambda: h.points(4)):
            refused(STATE, NEVER4, fn)
        for fn in (lambda: h.clear(-1), lambda: h.clear(5), lambda: h.points(7)):
            refused(INV, RANGE, fn)
        for fn in (lambda: h.points(0, min_weight=0), lambda: h.points(0, capacity=-1)):
            refused(INV, POINTS, fn)
        n = C.c_longlong(0)
        assert lib.dvo_tsdf_extract_points(h._h, 0, 1, None, 4, C.byref(n)) == INV and lib.dvo_tsdf_last_error(h._h).decode() == POINTS
        assert lib.dvo_tsdf_extract_points(h._h, 0, 1, None, 0, None) == INV and lib.dvo_tsdf_last_error(h._h).decode() == POINTS
        assert lib.dvo_tsdf_get_voxels(h._h, 0, None) == INV and lib.dvo_tsdf_last_error(h._h).decode() == "a NULL buffer"
        assert lib.dvo_tsdf_set_voxels(h._h, 0, None) == INV and lib.dvo_tsdf_last_error(h._h).decode() == "a NULL buffer"
        assert same_state(all_voxels(h), before)
        # the handle still works
        h.integrate([0], imgs[:1], K, one)
        assert not np.array_equal(h.voxels(0), before[0]) and same_state(all_voxels(h)[1:], before[1:])
    for bad in ((0, 10), (1, 0), (3, 2), (-1, 10)):
        with pytest.raises(capi.DvoError) as ei:
            capi.DvoTsdfVolumes(*bad)
        assert ei.value.code == capi.DVO_ERR_INVALID
        assert str(ei.value) == "dvo error 1: bad capacities (max_volumes >= 1, max_voxels_total >= max_volumes)"
    with pytest.raises(capi.DvoError) as ei:           # a pool beyond what a handle supports: refused before any allocation is tried
        capi.DvoTsdfVolumes(1, 2 ** 38 + 1)
    assert ei.value.code == capi.DVO_ERR_NOMEM and str(ei.value) == "dvo error 5: a pool above 2^38 voxels is not supported"


def test_lifecycle():
    """clear, then a set_voxels / get_voxels round trip; a volume set again in place; a handle created and destroyed twenty times"""
    from rgbd_odometry_amd import capi
    rng = np.random.RandomState(5)
    with new_handle() as h:
        imgs, poses = tr.frame_list("u16")
        h.integrate(LIST, imgs, tr.K4, poses)
        state = all_voxels(h)
        h.clear(1)
        assert not h.voxels(1).any() and np.array_equal(h.voxels(0), state[0]) and np.array_equal(h.voxels(2), state[2])
        words = [rng.randint(0, 2 ** 32, size=tr.voxels_of(v), dtype=np.uint64).astype(np.uint32) for v in tr.VOLUMES]
        for i in (2, 0, 3, 1):
            h.set_voxels(i, words[i])
        assert same_state(all_voxels(h), words)
        h.set_volume(2, c_volume(dict(tr.VOLUMES[2], trunc=0.3)))          # the same count: in place, cleared, the neighbours untouched
        assert not h.voxels(2).any() and np.array_equal(h.voxels(1), words[1]) and np.array_equal(h.voxels(3), words[3])
        h.set_voxels(2, state[2])
        h.set_voxels(1, state[1])
        assert np.array_equal(h.voxels(2), state[2]) and np.array_equal(h.voxels(1), state[1])
    for k in range(20):
        with capi.DvoTsdfVolumes(2, 4096) as h:
            h.set_volume(k % 2, c_volume(tr.VOLUMES[2]))
            assert not h.voxels(k % 2).any()
