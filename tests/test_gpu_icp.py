"""Frame-to-model alignment on the device (include/dvo_amd.h, "frame-to-model alignment"): dvo_icp_align against the host definition
(dvo_icp_align_host), which tests/test_icp_cpu.py pins to the numpy restatement.  The views are those of tests/icp_reference.py at
24 x 32, 37 x 53 (partial 64-runs, odd sub-grids at levels 1 and 2) and 72 x 88 (more than 4096 pixels: two sweep workgroups per view
at level 0 and a third round of the tree in the solve kernel), and at icp_reference.TREE_SIZES: the list lengths on both sides of every
branch of the two kernels, up to 481 x 545 = 2^18 + 1 entries -- 65 sweep workgroups per view, the solve kernel's fourth round --, which
also runs with four levels.  One handle serves every size.  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import icp_reference as ir
import tsdf_map_reference as tr

pytestmark = pytest.mark.gpu
#: (now format, model format) x settings of the byte-equality cases: the defaults, stop_norm on, Huber and stop_norm with a level of no sweeps
PAIRS = [("u16", "u16"), ("f32", "f32"), ("u16", "f32")]
SETTINGS = [dict(), dict(stop_norm=2e-3), dict(levels=3, iterations=(2, 0, 3), huber=0.001, stop_norm=1e-3), dict(levels=1, iterations=(0,))]


def c_params(**changes):
    from rgbd_odometry_amd import capi
    return capi.DvoIcpParams.default(**changes)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def mixed_views(size):
    """the plane (DEGENERATE) and the frame of holes (FEW) between the good views: stopped views must not disturb their neighbours"""
    g, s = ir.good_views(size), ir.stopping_views(size)
    return [g[0], s[0], g[1], s[1], g[2]]


def arrays(views, now_fmt, model_fmt):
    return ([v["now_" + now_fmt] for v in views], [v["model_" + model_fmt] for v in views], [v["normals"] for v in views],
            np.array([v["K"] for v in views]), np.stack([v["model_pose"] for v in views]), np.stack([v["start_pose"] for v in views]))


_host = {}


def host(size, now_fmt, model_fmt, setting):
    """the host definition's (poses, records) of mixed_views(size); computed once"""
    from rgbd_odometry_amd import capi
    key = (size, now_fmt, model_fmt, tuple(sorted(setting.items())))
    if key not in _host:
        poses, recs = capi.icp_align_host(*arrays(mixed_views(size), now_fmt, model_fmt), c_params(**setting))
        poses.setflags(write=False)
        recs.setflags(write=False)
        _host[key] = (poses, recs)
    return _host[key]


@pytest.fixture(scope="module")
def icp():
    from rgbd_odometry_amd import capi
    h = capi.DvoIcp(8)
    yield h
    h.close()


@pytest.mark.parametrize("size", ir.SIZES)
def test_device_equals_the_host_definition(icp, size):
    """all views of a size in one call, in every format pair and setting; the launches and the one synchronisation of the contract"""
    from rgbd_odometry_amd import capi
    views = mixed_views(size)
    for setting in SETTINGS:
        p = c_params(**setting)
        for now_fmt, model_fmt in PAIRS:
            want_poses, want = host(size, now_fmt, model_fmt, setting)
            poses, recs = icp.align(*arrays(views, now_fmt, model_fmt), p)
            assert icp.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * p.sweeps(), 1), (size, setting)
            assert same_bits(poses, want_poses), (size, setting, now_fmt, model_fmt, [int(r["status"]) for r in recs], want["status"].tolist())
            assert recs.tobytes() == want.tobytes(), (size, setting, now_fmt, model_fmt)
    want_poses, want = host(size, "f32", "f32", SETTINGS[0])
    assert want["status"].tolist() == [ir.OK, ir.DEGENERATE, ir.OK, ir.FEW, ir.OK] and want["iterations"].tolist() == [19, 0, 19, 0, 19]
    assert capi.DVO_ICP_LAUNCHES_PER_SWEEP * c_params().sweeps() == 40


def test_batch_independence(icp):
    """all views in one call (above), one call per view, the list reversed: the same bytes"""
    for size, (now_fmt, model_fmt), setting in ((ir.SIZES[1], PAIRS[0], SETTINGS[0]), (ir.SIZES[2], PAIRS[2], SETTINGS[2])):
        views = mixed_views(size)
        want_poses, want = host(size, now_fmt, model_fmt, setting)
        p = c_params(**setting)
        for i in range(len(views)):
            poses, recs = icp.align(*arrays(views[i:i + 1], now_fmt, model_fmt), p)
            assert same_bits(poses[0], want_poses[i]) and recs[0].tobytes() == want[i].tobytes(), (size, i)
        poses, recs = icp.align(*arrays(views[::-1], now_fmt, model_fmt), p)
        assert same_bits(poses, want_poses[::-1]) and recs.tobytes() == np.ascontiguousarray(want[::-1]).tobytes(), size


def test_both_sweep_kernels_in_one_call():
    """260 views of 72 x 88 with two levels: level 0 is 520 sweep workgroups -- above the number up to which a sweep takes the
    sixteen-wave kernel, so the four-wave kernel runs it --, level 1 is 260: the sixteen-wave kernel.  The bytes are the host's"""
    import os
    import re
    from rgbd_odometry_amd import capi
    launch = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rgbd_odometry_amd", "csrc", "dvo_icp_launch.h")).read()
    most = int(re.search(r"kWideSweepMost\s*=\s*(\d+)", launch).group(1))
    size, repeats = ir.SIZES[2], 52
    views = mixed_views(size)
    n = repeats * len(views)
    assert n * 1 <= most < n * 2 and size[0] * size[1] > 4096 and (size[0] // 2) * (size[1] // 2) <= 4096
    setting = dict(levels=2, iterations=(2, 2))
    want_poses, want = host(size, "f32", "u16", setting)
    with capi.DvoIcp(n) as h:
        poses, recs = h.align(*arrays(views * repeats, "f32", "u16"), c_params(**setting))
        assert h.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * 5, 1)
    assert same_bits(poses, np.tile(want_poses, (repeats, 1))) and recs.tobytes() == np.tile(want, repeats).tobytes()
    assert want["status"].tolist() == [ir.OK, ir.DEGENERATE, ir.OK, ir.FEW, ir.OK]


def launch_constant(name):
    import os
    import re
    launch = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rgbd_odometry_amd", "csrc", "dvo_icp_launch.h")).read()
    return int(re.search(r"%s\s*=\s*(\d+)" % name, launch).group(1))


#: the list lengths around every branch of the sweep and the solve kernel: one format pair per size, all three at 481 x 545
TREE_CASES = [(size, PAIRS[k % 3]) for k, size in enumerate(ir.TREE_SIZES[:-1])] + [(ir.TREE_TOP, pair) for pair in PAIRS]
GROUP = 64 * 64                                  # kGroup of dvo_icp_launch.h: the entries of one sweep workgroup
TREE_STATUS, TREE_UPDATES = [ir.OK, ir.DEGENERATE, ir.OK, ir.FEW, ir.OK, ir.OK], [4, 0, 4, 0, 4, 4]


def tree_views(size):
    """mixed_views and the view whose last list entries stay paired until the record's sweep (icp_reference.tail_view): at 481 x 545
    the one entry of the 65th sweep workgroup, which is all of the fourth round's second value"""
    return mixed_views(size) + [ir.tail_view(size)]


def tree_host(size, now_fmt, model_fmt):
    """the host definition's (poses, records) of tree_views(size) with icp_reference.TREE_SETTING; computed once"""
    from rgbd_odometry_amd import capi
    key = ("tree", size, now_fmt, model_fmt)
    if key not in _host:
        poses, recs = capi.icp_align_host(*arrays(tree_views(size), now_fmt, model_fmt), c_params(**ir.TREE_SETTING))
        poses.setflags(write=False)
        recs.setflags(write=False)
        _host[key] = (poses, recs)
    return _host[key]


def check_call(h, views, now_fmt, model_fmt, setting, want_poses, want, where):
    from rgbd_odometry_amd import capi
    p = c_params(**setting)
    poses, recs = h.align(*arrays(views, now_fmt, model_fmt), p)
    assert h.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * p.sweeps(), 1), where
    assert same_bits(poses, want_poses), (where, [int(r["status"]) for r in recs], [int(r["iterations"]) for r in recs])
    assert recs.tobytes() == np.ascontiguousarray(want).tobytes(), where


@pytest.mark.parametrize("size,pair", TREE_CASES)
def test_tree_boundaries(icp, size, pair):
    """64 / 65 entries (the sweep kernel's single round against its second), 4096 / 4100 (one sweep workgroup against two, the solve
    kernel's third round), 2^18 / 2^18 + 1 (64 workgroups against 65: the third round with every lane and group loaded, and the fourth).
    The stopped views' workgroups sit between live ones; the last view keeps the last entries of its list paired"""
    entries = size[0] * size[1]
    assert entries in (64, 65, GROUP, GROUP + 4, 64 * GROUP, 64 * GROUP + 1)
    want_poses, want = tree_host(size, pair[0], pair[1])
    check_call(icp, tree_views(size), pair[0], pair[1], ir.TREE_SETTING, want_poses, want, (size, pair))
    assert want["status"].tolist() == TREE_STATUS and want["iterations"].tolist() == TREE_UPDATES


@pytest.mark.parametrize("size,setting", ir.LEVEL3_CASES)
def test_level_3(icp, size, setting):
    """levels = 4: i << 3 and lists of ceil(rows / 8) x ceil(cols / 8); every OK view applied the updates of every level"""
    for now_fmt, model_fmt in (PAIRS if size != ir.TREE_TOP else PAIRS[2:]):
        want_poses, want = host(size, now_fmt, model_fmt, setting)
        check_call(icp, mixed_views(size), now_fmt, model_fmt, setting, want_poses, want, (size, now_fmt, model_fmt))
    assert want["status"].tolist() == [ir.OK, ir.DEGENERATE, ir.OK, ir.FEW, ir.OK]
    assert want["iterations"].tolist() == [sum(setting["iterations"]), 0] * 2 + [sum(setting["iterations"])] and setting["iterations"][3] > 0


def test_sum_order_in_the_upper_rounds(icp):
    """the wide-range view at 481 x 545, whose sums tests/test_icp_cpu.py shows to depend on the association of the third and fourth
    round: the record without updates and the pose after three.  Then at 724 x 725 -- 129 sweep workgroups, three values in the fourth
    round: the fewest whose order shows"""
    from rgbd_odometry_amd import capi
    for size in (ir.TREE_TOP, ir.TREE_DEEP):
        v = ir.wide_range_view(size=size)
        for setting in (dict(levels=1, iterations=(0,)), dict(levels=1, iterations=(3,), min_pivot_ratio=1e-30)):
            want_poses, want = capi.icp_align_host(*arrays([v], "f32", "f32"), c_params(**setting))
            assert want["status"].tolist() == [ir.OK] and want["iterations"].tolist() == [setting["iterations"][0]]
            check_call(icp, [v], "f32", "f32", setting, want_poses, want, (size, setting))


def test_one_handle_across_sizes():
    """a new handle at 481 x 545, then 24 x 32, then 481 x 545 again: the partials buffer is kept and its pitch goes 65, 1, 65"""
    from rgbd_odometry_amd import capi
    with capi.DvoIcp(6) as h:
        for size, pair in ((ir.TREE_TOP, PAIRS[0]), (ir.SIZES[0], PAIRS[0]), (ir.TREE_TOP, PAIRS[1])):
            want_poses, want = tree_host(size, pair[0], pair[1])
            check_call(h, tree_views(size), pair[0], pair[1], ir.TREE_SETTING, want_poses, want, (size, pair))
            assert want["status"].tolist() == TREE_STATUS and want["iterations"].tolist() == TREE_UPDATES


def test_batch_independence_with_a_fourth_round(icp):
    """481 x 545: one call per view and the list reversed give the bytes of the batch"""
    size, (now_fmt, model_fmt) = ir.TREE_TOP, PAIRS[2]
    views = tree_views(size)
    want_poses, want = tree_host(size, now_fmt, model_fmt)
    for i in range(len(views)):
        check_call(icp, views[i:i + 1], now_fmt, model_fmt, ir.TREE_SETTING, want_poses[i:i + 1], want[i:i + 1], i)
    check_call(icp, views[::-1], now_fmt, model_fmt, ir.TREE_SETTING, want_poses[::-1], want[::-1], "reversed")


def test_both_sweep_kernels_with_a_fourth_round(icp):
    """481 x 545 is 65 sweep workgroups per view.  Six views are 390 -- at most kWideSweepMost: the sixteen-wave kernel runs views of
    many workgroups --; eight are 520, above it: the four-wave kernel does, with 65 workgroups per view in its index arithmetic"""
    size, (now_fmt, model_fmt) = ir.TREE_TOP, PAIRS[1]
    most, blocks = launch_constant("kWideSweepMost"), -(-(size[0] * size[1]) // GROUP)
    views = tree_views(size)
    assert blocks == 65 and len(views) * blocks <= most < 8 * blocks
    want_poses, want = tree_host(size, now_fmt, model_fmt)
    check_call(icp, views, now_fmt, model_fmt, ir.TREE_SETTING, want_poses, want, "sixteen waves")
    pick = [0, 1, 2, 3, 4, 5, 2, 5]
    check_call(icp, [views[i] for i in pick], now_fmt, model_fmt, ir.TREE_SETTING, want_poses[pick], want[pick], "four waves")


def test_device_images_at_481_x_545(icp):
    """DVO_UPLOAD_DEVICE at the size of the fourth round: the bytes of host images, and no input changes"""
    import torch
    from rgbd_odometry_amd import capi
    size, (now_fmt, model_fmt) = ir.TREE_TOP, PAIRS[2]
    now, model, nrm, K, Pm, Ps = arrays(tree_views(size), now_fmt, model_fmt)
    as_torch = lambda a: torch.from_numpy(np.array(a).view(np.int16) if a.dtype == np.uint16 else np.array(a)).cuda()
    tn, tm, tq = [as_torch(a) for a in now], [as_torch(a) for a in model], [as_torch(a) for a in nrm]
    torch.cuda.synchronize()
    want_poses, want = tree_host(size, now_fmt, model_fmt)
    poses, recs = icp.align(tn, tm, tq, K, Pm, Ps, c_params(**ir.TREE_SETTING), device=True)
    assert icp.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * c_params(**ir.TREE_SETTING).sweeps(), 1)
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()
    for t, a in zip(tn + tm + tq, now + model + nrm):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_device_images_are_read_in_place_and_not_modified(icp):
    """DVO_UPLOAD_DEVICE torch tensors give the bytes of host images, and no input changes"""
    import torch
    from rgbd_odometry_amd import capi
    for size, (now_fmt, model_fmt) in ((ir.SIZES[1], PAIRS[2]), (ir.SIZES[2], PAIRS[1])):
        views = mixed_views(size)
        now, model, nrm, K, Pm, Ps = arrays(views, now_fmt, model_fmt)
        as_torch = lambda a: torch.from_numpy(np.array(a).view(np.int16) if a.dtype == np.uint16 else np.array(a)).cuda()
        tn, tm, tq = [as_torch(a) for a in now], [as_torch(a) for a in model], [as_torch(a) for a in nrm]
        torch.cuda.synchronize()
        want_poses, want = host(size, now_fmt, model_fmt, SETTINGS[0])
        poses, recs = icp.align(tn, tm, tq, K, Pm, Ps, device=True)
        assert icp.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * c_params().sweeps(), 1)
        assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes(), size
        for t, a in zip(tn + tm + tq, now + model + nrm):
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
        before = [np.array(a) for a in now + model + nrm]
        icp.align(now, model, nrm, K, Pm, Ps)
        assert all(same_bits(a, b) for a, b in zip(now + model + nrm, before))


def test_refusals_write_nothing():
    from rgbd_odometry_amd import capi
    views = ir.good_views(ir.SIZES[0])[:2]
    rows, cols = ir.SIZES[0]
    now, model, nrm, K, Pm, Ps = arrays(views, "u16", "u16")
    lists = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    half = lambda arrs: (C.c_void_p * 2)(arrs[0].ctypes.data, None)
    poses = np.full((2, 12), -7.5)
    recs = np.zeros(2, capi.ICP_RECORD_DTYPE)
    recs.view(np.uint8)[:] = 0x5A
    prm = c_params()
    INV = capi.DVO_ERR_INVALID
    with capi.DvoIcp(2) as h:
        lib = h.lib

        def raw(p=prm, count=2, nf=capi.DVO_DEPTH_U16, mf=capi.DVO_DEPTH_U16, r=rows, c=cols, k=K, n=lists(now), m=lists(model), q=lists(nrm), pm=Pm, ps=Ps,
                out=poses, rec=recs, flags=0):
            ptr = lambda a: None if a is None else capi._ptr(a)
            return lib.dvo_icp_align(h._h, None if p is None else C.byref(p), count, nf, mf, r, c, ptr(k), n, m, q, ptr(pm), ptr(ps), ptr(out), ptr(rec), flags)

        def untouched():
            return np.all(poses == -7.5) and np.all(recs.view(np.uint8) == 0x5A)

        nan, inf = float("nan"), float("inf")
        PARAMS = ("bad parameters (levels in [1, DVO_ICP_MAX_LEVELS], iterations in [0, DVO_ICP_MAX_ITERATIONS], 0 < z_near < z_far, dist_max > 0, "
                  "huber and stop_norm >= 0, min_pivot_ratio inside (0, 1), all finite, min_count >= 1)")
        COUNT, MAX, FLAGS, IMAGE = "count < 1 or a NULL argument", "count above max_views", "unknown flags (0 or DVO_UPLOAD_DEVICE)", "a NULL image"
        SHAPE = "rows or cols < 1, rows * cols > DVO_ICP_MAX_PIXELS, or an unknown depth format"
        VIEW = "view %d: a K4 or pose that is not finite, or fx / fy not positive"
        bad = [(COUNT, dict(k=None)), (COUNT, dict(n=None)), (COUNT, dict(m=None)), (COUNT, dict(q=None)), (COUNT, dict(pm=None)), (COUNT, dict(ps=None)),
               (COUNT, dict(out=None)), (COUNT, dict(rec=None)), (COUNT, dict(count=0)), (COUNT, dict(count=-1)), (MAX, dict(count=3)),
               (SHAPE, dict(r=0)), (SHAPE, dict(c=-2)), (SHAPE, dict(r=4097, c=4096)), (SHAPE, dict(nf=2)), (SHAPE, dict(mf=-1)),
               (FLAGS, dict(flags=1)), (FLAGS, dict(flags=capi.DVO_UPLOAD_DEVICE | 1)), (FLAGS, dict(flags=-1)),
               (IMAGE, dict(n=half(now))), (IMAGE, dict(m=half(model))), (IMAGE, dict(q=half(nrm))),
               (COUNT, dict(count=0, r=0, flags=9)), (SHAPE, dict(r=0, flags=9)), (FLAGS, dict(flags=9, n=half(now)))]      # the order of the checks
        bad += [(PARAMS, dict(p=c_params(**kw))) for kw in (dict(levels=0), dict(levels=5), dict(iterations=(65,)), dict(iterations=(1, -1)), dict(z_near=0.0),
                                                              dict(z_near=9.0), dict(z_far=nan), dict(dist_max=0.0), dict(dist_max=inf), dict(huber=-1.0),
                                                              dict(stop_norm=-1.0), dict(stop_norm=nan), dict(min_pivot_ratio=0.0), dict(min_pivot_ratio=1.0),
                                                              dict(min_count=0))]
        for j in (0, 3):
            Kb = K.copy()
            Kb[1, j] = nan
            bad.append((VIEW % 1, dict(k=Kb)))
        bad.append((VIEW % 0, dict(k=np.array([[0.0, 30.0, 15.5, 11.5], [30.0, 30.0, 15.5, 11.5]]))))
        for which in ("pm", "ps"):
            Pb = (Pm if which == "pm" else Ps).copy()
            Pb[1, 10] = inf
            bad.append((VIEW % 1, {which: Pb}))
        for msg, kw in bad:
            assert raw(**kw) == INV, kw
            assert lib.dvo_icp_last_error(h._h).decode() == msg, kw
            assert untouched(), kw
        with pytest.raises(capi.DvoError) as ei:
            h.align(now, model, nrm, K, Pm, Ps, c_params(levels=9))
        assert ei.value.code == INV and str(ei.value) == "dvo error 1: " + PARAMS
        # the handle still works; p NULL is the defaults
        assert raw(p=None) == capi.DVO_OK and h.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * prm.sweeps(), 1)
        want_poses, want = capi.icp_align_host(now, model, nrm, K, Pm, Ps)
        assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()
    out = C.c_void_p()
    assert lib.dvo_icp_create(0, C.byref(out)) == INV and lib.dvo_icp_last_error(None).decode() == "max_views < 1" and not out.value


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


#: the end-to-end case: per view (volume, the fusion pose the model is rendered from, the pose the now depth is rendered from)
CHAIN = [(1, 0, 3), (0, 0, 4), (1, 1, 6), (2, 3, 0), (3, 6, 0), (1, 4, 3)]


@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_render_align_chain_on_the_device(fmt):
    """fuse the four volumes of tests/tsdf_map_reference.py, render model views (depth and normals) and second depth views into device
    memory, align the second against the first from the model's pose -- nothing but poses and records leaves the device -- and compare
    with the same chain through the three host definitions"""
    from rgbd_odometry_amd import capi
    rows, cols = tr.ROWS, tr.COLS
    imgs, fusion_poses = tr.frame_list("u16")
    vols = [c for c, _, _ in CHAIN]
    model_poses = np.stack([tr.POSES[a] for _, a, _ in CHAIN])
    now_poses = np.stack([tr.POSES[b] for _, _, b in CHAIN])
    # the host chain
    words = []
    for vi, vol in enumerate(tr.VOLUMES):
        idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
        words.append(capi.tsdf_integrate_host(c_volume(vol), None, [imgs[i] for i in idx], tr.K4, fusion_poses[idx]))
    md, mn, nd = [], [], []
    for k, vi in enumerate(vols):
        d, n = capi.tsdf_raycast_host(c_volume(tr.VOLUMES[vi]), words[vi], tr.K4, model_poses[k:k + 1], rows, cols, None, fmt, True)
        md.append(d[0])
        mn.append(n[0])
        nd.append(capi.tsdf_raycast_host(c_volume(tr.VOLUMES[vi]), words[vi], tr.K4, now_poses[k:k + 1], rows, cols, None, fmt)[0])
    want_poses, want = capi.icp_align_host(nd, md, mn, tr.K4, model_poses, model_poses)
    assert (want["status"] == ir.OK).sum() >= 2 and want["iterations"].max() == 19 and (want["status"] == ir.FEW).sum() >= 2
    # the device chain
    with capi.DvoTsdfVolumes(len(tr.VOLUMES), sum(tr.voxels_of(v) for v in tr.VOLUMES)) as maps, capi.DvoIcp(len(CHAIN)) as icp:
        for i, vol in enumerate(tr.VOLUMES):
            maps.set_volume(i, c_volume(vol))
        maps.integrate(tr.FRAME_VOLUMES, imgs, tr.K4, fusion_poses)
        model_d, model_n = maps.raycast(vols, tr.K4, model_poses, rows, cols, fmt=fmt, normals=True, device=True)
        now_d = maps.raycast(vols, tr.K4, now_poses, rows, cols, fmt=fmt, device=True)
        poses, recs = icp.align(list(now_d), list(model_d), list(model_n), tr.K4, model_poses, model_poses, device=True)
        assert icp.stats() == (capi.DVO_ICP_LAUNCHES_PER_SWEEP * c_params().sweeps(), 1)
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()
