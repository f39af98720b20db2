"""The front end of the frame-to-model alignment on the device (include/dvo_amd.h, "preparing a depth frame"): dvo_icp_prepare and
dvo_icp_align_gated against the host definitions (dvo_icp_prepare_host, dvo_icp_align_gated_host), which
tests/test_icp_prepare_cpu.py pins to the numpy restatement.  The images are those of tests/icp_prepare_reference.py at 5 x 13 (the
window of radius 6 is larger than the image), 24 x 32, 37 x 53 and 72 x 88 (several tiles of the filter kernel), and at 16 x 64,
32 x 128 and 17 x 65: the last row and column end a tile, or begin one.  One handle serves every case.  All comparisons are byte
equality."""
import ctypes as C

import numpy as np
import pytest

import icp_prepare_reference as pr
import icp_reference as ir

pytestmark = pytest.mark.gpu
FORMATS = ["u16", "f32"]
#: the sizes of icp_prepare_reference and the tile borders of the filter kernel (16 rows x 64 columns per workgroup)
SIZES = pr.FILTER_SIZES + [(16, 64), (32, 128), (17, 65)]
PAIRS = [("u16", "u16"), ("f32", "f32"), ("u16", "f32")]
SETTINGS = [dict(), dict(levels=3, iterations=(2, 0, 3), huber=0.001, stop_norm=1e-3)]


def capi():
    from rgbd_odometry_amd import capi as m
    return m


def c_params(**changes):
    return capi().DvoIcpParams.default(**changes)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_lists(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def icp():
    h = capi().DvoIcp(8)
    yield h
    h.close()


_host = {}


def host_prepared(size, fmt, radius):
    """the host definition's (filtered, normals) of filter_inputs(size, fmt) at a radius; computed once"""
    key = ("prepared", size, fmt, radius)
    if key not in _host:
        m = capi()
        out, nrm = m.icp_prepare_host(pr.filter_inputs(size, fmt), ir.k4_for(*size), m.DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05))
        for a in out + nrm:
            a.setflags(write=False)
        _host[key] = (out, nrm)
    return _host[key]


def mixed_views(size):
    """the plane (DEGENERATE) and the frame of holes (FEW) between the good views"""
    g, s = ir.good_views(size), ir.stopping_views(size)
    return [g[0], s[0], g[1], s[1], g[2]]


def arrays(views, now_fmt, model_fmt):
    return ([v["now_" + now_fmt] for v in views], [v["model_" + model_fmt] for v in views], [v["normals"] for v in views],
            np.array([v["K"] for v in views]), np.stack([v["model_pose"] for v in views]), np.stack([v["start_pose"] for v in views]))


def host_gate(size, now_fmt):
    """the now normals of mixed_views(size): the host definition's, default tables; computed once"""
    key = ("gate", size, now_fmt)
    if key not in _host:
        m = capi()
        views = mixed_views(size)
        prm = m.DvoIcpPrepareParams.gaussian(pr.DEFAULT[0], pr.DEFAULT[1], pr.DEFAULT[2], pr.GATE_EDGE_MAX[size])
        _host[key] = m.icp_prepare_host([v["now_" + now_fmt] for v in views], np.array([v["K"] for v in views]), prm)[1]
    return _host[key]


def host_gated(size, now_fmt, model_fmt, setting):
    """the host definition's gated (poses, records) of mixed_views(size); computed once"""
    key = ("gated", size, now_fmt, model_fmt, tuple(sorted(setting.items())))
    if key not in _host:
        _host[key] = capi().icp_align_host(*arrays(mixed_views(size), now_fmt, model_fmt), c_params(**setting), now_normals=host_gate(size, now_fmt),
                                           normal_cos_min=pr.COS_MIN)
    return _host[key]


@pytest.mark.parametrize("size", SIZES)
def test_device_equals_the_host_definition(icp, size):
    """five images per call (clean, holed, all holes, a noisy holed plane and, in f32, one with NaN, inf, negative and zero pixels) at
    every radius in both formats, with and without normals; two launches and one synchronisation, or one and one"""
    m = capi()
    K = ir.k4_for(*size)
    for fmt in FORMATS:
        imgs = pr.filter_inputs(size, fmt)
        for radius in pr.RADII:
            prm = m.DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
            want, want_n = host_prepared(size, fmt, radius)
            out, nrm = icp.prepare(imgs, K, prm)
            assert icp.stats() == (m.DVO_ICP_PREPARE_LAUNCHES, 1) == (2, 1)
            assert same_lists(out, want), (size, fmt, radius)
            assert same_lists(nrm, want_n), (size, fmt, radius)
            only = icp.prepare(imgs, K, prm, normals=False)
            assert icp.stats() == (1, 1)
            assert same_lists(only, want), (size, fmt, radius)
    # NULL parameters are the default
    want, want_n = m.icp_prepare_host(pr.filter_inputs(size, "u16"), K)
    out, nrm = icp.prepare(pr.filter_inputs(size, "u16"), K)
    assert same_lists(out, want) and same_lists(nrm, want_n)


def test_batch_independence(icp):
    """all images in one call (above), one call per image, the list reversed: the same bytes"""
    m = capi()
    for size, fmt, radius in ((ir.SIZES[1], "u16", 3), (ir.SIZES[2], "f32", 6), ((17, 65), "u16", 1)):
        imgs, K = pr.filter_inputs(size, fmt), ir.k4_for(*size)
        prm = m.DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
        want, want_n = host_prepared(size, fmt, radius)
        for i in range(len(imgs)):
            out, nrm = icp.prepare(imgs[i:i + 1], K, prm)
            assert same_bits(out[0], want[i]) and same_bits(nrm[0], want_n[i]), (size, i)
        out, nrm = icp.prepare(imgs[::-1], K, prm)
        assert same_lists(out, want[::-1]) and same_lists(nrm, want_n[::-1]), size


def as_torch(a):
    import torch
    return torch.from_numpy(np.array(a).view(np.int16) if a.dtype == np.uint16 else np.array(a)).cuda()


def test_device_in_and_out(icp):
    """inputs in device memory, outputs into device buffers read back by the test: the bytes of the staged call, the inputs unchanged;
    equal in and out pointers are refused with nothing written"""
    import torch
    m = capi()
    for size, fmt, radius in ((ir.SIZES[1], "u16", 3), (ir.SIZES[2], "f32", 3), ((32, 128), "f32", 6)):
        imgs, K = pr.filter_inputs(size, fmt), ir.k4_for(*size)
        prm = m.DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
        want, want_n = host_prepared(size, fmt, radius)
        dev = [as_torch(a) for a in imgs]
        torch.cuda.synchronize()
        out, nrm = icp.prepare(dev, K, prm, device=True)
        assert icp.stats() == (2, 1)
        assert same_lists([t.cpu().numpy() for t in out], want) and same_lists([t.cpu().numpy() for t in nrm], want_n), size
        only = icp.prepare(dev, K, prm, normals=False, device=True)
        assert icp.stats() == (1, 1) and same_lists([t.cpu().numpy() for t in only], want)
        for t, a in zip(dev, imgs):
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    # f32 in place: refused, nothing written
    rows, cols = ir.SIZES[1]
    src = [as_torch(a) for a in pr.filter_inputs(ir.SIZES[1], "f32")[:2]]
    other = torch.full((rows, cols), -7.5, dtype=torch.float32, device="cuda")
    nrm = [torch.full((rows, cols, 3), -7.5, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    before = [t.cpu().numpy().copy() for t in src]
    K2 = np.array([ir.k4_for(rows, cols)] * 2)
    ptrs = lambda ts: (C.c_void_p * 2)(*[int(t.data_ptr()) for t in ts])
    rc = icp.lib.dvo_icp_prepare(icp._h, None, 2, m.DVO_DEPTH_F32, rows, cols, m._ptr(K2), ptrs(src), ptrs([other, src[1]]), ptrs(nrm), m.DVO_UPLOAD_DEVICE)
    assert rc == m.DVO_ERR_INVALID and "depth_out is its depth" in icp.lib.dvo_icp_last_error(icp._h).decode()
    torch.cuda.synchronize()
    assert all(same_bits(t.cpu().numpy(), b) for t, b in zip(src, before))
    assert bool((other == -7.5).all()) and all(bool((t == -7.5).all()) for t in nrm)


def test_refusals_write_nothing():
    m = capi()
    rows, cols = ir.SIZES[0]
    imgs = [np.ascontiguousarray(a) for a in pr.filter_inputs(ir.SIZES[0], "u16")[:2]]
    out = [np.full((rows, cols), -7.5, np.float32) for _ in range(2)]
    nrm = [np.full((rows, cols, 3), -7.5, np.float32) for _ in range(2)]
    lists = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    half = lambda arrs: (C.c_void_p * 2)(arrs[0].ctypes.data, None)
    K = np.array([ir.k4_for(rows, cols)] * 2)
    INV = m.DVO_ERR_INVALID
    with m.DvoIcp(2) as h:
        lib = h.lib

        def changed(**kw):
            p = m.DvoIcpPrepareParams.default()
            for k, v in kw.items():
                if k == "range0":
                    p.range[0] = v
                elif k == "centre":
                    p.spatial[p.radius * (2 * p.radius + 1) + p.radius] = v
                else:
                    setattr(p, k, v)
            return p

        def raw(p=None, count=2, fmt=m.DVO_DEPTH_U16, r=rows, c=cols, k=K, d=lists(imgs), o=lists(out), q=lists(nrm), flags=0):
            return lib.dvo_icp_prepare(h._h, None if p is None else C.byref(p), count, fmt, r, c, None if k is None else m._ptr(k), d, o, q, flags)

        untouched = lambda: all(np.all(a == -7.5) for a in out + nrm)
        nan, inf = float("nan"), float("inf")
        PARAMS = ("bad parameters (radius in [0, DVO_ICP_PREPARE_MAX_RADIUS], reserved 0, range_scale and edge_max finite and > 0, range[0] and the centre's "
                  "spatial weight >= 1)")
        COUNT, MAX, FLAGS, IMAGE = "count < 1 or a NULL argument", "count above max_views", "unknown flags (0 or DVO_UPLOAD_DEVICE)", "a NULL image"
        SHAPE = "rows or cols < 1, rows * cols > DVO_ICP_MAX_PIXELS, or an unknown depth format"
        VIEW = "image %d: a K4 that is not finite, or fx / fy not positive"
        bad = [(COUNT, dict(k=None)), (COUNT, dict(d=None)), (COUNT, dict(o=None)), (COUNT, dict(count=0)), (COUNT, dict(count=-1)), (MAX, dict(count=3)),
               (SHAPE, dict(r=0)), (SHAPE, dict(c=-2)), (SHAPE, dict(r=4097, c=4096)), (SHAPE, dict(fmt=2)), (SHAPE, dict(fmt=-1)),
               (FLAGS, dict(flags=1)), (FLAGS, dict(flags=m.DVO_UPLOAD_DEVICE | 1)), (FLAGS, dict(flags=-1)),
               (IMAGE, dict(d=half(imgs))), (IMAGE, dict(o=half(out))), (IMAGE, dict(q=half(nrm)))]
        bad += [(PARAMS, dict(p=changed(**kw))) for kw in (dict(radius=-1), dict(radius=7), dict(reserved=2), dict(range_scale=0.0), dict(range_scale=nan),
                                                            dict(range_scale=inf), dict(edge_max=0.0), dict(edge_max=-1.0), dict(edge_max=nan),
                                                            dict(range0=0), dict(centre=0))]
        for j in (0, 3):
            Kb = K.copy()
            Kb[1, j] = nan
            bad.append((VIEW % 1, dict(k=Kb)))
        bad.append((VIEW % 0, dict(k=np.array([[0.0, 30.0, 15.5, 11.5], [30.0, 30.0, 15.5, 11.5]]))))
        for msg, kw in bad:
            assert raw(**kw) == INV, kw
            assert lib.dvo_icp_last_error(h._h).decode() == msg, kw
            assert untouched(), kw
        # the gated alignment's own refusals
        views = ir.good_views(ir.SIZES[0])[:2]
        now, model, normals, Kv, Pm, Ps = arrays(views, "u16", "u16")
        gate = [np.ascontiguousarray(g) for g in m.icp_prepare_host(now, Kv)[1]]
        poses = np.full((2, 12), -7.5)
        recs = np.zeros(2, m.ICP_RECORD_DTYPE)
        recs.view(np.uint8)[:] = 0x5A
        keep = [[np.ascontiguousarray(a) for a in lst] for lst in (now, model, normals)]

        def gated(g=lists(gate), cos_min=0.9, flags=0):
            return lib.dvo_icp_align_gated(h._h, None, 2, m.DVO_DEPTH_U16, m.DVO_DEPTH_U16, rows, cols, m._ptr(Kv), lists(keep[0]), lists(keep[1]), lists(keep[2]),
                                           m._ptr(Pm), m._ptr(Ps), g, cos_min, m._ptr(poses), m._ptr(recs), flags)

        COS = "normal_cos_min not finite or outside [-1, 1]"
        for msg, kw in ((IMAGE, dict(g=half(gate))), (COS, dict(cos_min=nan)), (COS, dict(cos_min=inf)), (COS, dict(cos_min=1.5)), (COS, dict(cos_min=-1.01)),
                        (FLAGS, dict(flags=3))):
            assert gated(**kw) == INV, kw
            assert lib.dvo_icp_last_error(h._h).decode() == msg, kw
            assert np.all(poses == -7.5) and np.all(recs.view(np.uint8) == 0x5A), kw
        # the handle still works
        assert raw() == m.DVO_OK and h.stats() == (2, 1) and not untouched()
        want, want_n = m.icp_prepare_host(imgs, K[0])
        assert same_lists(out + nrm, want + want_n)
        assert gated() == m.DVO_OK and h.stats() == (m.DVO_ICP_LAUNCHES_PER_SWEEP * c_params().sweeps(), 1)
        want_poses, want_recs = m.icp_align_host(now, model, normals, Kv, Pm, Ps, now_normals=gate, normal_cos_min=0.9)
        assert same_bits(poses, want_poses) and recs.tobytes() == want_recs.tobytes()


# ---- the gated alignment ----

def check_gated(h, views, now_fmt, model_fmt, setting, gate, want_poses, want, where):
    m = capi()
    p = c_params(**setting)
    poses, recs = h.align(*arrays(views, now_fmt, model_fmt), p, now_normals=gate, normal_cos_min=pr.COS_MIN)
    assert h.stats() == (m.DVO_ICP_LAUNCHES_PER_SWEEP * p.sweeps(), 1), where
    assert same_bits(poses, want_poses), (where, [int(r["status"]) for r in recs], [int(r["iterations"]) for r in recs])
    assert recs.tobytes() == np.ascontiguousarray(want).tobytes(), where


@pytest.mark.parametrize("size", ir.SIZES + [(50, 82)])
def test_gated_device_equals_the_host_definition(icp, size):
    """good views, the plane and the frame of holes in one call, in both settings; three format pairs at 37 x 53.  50 x 82 is 4100
    entries: two sweep workgroups and the solve kernel's third round.  The gate takes effect: the gated records count fewer pixels"""
    m = capi()
    views = mixed_views(size)
    assert size != (50, 82) or size in ir.TREE_SIZES and size[0] * size[1] > 4096
    for now_fmt, model_fmt in (PAIRS if size == ir.SIZES[1] else PAIRS[2:]):
        gate = host_gate(size, now_fmt)
        for setting in SETTINGS:
            want_poses, want = host_gated(size, now_fmt, model_fmt, setting)
            check_gated(icp, views, now_fmt, model_fmt, setting, gate, want_poses, want, (size, now_fmt, model_fmt, setting))
            _, open_recs = m.icp_align_host(*arrays(views, now_fmt, model_fmt), c_params(**setting))
            assert all(int(a["count"]) < int(b["count"]) for a, b in zip(want, open_recs) if int(b["count"]) > 0)
            assert want["status"].tolist()[1::2] == [ir.DEGENERATE, ir.FEW]


def test_both_sweep_kernels_gated():
    """260 views of 72 x 88 with two levels, the construction of test_gpu_icp.test_both_sweep_kernels_in_one_call: level 0 is 520 sweep
    workgroups -- the four-wave kernel --, level 1 is 260: the sixteen-wave kernel, both in their gated form"""
    import os
    import re
    m = capi()
    launch = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rgbd_odometry_amd", "csrc", "dvo_icp_launch.h")).read()
    most = int(re.search(r"kWideSweepMost\s*=\s*(\d+)", launch).group(1))
    size, repeats = ir.SIZES[2], 52
    views = mixed_views(size)
    n = repeats * len(views)
    assert n * 1 <= most < n * 2 and size[0] * size[1] > 4096 and (size[0] // 2) * (size[1] // 2) <= 4096
    setting = dict(levels=2, iterations=(2, 2))
    gate = host_gate(size, "f32")
    want_poses, want = host_gated(size, "f32", "u16", setting)
    with m.DvoIcp(n) as h:
        poses, recs = h.align(*arrays(views * repeats, "f32", "u16"), c_params(**setting), now_normals=list(gate) * repeats, normal_cos_min=pr.COS_MIN)
        assert h.stats() == (m.DVO_ICP_LAUNCHES_PER_SWEEP * 5, 1)
    assert same_bits(poses, np.tile(want_poses, (repeats, 1))) and recs.tobytes() == np.tile(want, repeats).tobytes()


def test_the_whole_hand_off_on_the_device(icp):
    """37 x 53: prepare(DVO_UPLOAD_DEVICE) writes filtered depth and normals into device buffers, align(DVO_UPLOAD_DEVICE) reads the
    normals where prepare wrote them (and the filtered depth as its now depth).  Poses and records equal the host pipeline's"""
    import torch
    m = capi()
    size = ir.SIZES[1]
    views = mixed_views(size)
    now, model, normals, K, Pm, Ps = arrays(views, "u16", "f32")
    prm = m.DvoIcpPrepareParams.gaussian(pr.DEFAULT[0], pr.DEFAULT[1], pr.DEFAULT[2], pr.GATE_EDGE_MAX[size])
    F, N = m.icp_prepare_host(now, K, prm)
    want_poses, want = m.icp_align_host(F, model, normals, K, Pm, Ps, now_normals=N, normal_cos_min=pr.COS_MIN)
    assert (want["status"] == ir.OK).sum() == 3
    tn, tm, tq = [as_torch(a) for a in now], [as_torch(a) for a in model], [as_torch(a) for a in normals]
    torch.cuda.synchronize()
    dF, dN = icp.prepare(tn, K, prm, device=True)
    assert icp.stats() == (2, 1)
    poses, recs = icp.align(dF, tm, tq, K, Pm, Ps, device=True, now_normals=dN, normal_cos_min=pr.COS_MIN)
    assert icp.stats() == (m.DVO_ICP_LAUNCHES_PER_SWEEP * c_params().sweeps(), 1)
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()
    assert same_lists([t.cpu().numpy() for t in dF], F) and same_lists([t.cpu().numpy() for t in dN], N)


def test_ungated_bytes(icp):
    """align with now_normals=None is dvo_icp_align: the bytes of icp_align_host"""
    m = capi()
    size = ir.SIZES[1]
    views = mixed_views(size)
    want_poses, want = m.icp_align_host(*arrays(views, "u16", "f32"))
    poses, recs = icp.align(*arrays(views, "u16", "f32"), now_normals=None, normal_cos_min=0.9)
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()
    lists = [(C.c_void_p * len(views))(*[np.ascontiguousarray(a).ctypes.data for a in lst]) for lst in arrays(views, "u16", "f32")[:3]]
    _, _, _, K, Pm, Ps = arrays(views, "u16", "f32")
    poses2, recs2 = np.zeros((len(views), 12)), np.zeros(len(views), m.ICP_RECORD_DTYPE)
    rc = icp.lib.dvo_icp_align_gated(icp._h, None, len(views), m.DVO_DEPTH_U16, m.DVO_DEPTH_F32, size[0], size[1], m._ptr(K), lists[0], lists[1], lists[2],
                                     m._ptr(Pm), m._ptr(Ps), None, float("nan"), m._ptr(poses2), m._ptr(recs2), 0)
    assert rc == m.DVO_OK and same_bits(poses2, want_poses) and recs2.tobytes() == want.tobytes()
