"""The front end of the frame-to-model alignment on the CPU (include/dvo_amd.h, "preparing a depth frame"): dvo_icp_prepare_host and
dvo_icp_align_gated_host against the numpy restatement (tests/icp_prepare_reference.py) on every size, radius and format, the exact
cases of the filter, the orientation of the normals, what filtering buys on a noisy plane (recorded with the host definition itself),
the Gaussian builder, every refusal, the layout of the mirror, the definition's own code as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/host/icp_prepare_main.cpp) and the C++ mirror (tests/host/icp_prepare_hpp_main.cpp).  No GPU.
Comparisons are byte equality unless a bound is stated."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import icp_prepare_reference as pr
import icp_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["u16", "f32"]
#: the settings of the gated cases: the defaults, and Huber and stop_norm with a level of no sweeps
SETTINGS = [dict(), dict(levels=3, iterations=(2, 0, 3), huber=0.001, stop_norm=1e-3)]


def capi():
    from rgbd_odometry_amd import capi as m
    return m


def c_params(**changes):
    return capi().DvoIcpParams.default(**changes)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_record(rec, want, where):
    assert (int(rec["status"]), int(rec["iterations"]), int(rec["count"]), int(rec["reserved"])) == (want["status"], want["iterations"], want["count"], 0), where
    assert same_bits(np.float64(rec["sum_r2"]), np.float64(want["sum_r2"])) and same_bits(np.float64(rec["rms"]), np.float64(want["rms"])), where
    assert same_bits(np.array(rec["info"]), want["info"]), where


# ---- filter and normals ----

@pytest.mark.parametrize("size", pr.FILTER_SIZES)
def test_host_equals_the_restatement(size):
    """five images per size (clean, holed, all holes, a noisy holed plane, and in f32 one with NaN, inf, negative and zero pixels) at
    every radius in both formats: the filtered image and the normals"""
    K = ir.k4_for(*size)
    normals_seen = 0
    for fmt in FORMATS:
        imgs = pr.filter_inputs(size, fmt)
        if fmt == "f32":
            bad = imgs[4]
            assert np.isnan(bad).any() and np.isinf(bad).any() and (bad < 0.0).any() and (bad == 0.0).any()
        assert all((np.asarray(a) == 0).mean() > 0.04 for a in imgs[1:2]) and not np.any(imgs[2])
        for radius in pr.RADII:
            prm = capi().DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
            fp = pr.from_c(prm)
            out, nrm = capi().icp_prepare_host(imgs, K, prm)
            only = capi().icp_prepare_host(imgs, K, prm, normals=False)
            for i, img in enumerate(imgs):
                F, N = pr.prepare(img, K, fp)
                assert same_bits(out[i], F), (size, fmt, radius, i)
                assert same_bits(nrm[i], N), (size, fmt, radius, i)
                assert same_bits(only[i], F)
                assert np.array_equal(out[i] == 0.0, ir.tr.metres(img)[1]), "a hole stays a hole, and nothing else becomes one"
                normals_seen += int(np.any(N != 0.0, axis=-1).sum())
    assert normals_seen > 0


def test_constant_regions_come_out_exact_and_the_step_is_not_smeared():
    """two constant regions, 1.0 and 1.5 m: every product and sum of the definition is exact and 0.5 m is beyond bin 255, so the output
    is the input bit for bit; no normal on the two columns at the step"""
    rows, cols, step = 19, 23, 11
    img = np.full((rows, cols), 1.0, np.float32)
    img[:, step:] = 1.5
    K = ir.k4_for(rows, cols)
    for radius in (1, 3, 6):
        prm = capi().DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
        assert 0.5 * prm.range_scale >= 256.0 and prm.edge_max < 0.5
        out, nrm = capi().icp_prepare_host([img], K, prm)
        assert same_bits(out[0], img), radius
        have = np.any(nrm[0] != 0.0, axis=-1)
        assert not have[:, step - 1:step + 1].any()
        inner = np.zeros((rows, cols), bool)
        inner[1:-1, 1:-1] = True
        inner[:, step - 1:step + 1] = False
        assert np.array_equal(have, inner)
        assert same_bits(nrm[0], pr.normals_image(out[0], K, prm.edge_max))


def test_range_index_255_is_in_and_256_is_out():
    """depth differences built from range_scale: 255 / 64 m lands in bin 255 exactly, 256 / 64 m is past the table"""
    m = capi()
    prm = m.DvoIcpPrepareParams()
    prm.radius, prm.reserved, prm.range_scale, prm.edge_max = 1, 0, 64.0, 0.05
    for k in range(256):
        prm.range[k] = 3
    prm.range[255] = 1000
    for k in range(9):
        prm.spatial[k] = 1
    near, far = np.float32(1.0 + 255.0 / 64.0), np.float32(1.0 + 256.0 / 64.0)
    assert (float(near) - 1.0) * 64.0 == 255.0 and (float(far) - 1.0) * 64.0 == 256.0
    img = np.array([[near, 1.0, far]], np.float32)
    out = m.icp_prepare_host([img], (1.0, 1.0, 0.0, 0.0), prm, normals=False)[0]
    want = np.float32((1000.0 * float(near) + 3.0 * 1.0) / 1003.0)       # the tap at 255 with its weight, the centre, not the tap at 256
    assert same_bits(out[0, 1], want)
    assert out[0, 1] != np.float32((1000.0 * float(near) + 3.0 + 3.0 * float(far)) / 1006.0)
    assert same_bits(out, pr.filter_image(img, pr.from_c(prm)))
    # the outer pixels see the centre at 255 and 256, and each other far past the table
    assert same_bits(out[0, 0], np.float32((3.0 * float(near) + 1000.0 * 1.0) / 1003.0)) and same_bits(out[0, 2], far)


@pytest.mark.parametrize("scene", ["plane", "corner"])
def test_normals_point_to_the_viewer(scene):
    """clean f32 depth, radius 0: every non-zero normal, rotated to the world, has a positive dot product with the scene's true normal
    of its pixel"""
    m = capi()
    prm = m.DvoIcpPrepareParams.gaussian(0, 2.0, 0.03, 0.05)
    seen = 0
    for size in ir.SIZES:
        K = ir.k4_for(*size)
        for pose in ir.MODEL_POSES.values():
            Z, N = ir.raycast(ir.SCENES[scene], K, pose, *size)
            out, nrm = m.icp_prepare_host([Z.astype(np.float32)], K, prm)
            assert same_bits(out[0], np.where(Z > 0.0, Z, 0.0).astype(np.float32))
            R = pose[:9].reshape(3, 3).T
            world = nrm[0].astype(np.float64) @ R.T
            have = np.any(nrm[0] != 0.0, axis=-1)
            dots = (world * N).sum(axis=-1)[have]
            # at 24 x 32 the side wall and the floor step by more than edge_max from pixel to pixel: under half the pixels have a normal
            assert have.sum() >= 100 and np.all(dots > 0.0), (scene, size, float(dots.min()))
            assert np.allclose(np.linalg.norm(nrm[0][have], axis=-1), 1.0, atol=1e-6)
            seen += int(have.sum())
    assert seen > 0


def test_filtering_a_noisy_plane_improves_its_normals():
    """the slanted plane at 1 m in 16-bit millimetres with seeded noise of +-5 mm: the mean angular error of the normals after the
    default filter is below that of the raw depth, and both are the values recorded in tests/icp_prepare_reference.py"""
    m = capi()
    img, K, true = pr.noisy_plane()
    assert img.shape == (37, 53) and img.dtype == np.uint16
    raw, n_raw = pr.mean_angle_deg(m.icp_prepare_host([img], K, m.DvoIcpPrepareParams.gaussian(0, 2.0, 0.03, 0.05))[1][0], true)
    filtered, n_f = pr.mean_angle_deg(m.icp_prepare_host([img], K, m.DvoIcpPrepareParams.default())[1][0], true)
    print("mean angular error: raw %.12f degrees (%d normals), filtered %.12f degrees (%d normals)" % (raw, n_raw, filtered, n_f))
    assert n_raw == n_f == 35 * 51
    assert filtered < raw
    assert abs(raw - pr.MEASURED_NORMAL_ERRORS_DEG["raw"]) <= 1e-9 and abs(filtered - pr.MEASURED_NORMAL_ERRORS_DEG["filtered"]) <= 1e-9


# ---- the gate ----

def gate_inputs(views, now_fmt, edge_max):
    """the now normals of the views: icp_prepare_host of their now depth with the default tables and `edge_max`"""
    m = capi()
    prm = m.DvoIcpPrepareParams.gaussian(pr.DEFAULT[0], pr.DEFAULT[1], pr.DEFAULT[2], edge_max)
    return m.icp_prepare_host([v["now_" + now_fmt] for v in views], np.array([v["K"] for v in views]), prm)[1]


def host_align(views, now_fmt, model_fmt, now_normals=None, cos_min=0.0, **changes):
    return capi().icp_align_host([v["now_" + now_fmt] for v in views], [v["model_" + model_fmt] for v in views], [v["normals"] for v in views],
                                 np.array([v["K"] for v in views]), np.stack([v["model_pose"] for v in views]),
                                 np.stack([v["start_pose"] for v in views]), c_params(**changes), now_normals=now_normals, normal_cos_min=cos_min)


@pytest.mark.parametrize("size", ir.SIZES)
def test_gated_host_equals_the_restatement(size):
    """good_views of the size with now normals from icp_prepare_host, normal_cos_min 0.9, in the default setting and one with Huber
    weights, stop_norm and a level of no sweeps: poses and records in bits.  At the start pose the cosine test proper rejects pairs, and
    the gated record counts fewer pixels than the ungated one"""
    views = ir.good_views(size)
    statuses = []
    for now_fmt, model_fmt in (("u16", "u16"), ("f32", "u16")):
        gate = gate_inputs(views, now_fmt, pr.GATE_EDGE_MAX[size])
        p0 = ir.params()
        rejected = [int(pr.gated_terms(v, now_fmt, model_fmt, v["start_pose"][:9], v["start_pose"][9:], 0, p0, g, pr.COS_MIN)[2].sum())
                    for v, g in zip(views, gate)]
        with_normal = [int(np.any(g != 0.0, axis=-1).sum()) for g in gate]
        print("%s %s/%s: pairs rejected by the cosine test at the start pose %s, now pixels with a normal %s of %d" %
              (size, now_fmt, model_fmt, rejected, with_normal, size[0] * size[1]))
        assert sum(rejected) >= 1 and rejected[0] >= 1, (size, rejected)
        for setting in SETTINGS:
            p = ir.params(**setting)
            poses, recs = host_align(views, now_fmt, model_fmt, gate, pr.COS_MIN, **setting)
            _, open_recs = host_align(views, now_fmt, model_fmt, **setting)
            for i, v in enumerate(views):
                where = (size, setting, now_fmt, model_fmt, i)
                want_pose, want = pr.align_view_gated(v, now_fmt, model_fmt, p, gate[i], pr.COS_MIN)
                assert same_bits(poses[i], want_pose), where
                assert_record(recs[i], want, where)
                assert int(recs[i]["count"]) < int(open_recs[i]["count"]), where
                statuses.append(want["status"])
    # at 24 x 32 level 2 is a list of 6 x 8 pixels, few of them with a normal: some views stop there.  The larger sizes run through
    print("%s: statuses %s" % (size, statuses))
    assert ir.OK in statuses and (size == ir.SIZES[0] or all(s == ir.OK for s in statuses))


def test_the_restatement_without_normals_is_icp_reference():
    v = ir.good_views(ir.SIZES[0])[1]
    p = ir.params()
    a, b = pr.align_view_gated(v, "u16", "f32", p, None, 0.9), ir.align_view(v, "u16", "f32", p)
    assert same_bits(a[0], b[0]) and a[1]["count"] == b[1]["count"] and same_bits(a[1]["info"], b[1]["info"])


def test_a_null_list_is_the_ungated_call():
    """dvo_icp_align_gated_host with now_normals NULL: the bytes of dvo_icp_align_host, normal_cos_min ignored (even a NaN)"""
    m = capi()
    lib = m.load_library()
    views = ir.good_views(ir.SIZES[1]) + ir.stopping_views(ir.SIZES[1])
    n = len(views)
    want_poses, want = host_align(views, "u16", "f32")
    lists = [(C.c_void_p * n)(*[np.ascontiguousarray(v[k]).ctypes.data for v in views]) for k in ("now_u16", "model_f32", "normals")]
    K, Pm, Ps = np.array([v["K"] for v in views]), np.stack([v["model_pose"] for v in views]), np.stack([v["start_pose"] for v in views])
    rows, cols = ir.SIZES[1]
    for cos_min in (0.0, 0.9, 7.0, float("nan")):
        poses, recs = np.zeros((n, 12)), np.zeros(n, m.ICP_RECORD_DTYPE)
        rc = lib.dvo_icp_align_gated_host(C.byref(c_params()), n, m.DVO_DEPTH_U16, m.DVO_DEPTH_F32, rows, cols, m._ptr(K), lists[0], lists[1], lists[2],
                                          m._ptr(Pm), m._ptr(Ps), None, cos_min, m._ptr(poses), m._ptr(recs))
        assert rc == m.DVO_OK and same_bits(poses, want_poses) and recs.tobytes() == want.tobytes(), cos_min


# ---- the Gaussian builder, the constants, the layout ----

def test_gaussian_builder():
    m = capi()
    for radius, ss, sr, edge in (pr.DEFAULT, (6, 3.5, 0.01, 0.02), (0, 1.0, 0.1, 1.0), (1, 0.5, 0.004, 0.3), (6, 0.7, 0.05, 0.05)):
        prm = m.DvoIcpPrepareParams.gaussian(radius, ss, sr, edge)
        want = pr.gaussian(radius, ss, sr, edge)
        assert (prm.radius, prm.reserved, prm.edge_max) == (radius, 0, edge)
        assert same_bits(np.float64(prm.range_scale), np.float64(256.0 / (3.0 * sr)))
        sp = prm.spatial_table().astype(np.int64)
        rng = np.array(prm.range[:], np.int64)
        assert sp[radius, radius] == 255
        assert np.array_equal(sp, sp.T) and np.array_equal(sp, sp[::-1]) and np.array_equal(sp, sp[:, ::-1])
        dist = sorted((dx * dx + dy * dy, int(sp[dy + radius, dx + radius])) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1))
        by_distance = {}
        for d2, w in dist:
            by_distance.setdefault(d2, set()).add(w)
        assert all(len(ws) == 1 for ws in by_distance.values())
        values = [ws.pop() for _, ws in sorted(by_distance.items())]
        assert all(a >= b for a, b in zip(values, values[1:]))
        assert np.all(np.diff(rng) <= 0) and rng[0] >= 1
        assert np.abs(sp - want["spatial"].astype(np.int64)).max() <= 1
        assert np.abs(rng - want["range"].astype(np.int64)).max() <= 1
        assert not any(prm.spatial[(2 * radius + 1) ** 2:])
    d = m.DvoIcpPrepareParams.default()
    assert bytes(d) == bytes(m.DvoIcpPrepareParams.gaussian(*pr.DEFAULT))
    assert (d.radius, d.edge_max) == (3, 0.05) and math.isclose(d.range_scale, 256.0 / 0.09)
    lib = m.load_library()
    assert lib.dvo_icp_prepare_params_default(None) == m.DVO_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    blank = m.DvoIcpPrepareParams()
    C.memset(C.byref(blank), 0x5A, C.sizeof(blank))
    before = bytes(blank)
    for args in ((-1, 2.0, 0.03, 0.05), (7, 2.0, 0.03, 0.05), (3, 0.0, 0.03, 0.05), (3, -2.0, 0.03, 0.05), (3, nan, 0.03, 0.05), (3, inf, 0.03, 0.05),
                 (3, 2.0, 0.0, 0.05), (3, 2.0, -0.03, 0.05), (3, 2.0, nan, 0.05), (3, 2.0, inf, 0.05), (3, 2.0, 0.03, 0.0), (3, 2.0, 0.03, -1.0),
                 (3, 2.0, 0.03, nan), (3, 2.0, 0.03, inf)):
        assert lib.dvo_icp_prepare_params_gaussian(args[0], args[1], args[2], args[3], C.byref(blank)) == m.DVO_ERR_INVALID, args
        assert bytes(blank) == before, args
        with pytest.raises(m.DvoError):
            m.DvoIcpPrepareParams.gaussian(*args)
    assert lib.dvo_icp_prepare_params_gaussian(3, 2.0, 0.03, 0.05, None) == m.DVO_ERR_INVALID


def test_constants_and_symbols():
    m = capi()
    lib = m.load_library()
    strip = lambda src: re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    text = strip(open(os.path.join(ROOT, "include", "dvo_amd.h")).read())
    own = strip(open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_icp_prepare.h")).read())
    for name, value in (("DVO_ICP_PREPARE_MAX_RADIUS", m.DVO_ICP_PREPARE_MAX_RADIUS), ("DVO_ICP_PREPARE_RANGE_BINS", m.DVO_ICP_PREPARE_RANGE_BINS)):
        for src in (text, own):
            assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == value, name
    assert int(re.search(r"#define\s+DVO_ICP_PREPARE_LAUNCHES\s+(\d+)", text).group(1)) == m.DVO_ICP_PREPARE_LAUNCHES == 2
    launch = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_icp_prepare_launch.h")).read()
    assert int(re.search(r"kPrepareLaunches\s*=\s*(\d+)", launch).group(1)) == m.DVO_ICP_PREPARE_LAUNCHES
    block = lambda src: re.search(r"#ifndef DVO_ICP_PREPARE_TYPES_DEFINED_(.*?)#endif", src, flags=re.S).group(1).split()
    assert block(text) == block(own)
    for name in ("dvo_icp_prepare_params_default", "dvo_icp_prepare_params_gaussian", "dvo_icp_prepare_host", "dvo_icp_prepare", "dvo_icp_align_gated_host",
                 "dvo_icp_align_gated"):
        assert name in m.C_ABI_SYMBOLS and hasattr(lib, name)
    # the two lists of what is out of scope no longer name what this front end does
    for path, section in ((os.path.join(ROOT, "include", "dvo_amd.h"), "---- frame-to-model alignment"),
                          (os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_icp.h"), "dvo_icp.h --")):
        scope = re.search(r"OUT OF SCOPE:(.*?)\*/", open(path).read().split(section, 1)[1], flags=re.S).group(1)
        assert "bilateral" not in scope and "normals of the now frame" not in scope and "pyramid" in scope and "damping" in scope


def test_struct_layout_matches_header(tmp_path):
    """the ctypes mirror must have the layout the C compiler gives dvo_icp_prepare_params"""
    m = capi()
    fields = ["radius", "reserved", "range_scale", "edge_max", "range", "spatial"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu' + " %zu" * len(fields) + '", '
                   "sizeof(dvo_icp_prepare_params), " + ", ".join("offsetof(dvo_icp_prepare_params, %s)" % f for f in fields) + ");return 0;}")
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    P = m.DvoIcpPrepareParams
    assert [C.sizeof(P)] + [getattr(P, f).offset for f in fields] == got
    assert got[0] == 712 and P.range.size == 512 and P.spatial.size == 169


# ---- refusals ----

def test_prepare_refusals_write_nothing():
    m = capi()
    lib = m.load_library()
    rows, cols = ir.SIZES[0]
    imgs = [np.ascontiguousarray(a) for a in pr.filter_inputs(ir.SIZES[0], "u16")[:2]]
    out = [np.full((rows, cols), -7.5, np.float32) for _ in range(2)]
    nrm = [np.full((rows, cols, 3), -7.5, np.float32) for _ in range(2)]
    lists = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    half = lambda arrs: (C.c_void_p * 2)(arrs[0].ctypes.data, None)
    K = np.array([ir.k4_for(rows, cols)] * 2)
    prm = m.DvoIcpPrepareParams.default()

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

    def raw(p=prm, count=2, fmt=m.DVO_DEPTH_U16, r=rows, c=cols, k=K, d=lists(imgs), o=lists(out), q=lists(nrm)):
        return lib.dvo_icp_prepare_host(None if p is None else C.byref(p), count, fmt, r, c, None if k is None else m._ptr(k), d, o, q)

    def untouched():
        return all(np.all(a == -7.5) for a in out + nrm)

    nan, inf = float("nan"), float("inf")
    bad = [dict(p=None), dict(k=None), dict(d=None), dict(o=None), dict(d=half(imgs)), dict(o=half(out)), dict(q=half(nrm)), dict(count=0), dict(count=-2),
           dict(r=0), dict(c=0), dict(c=-3), dict(r=4097, c=4096), dict(fmt=2), dict(fmt=-1)]
    bad += [dict(p=changed(**kw)) for kw in (dict(radius=-1), dict(radius=7), dict(reserved=1), dict(range_scale=0.0), dict(range_scale=-1.0),
                                              dict(range_scale=nan), dict(range_scale=inf), dict(edge_max=0.0), dict(edge_max=-0.05), dict(edge_max=nan),
                                              dict(edge_max=inf), dict(range0=0), dict(centre=0))]
    for j in range(4):
        for value in (nan, inf):
            Kb = K.copy()
            Kb[1, j] = value
            bad.append(dict(k=Kb))
    bad += [dict(k=np.array([[30.0, 30.0, 15.5, 11.5], [0.0, 30.0, 15.5, 11.5]])), dict(k=np.array([[30.0, -1.0, 15.5, 11.5], [30.0, 30.0, 15.5, 11.5]]))]
    for kw in bad:
        assert raw(**kw) == m.DVO_ERR_INVALID, kw
        assert untouched(), kw
    # a radius whose centre weight lies elsewhere in the table: the check follows the radius
    assert raw(p=changed(radius=2)) == m.DVO_OK
    for a in out + nrm:
        a[...] = -7.5
    assert raw(q=None) == m.DVO_OK and all(np.all(a == -7.5) for a in nrm) and not any(np.any(a == -7.5) for a in out)
    assert raw() == m.DVO_OK and not any(np.all(a == -7.5) for a in nrm)
    want, want_n = m.icp_prepare_host(imgs, K[0])
    assert all(same_bits(a, b) for a, b in zip(out + nrm, want + want_n))
    # the handle's entry points without a handle
    assert lib.dvo_icp_prepare(None, None, 1, 0, 1, 1, None, None, None, None, 0) == m.DVO_ERR_INVALID
    assert lib.dvo_icp_align_gated(None, None, 1, 0, 0, 1, 1, None, None, None, None, None, None, None, 0.0, None, None, 0) == m.DVO_ERR_INVALID


def test_gated_refusals_write_nothing():
    """with a list of now normals: a NULL entry, a normal_cos_min that is not finite or outside [-1, 1] -- and what the ungated call
    refuses; -1 and 1 themselves are taken"""
    m = capi()
    lib = m.load_library()
    views = ir.good_views(ir.SIZES[0])[:2]
    rows, cols = ir.SIZES[0]
    keep = [[np.ascontiguousarray(v[k]) for v in views] for k in ("now_u16", "model_u16", "normals")]
    gate = [np.ascontiguousarray(g) for g in gate_inputs(views, "u16", 0.05)]
    lists = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    K, Pm, Ps = np.array([v["K"] for v in views]), np.stack([v["model_pose"] for v in views]), np.stack([v["start_pose"] for v in views])
    poses = np.full((2, 12), -7.5)
    recs = np.zeros(2, m.ICP_RECORD_DTYPE)
    recs.view(np.uint8)[:] = 0x5A

    def raw(p=c_params(), count=2, g=lists(gate), cos_min=0.9, k=K, n=lists(keep[0])):
        return lib.dvo_icp_align_gated_host(C.byref(p), count, m.DVO_DEPTH_U16, m.DVO_DEPTH_U16, rows, cols, m._ptr(k), n, lists(keep[1]), lists(keep[2]),
                                            m._ptr(Pm), m._ptr(Ps), g, cos_min, m._ptr(poses), m._ptr(recs))

    untouched = lambda: np.all(poses == -7.5) and np.all(recs.view(np.uint8) == 0x5A)
    Kb = K.copy()
    Kb[0, 0] = 0.0
    for kw in (dict(g=(C.c_void_p * 2)(gate[0].ctypes.data, None)), dict(g=(C.c_void_p * 2)(None, gate[1].ctypes.data)), dict(cos_min=float("nan")),
               dict(cos_min=float("inf")), dict(cos_min=-float("inf")), dict(cos_min=1.0000001), dict(cos_min=-1.5), dict(count=0), dict(p=c_params(levels=0)),
               dict(k=Kb), dict(n=(C.c_void_p * 2)(keep[0][0].ctypes.data, None))):
        assert raw(**kw) == m.DVO_ERR_INVALID, kw
        assert untouched(), kw
    for cos_min in (-1.0, 1.0, 0.9):
        assert raw(cos_min=cos_min) == m.DVO_OK and not untouched()
    want_poses, want = host_align(views, "u16", "u16", gate, 0.9)
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()


def test_inputs_are_not_modified():
    views = ir.good_views(ir.SIZES[1])
    gate = gate_inputs(views, "f32", 0.05)
    before = [g.copy() for g in gate] + [v["now_f32"].copy() for v in views]
    host_align(views, "f32", "u16", gate, 0.9)
    assert all(same_bits(a, b) for a, b in zip(gate + [v["now_f32"] for v in views], before))


# ---- the definition's own code under sanitizers, and the C++ mirror ----

def write_case(d, views, now_fmt, model_fmt, fp, prm):
    paths = {k: str(d / (k + ".bin")) for k in ("prepare", "params", "views")}
    open(paths["prepare"], "wb").write(bytes(fp))
    open(paths["params"], "wb").write(bytes(prm))
    with open(paths["views"], "wb") as f:
        f.write(np.array([v["K"] for v in views], np.float64).tobytes())
        f.write(np.stack([v["model_pose"] for v in views]).astype(np.float64).tobytes())
        f.write(np.stack([v["start_pose"] for v in views]).astype(np.float64).tobytes())
        for v in views:
            f.write(np.ascontiguousarray(v["now_" + now_fmt]).tobytes())
            f.write(np.ascontiguousarray(v["model_" + model_fmt]).tobytes())
            f.write(np.ascontiguousarray(v["normals"]).tobytes())
    return paths


def parse_output(stdout, count, rows, cols):
    m = capi()
    lines = stdout.splitlines()
    assert [lines[k].split() for k in (0, 2, 4, 6)] == [[name, str(count)] for name in ("depth", "normals", "poses", "records")]
    depth = np.frombuffer(bytes.fromhex(lines[1]), np.float32).reshape(count, rows, cols)
    normals = np.frombuffer(bytes.fromhex(lines[3]), np.float32).reshape(count, rows, cols, 3)
    poses = np.frombuffer(bytes.fromhex(lines[5]), ">u8").astype(np.uint64).view(np.float64).reshape(count, 12)
    recs = np.frombuffer(bytes.fromhex(lines[7]), m.ICP_RECORD_DTYPE)
    return depth, normals, poses, recs, lines[8:]


def code_of(fmt):
    m = capi()
    return {"u16": m.DVO_DEPTH_U16, "f32": m.DVO_DEPTH_F32}.get(fmt, fmt)


def bits_of(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def program_args(paths, now_fmt, model_fmt, rows, cols, count, cos_min):
    return [paths["prepare"], paths["params"], paths["views"], str(code_of(now_fmt)), str(code_of(model_fmt)), str(rows), str(cols), str(count), bits_of(cos_min)]


def expected(views, now_fmt, model_fmt, fp, cos_min, **setting):
    m = capi()
    F, N = m.icp_prepare_host([v["now_" + now_fmt] for v in views], np.array([v["K"] for v in views]), fp)
    poses, recs = host_align(views, now_fmt, model_fmt, N, cos_min, **setting)
    return np.stack(F), np.stack(N), poses, recs


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("icp_prepare")
    exe = str(d / "icp_prepare_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "icp_prepare_main.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/icp_prepare_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


#: 5 x 13 with radius 6 (the window is larger than the image); 16 x 64 and 32 x 128: the last row and column end a tile of the device's
#: filter kernel; 17 x 65: they begin one
PROGRAM_CASES = [((5, 13), 6, "u16", "f32"), ((16, 64), 3, "f32", "f32"), ((32, 128), 1, "u16", "u16"), ((17, 65), 6, "f32", "u16"), (ir.SIZES[1], 3, "u16", "u16")]


@pytest.mark.parametrize("size,radius,now_fmt,model_fmt", PROGRAM_CASES)
def test_definition_under_sanitizers(host_program, size, radius, now_fmt, model_fmt):
    """the same code the library compiles, with every buffer allocated to its exact size: the library's bytes, clean under
    -fsanitize=address,undefined"""
    m = capi()
    d, exe = host_program
    rows, cols = size
    views = ir.good_views(size) + ir.stopping_views(size)
    fp = m.DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
    paths = write_case(d, views, now_fmt, model_fmt, fp, c_params(**SETTINGS[1]))
    run = subprocess.run([exe] + program_args(paths, now_fmt, model_fmt, rows, cols, len(views), pr.COS_MIN), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    depth, normals, poses, recs, rest = parse_output(run.stdout, len(views), rows, cols)
    F, N, want_poses, want = expected(views, now_fmt, model_fmt, fp, pr.COS_MIN, **SETTINGS[1])
    assert rest == [] and same_bits(depth, F) and same_bits(normals, N)
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()


def test_program_refuses_what_the_definition_refuses(host_program):
    m = capi()
    d, exe = host_program
    rows, cols = ir.SIZES[0]
    views = ir.good_views(ir.SIZES[0])[:1]
    good = m.DvoIcpPrepareParams.default()
    broken = m.DvoIcpPrepareParams.default()
    broken.radius = 9
    for fp, prm, cos_min, count, refused in ((good, c_params(), 0.9, 1, False), (broken, c_params(), 0.9, 1, True), (good, c_params(levels=0), 0.9, 1, True),
                                             (good, c_params(), 1.5, 1, True), (good, c_params(), float("nan"), 1, True), (good, c_params(), 0.9, 0, True)):
        paths = write_case(d, views, "u16", "u16", fp, prm)
        run = subprocess.run([exe] + program_args(paths, "u16", "u16", rows, cols, count, cos_min), capture_output=True, text=True, timeout=300)
        assert run.returncode == (3 if refused else 0), run.stdout[-500:] + run.stderr[-4000:]
        assert not refused or run.stdout.strip() == "refused"


def test_cpp_mirror(tmp_path):
    """include/dvo_amd.hpp's icpPrepareHost, the now normals of IcpViews and IcpAligner::prepare: tests/host/icp_prepare_hpp_main.cpp
    compiles with plain g++ and every warning on and links against the library; the host functions give the library's bytes, and on two
    cases the device is asked too: the same bytes where there is one, a loud refusal where there is none"""
    import torch
    m = capi()
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "icp_prepare_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "icp_prepare_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    for size, radius, now_fmt, model_fmt, setting, on_device in ((ir.SIZES[0], 3, "u16", "u16", SETTINGS[0], False), ((17, 65), 6, "f32", "u16", SETTINGS[1], True),
                                                                  (ir.SIZES[2], 3, "u16", "f32", SETTINGS[0], True)):
        views = ir.good_views(size) + ir.stopping_views(size)
        rows, cols = size
        fp = m.DvoIcpPrepareParams.gaussian(radius, 2.0, 0.03, 0.05)
        paths = write_case(tmp_path, views, now_fmt, model_fmt, fp, c_params(**setting))
        run = subprocess.run([exe] + program_args(paths, now_fmt, model_fmt, rows, cols, len(views), pr.COS_MIN) + (["device"] if on_device else []),
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        depth, normals, poses, recs, rest = parse_output(run.stdout, len(views), rows, cols)
        F, N, want_poses, want = expected(views, now_fmt, model_fmt, fp, pr.COS_MIN, **setting)
        assert same_bits(depth, F) and same_bits(normals, N) and same_bits(poses, want_poses) and recs.tobytes() == want.tobytes(), size
        if not on_device:
            assert rest == []
        elif torch.cuda.is_available():
            assert rest[0] == "device equal 1", (size, rest)
        else:
            assert rest[0].startswith("device none") and "no CPU fallback" in rest[0]
    broken = m.DvoIcpPrepareParams.default()
    broken.reserved = 4
    views = ir.good_views(ir.SIZES[0])[:1]
    paths = write_case(tmp_path, views, "u16", "u16", broken, c_params())
    run = subprocess.run([exe] + program_args(paths, "u16", "u16", 24, 32, 1, 0.9), capture_output=True, text=True, timeout=120)
    assert run.returncode == 3 and run.stdout.strip() == "refused"
