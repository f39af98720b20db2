"""Frame-to-model alignment on the CPU (include/dvo_amd.h, "frame-to-model alignment"): dvo_icp_align_host against the numpy restatement
of the definition (tests/icp_reference.py) on every size, view, format and setting, the sum order, the two ways a view stops, every
refusal, convergence against floors measured with the host definition itself, the layout of the mirrors, the definition's own code
(rgbd_odometry_amd/csrc/dvo_icp.h) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/host/icp_main.cpp) and the C++ mirror (tests/host/icp_hpp_main.cpp).  No GPU.  Comparisons are byte equality unless a bound is
stated."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import icp_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["u16", "f32"]
#: the settings of the byte-equality cases: the defaults, Huber weights on, stop_norm on, and one level alone
SETTINGS = [dict(), dict(huber=0.0005), dict(stop_norm=2e-3), dict(levels=1, iterations=(6,)), dict(levels=3, iterations=(2, 0, 3), huber=0.001, stop_norm=1e-3)]


def c_params(**changes):
    from rgbd_odometry_amd import capi
    return capi.DvoIcpParams.default(**changes)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(views, now_fmt, model_fmt, **changes):
    from rgbd_odometry_amd import capi
    return capi.icp_align_host([v["now_" + now_fmt] for v in views], [v["model_" + model_fmt] for v in views], [v["normals"] for v in views],
                               np.array([v["K"] for v in views]), np.stack([v["model_pose"] for v in views]),
                               np.stack([v["start_pose"] for v in views]), c_params(**changes))


def assert_record(rec, want, where):
    assert (int(rec["status"]), int(rec["iterations"]), int(rec["count"]), int(rec["reserved"])) == (want["status"], want["iterations"], want["count"], 0), where
    assert same_bits(np.float64(rec["sum_r2"]), np.float64(want["sum_r2"])) and same_bits(np.float64(rec["rms"]), np.float64(want["rms"])), where
    assert same_bits(np.array(rec["info"]), want["info"]), where


@pytest.mark.parametrize("size", ir.SIZES)
def test_host_equals_the_restatement(size):
    """every view of the size -- three corner views, the plane, the frame of holes -- in both formats and one mixed pair, in every setting"""
    views = ir.good_views(size) + ir.stopping_views(size)
    updates, early = 0, 0
    for setting in SETTINGS:
        p = ir.params(**setting)
        for now_fmt, model_fmt in (("u16", "u16"), ("f32", "f32"), ("u16", "f32")):
            poses, recs = host(views, now_fmt, model_fmt, **setting)
            for i, v in enumerate(views):
                where = (size, setting, now_fmt, model_fmt, i)
                want_pose, want = ir.align_view(v, now_fmt, model_fmt, p)
                assert same_bits(poses[i], want_pose), where
                assert_record(recs[i], want, where)
                updates += want["iterations"]
                early += want["status"] == ir.OK and want["iterations"] < sum(p["iterations"][:p["levels"]])
    print("%s: %d updates in all, %d alignments ended a level early through stop_norm" % (size, updates, early))
    assert updates > 0 and early > 0


PAIRS = (("u16", "u16"), ("f32", "f32"), ("u16", "f32"))


def check_against_the_restatement(views, pairs, setting):
    """every view in every format pair, in bits; returns the restatement's records of the last pair, each with its "pose" added"""
    p = ir.params(**setting)
    for now_fmt, model_fmt in pairs:
        poses, recs = host(views, now_fmt, model_fmt, **setting)
        wanted = []
        for i, v in enumerate(views):
            where = (v["rows"], v["cols"], setting, now_fmt, model_fmt, i)
            want_pose, want = ir.align_view(v, now_fmt, model_fmt, p)
            assert same_bits(poses[i], want_pose), where
            assert_record(recs[i], want, where)
            wanted.append(dict(want, pose=want_pose))
    return wanted


@pytest.mark.parametrize("size", ir.TREE_SIZES)
def test_host_equals_the_restatement_at_the_tree_boundaries(size):
    """the list lengths on both sides of every branch of the sum tree -- 64 / 65, 4096 / 4100, 2^18 / 2^18 + 1: TreeSum's rounds 3 and 4
    and the path of finish() through them against tree_sum, which pads and reshapes for any length.  The two large sizes also with
    stop_norm on, in the mixed format pair"""
    views = ir.good_views(size) + ir.stopping_views(size) + [ir.tail_view(size)]
    entries = size[0] * size[1]
    assert entries in (64, 65, 4096, 4100, 1 << 18, (1 << 18) + 1)
    want = check_against_the_restatement(views, PAIRS, ir.TREE_SETTING)
    assert [w["status"] for w in want] == [ir.OK, ir.OK, ir.OK, ir.DEGENERATE, ir.FEW, ir.OK], size
    assert [w["iterations"] for w in want] == [4, 4, 4, 0, 0, 4], size
    # the entries behind the boundary -- the last run of 64, which is the whole last workgroup and the whole last group at 65, 4100 and
    # 2^18 + 1 -- take part in the last view's record: a sum that loses them is another one.  (At 481 x 545 the last entry of every
    # other view is skipped once the pose is near the true one: its point has left the model image)
    v, p, pose = views[-1], ir.params(**ir.TREE_SETTING), want[-1]["pose"]
    assert PAIRS[-1] == ("u16", "f32")
    assert ir.terms(v, "u16", "f32", pose[:9], pose[9:], 0, p)[1][-(entries % 64 or 64):].sum() >= min(entries % 64 or 64, 4), size
    if entries >= 1 << 18:
        setting = dict(ir.TREE_SETTING, stop_norm=2e-3)
        want = check_against_the_restatement(views, PAIRS[2:], setting)
        assert [w["status"] for w in want] == [ir.OK, ir.OK, ir.OK, ir.DEGENERATE, ir.FEW, ir.OK], size
        print("%s with stop_norm: updates %s" % (size, [w["iterations"] for w in want]))
        assert all(1 <= w["iterations"] for w in want[:3]) and any(w["iterations"] < 4 for w in want[:3]), size


@pytest.mark.parametrize("size,setting", ir.LEVEL3_CASES)
def test_level_3(size, setting):
    """levels = DVO_ICP_MAX_LEVELS: the sub-grid of every eighth pixel, ceil(cols / 8) per row.  Every OK view applied every update of
    every level, so level 3's sweeps ran"""
    from rgbd_odometry_amd import capi
    assert setting["levels"] == capi.DVO_ICP_MAX_LEVELS == 4 and setting["iterations"][3] > 0
    views = ir.good_views(size) + ir.stopping_views(size)
    want = check_against_the_restatement(views, PAIRS if size != ir.TREE_TOP else PAIRS[2:], setting)
    assert [w["status"] for w in want] == [ir.OK, ir.OK, ir.OK, ir.DEGENERATE, ir.FEW], size
    assert [w["iterations"] for w in want[:3]] == [sum(setting["iterations"])] * 3, size
    # level 3's sweeps are part of the result: without them the pose is another one
    without = dict(setting, iterations=setting["iterations"][:3] + (0,))
    for v in views[:1]:
        assert not same_bits(ir.align_view(v, "u16", "f32", ir.params(**setting))[0], ir.align_view(v, "u16", "f32", ir.params(**without))[0])


def sum_order_in_the_upper_rounds():
    """481 x 545, 65 sweep workgroups: the tree against NOT the definition -- the tree inside each run of 4096 entries, the 65 results
    added one after the other.  The sums and the pose after updates differ in their bits, and the library agrees with the tree: byte
    equality against it notices a wrong association in the third or the fourth round"""
    v = ir.wide_range_view(size=ir.TREE_TOP)
    p = ir.params(levels=1, iterations=(0,))
    for view, least in ((v, 14), (ir.good_views(ir.TREE_TOP)[0], 14)):
        out, ok = ir.terms(view, "f32", "f32", view["start_pose"][:9], view["start_pose"][9:], 0, p)
        tree, grouped = ir.tree_sum(out), ir.grouped_sum(out)
        assert ok.sum() > 100000 and np.all(np.isfinite(tree))
        differ = int((tree.view(np.uint64) != grouped.view(np.uint64)).sum())
        print("%d of 28 sums differ in their bits between the tree and the grouped order" % differ)
        assert differ >= least
        assert np.allclose(tree, grouped, rtol=1e-9, atol=0.0)
    _, want = ir.align_view(v, "f32", "f32", p)
    _, other = ir.align_view(v, "f32", "f32", p, total=ir.grouped_sum)
    poses, recs = host([v], "f32", "f32", levels=1, iterations=(0,))
    assert_record(recs[0], want, "record")
    assert not same_bits(np.array(recs[0]["info"]), other["info"])
    assert same_bits(poses[0], v["start_pose"])
    p3 = ir.params(levels=1, iterations=(3,), min_pivot_ratio=1e-30)
    want_pose, want = ir.align_view(v, "f32", "f32", p3)
    other_pose, _ = ir.align_view(v, "f32", "f32", p3, total=ir.grouped_sum)
    poses, recs = host([v], "f32", "f32", levels=1, iterations=(3,), min_pivot_ratio=1e-30)
    assert want["iterations"] == 3 and not same_bits(want_pose, other_pose)
    assert same_bits(poses[0], want_pose) and not same_bits(poses[0], other_pose)
    assert_record(recs[0], want, "after updates")


def test_sum_order_in_the_fourth_round():
    """724 x 725: three values in the fourth round, the fewest whose order shows (at 481 x 545 it adds two, and
    fourth_round_raster_sum has the tree's bits: asserted).  The library agrees with the tree and not with NOT the definition -- three
    rounds of the tree, then the three results one after the other"""
    p = ir.params(levels=1, iterations=(0,))
    differ = {}
    for size in (ir.TREE_TOP, ir.TREE_DEEP):
        v = ir.wide_range_view(size=size)
        out, ok = ir.terms(v, "f32", "f32", v["start_pose"][:9], v["start_pose"][9:], 0, p)
        tree, other = ir.tree_sum(out), ir.fourth_round_raster_sum(out)
        differ[size] = int((tree.view(np.uint64) != other.view(np.uint64)).sum())
        assert np.all(np.isfinite(tree)) and ok[-1] and -(-len(out) // (1 << 18)) == (2 if size == ir.TREE_TOP else 3)
    print("sums that differ in their bits between the tree and a fourth round in raster order: %s" % differ)
    assert differ[ir.TREE_TOP] == 0 and differ[ir.TREE_DEEP] >= 3
    _, want = ir.align_view(v, "f32", "f32", p)
    _, other = ir.align_view(v, "f32", "f32", p, total=ir.fourth_round_raster_sum)
    poses, recs = host([v], "f32", "f32", levels=1, iterations=(0,))
    assert_record(recs[0], want, "record")
    assert not same_bits(np.array(recs[0]["info"]), other["info"])


def test_sum_order():
    """terms of widely different magnitude: the restatement's tree and a raster-order sum of the same terms give different bits, and the
    library agrees with the tree -- in the record of an alignment without updates, and in the pose after updates.  Then the same at
    481 x 545 against a sum that is wrong in the upper rounds only (sum_order_in_the_upper_rounds)"""
    v = ir.wide_range_view()
    p = ir.params(levels=1, iterations=(0,))
    out, ok = ir.terms(v, "f32", "f32", v["start_pose"][:9], v["start_pose"][9:], 0, p)
    tree, raster = ir.tree_sum(out), ir.raster_sum(out)
    assert ok.sum() > 500 and np.all(np.isfinite(tree))
    differ = int((tree.view(np.uint64) != raster.view(np.uint64)).sum())
    print("%d of 28 sums differ in their bits between the tree and the raster order" % differ)
    assert differ >= 14
    assert np.allclose(tree, raster, rtol=1e-9, atol=0.0)
    _, want = ir.align_view(v, "f32", "f32", p)
    _, other = ir.align_view(v, "f32", "f32", p, total=ir.raster_sum)
    poses, recs = host([v], "f32", "f32", levels=1, iterations=(0,))
    assert_record(recs[0], want, "record")
    assert not same_bits(np.array(recs[0]["info"]), other["info"])
    assert same_bits(poses[0], v["start_pose"])
    # with updates the pose itself depends on the order of the sums
    p3 = ir.params(levels=1, iterations=(3,), min_pivot_ratio=1e-30)
    want_pose, want = ir.align_view(v, "f32", "f32", p3)
    other_pose, _ = ir.align_view(v, "f32", "f32", p3, total=ir.raster_sum)
    poses, recs = host([v], "f32", "f32", levels=1, iterations=(3,), min_pivot_ratio=1e-30)
    assert want["iterations"] == 3 and not same_bits(want_pose, other_pose)
    assert same_bits(poses[0], want_pose)
    assert_record(recs[0], want, "after updates")
    sum_order_in_the_upper_rounds()


@pytest.mark.parametrize("fmt", FORMATS)
def test_plane_is_degenerate_and_holes_are_few(fmt):
    from rgbd_odometry_amd import capi
    for size in ir.SIZES:
        plane, holes = ir.stopping_views(size)
        poses, recs = host([plane, holes], fmt, fmt)
        assert recs[0]["status"] == capi.DVO_ICP_DEGENERATE == ir.DEGENERATE and recs[0]["iterations"] == 0
        assert recs[0]["count"] >= 6 and recs[0]["sum_r2"] > 0.0 and np.any(recs[0]["info"] != 0.0)
        assert same_bits(poses[0], plane["start_pose"])
        assert recs[1]["status"] == capi.DVO_ICP_FEW == ir.FEW and (recs[1]["iterations"], recs[1]["count"]) == (0, 0)
        assert recs[1]["sum_r2"] == 0.0 and recs[1]["rms"] == 0.0 and not np.any(recs[1]["info"])
        assert same_bits(poses[1], holes["start_pose"])
    # min_count above what a level's list holds (12 x 16 at level 1 of 24 x 32): FEW with a count that is not zero
    v = ir.good_views(ir.SIZES[0])[0]
    poses, recs = host([v], fmt, fmt, levels=2, iterations=(3, 2), min_count=12 * 16 + 1)
    assert recs[0]["status"] == capi.DVO_ICP_FEW and recs[0]["iterations"] == 0 and 100 < recs[0]["count"] <= 12 * 16
    assert same_bits(poses[0], v["start_pose"])


@pytest.mark.parametrize("fmt", FORMATS)
def test_convergence(fmt):
    """the clean corner, started at the model's pose: both errors end strictly below where they started and below twice the floor the
    host definition reached when icp_reference.MEASURED_FINAL_ERRORS was recorded"""
    v = ir.convergence_view()
    rot0, trans0 = ir.pose_errors(v["start_pose"], v["true_pose"])
    poses, recs = host([v], fmt, fmt)
    rot, trans = ir.pose_errors(poses[0], v["true_pose"])
    floor_rot, floor_trans = ir.MEASURED_FINAL_ERRORS[fmt]
    print("%s: rotation %.6e -> %.6e rad (recorded %.6e), translation %.6e -> %.6e m (recorded %.6e), rms %.3e m" %
          (fmt, rot0, rot, floor_rot, trans0, trans, floor_trans, recs[0]["rms"]))
    assert recs[0]["status"] == ir.OK and recs[0]["iterations"] == 19
    assert rot < rot0 and trans < trans0
    assert rot <= 2.0 * floor_rot and trans <= 2.0 * floor_trans
    # the information matrix of the alignment: symmetric, positive definite
    info = np.array(recs[0]["info"])
    assert np.array_equal(info, info.T) and np.all(np.linalg.eigvalsh(info) > 0.0)


def test_information_in_the_pose_graph_convention():
    """capi.icp_information_right: a right increment d of the returned pose T is the left increment x = Ad d to first order --
    (I + hat(x)) T = T (I + hat(d)) -- so d^T (Ad^T H Ad) d = x^T H x; and graph_information accepts the result"""
    from rgbd_odometry_amd import capi
    v = ir.convergence_view()
    poses, recs = host([v], "f32", "f32")
    H, T = np.array(recs[0]["info"]), poses[0]
    R, t = T[:9].reshape(3, 3).T, T[9:]
    hat = lambda w: np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    HR = capi.icp_information_right(H, T)
    rng = np.random.RandomState(3)
    for _ in range(5):
        d = rng.randn(6)
        Dm = np.zeros((4, 4))
        Dm[:3, :3], Dm[:3, 3] = hat(d[3:]), d[:3]
        X = M @ Dm @ np.linalg.inv(M)                     # hat(x) of the left increment
        x = np.array([X[0, 3], X[1, 3], X[2, 3], X[2, 1], X[0, 2], X[1, 0]])
        assert np.allclose(X[:3, :3], hat(x[3:]), atol=1e-12)
        assert np.isclose(d @ HR @ d, x @ H @ x, rtol=1e-10)
    assert np.array_equal(HR, HR.T) and np.all(np.linalg.eigvalsh(HR) > 0.0)
    omega = capi.graph_information(HR, float(recs[0]["sum_r2"]), int(recs[0]["count"]))
    assert np.allclose(omega, HR * (recs[0]["count"] - 6) / recs[0]["sum_r2"], rtol=1e-12)


def test_defaults_and_constants():
    from rgbd_odometry_amd import capi
    p = c_params()
    assert (p.levels, list(p.iterations), p.z_near, p.z_far, p.dist_max, p.huber, p.stop_norm, p.min_pivot_ratio, p.min_count) == \
           (3, [10, 5, 4, 0], 0.1, 8.0, 0.1, 0.0, 0.0, 1e-9, 6)
    assert p.sweeps() == 20
    assert load().dvo_icp_params_default(None) == capi.DVO_ERR_INVALID
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    own = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_icp.h")).read(), flags=re.S)
    for name, value in (("DVO_ICP_MAX_LEVELS", capi.DVO_ICP_MAX_LEVELS), ("DVO_ICP_MAX_ITERATIONS", capi.DVO_ICP_MAX_ITERATIONS),
                        ("DVO_ICP_MAX_PIXELS", capi.DVO_ICP_MAX_PIXELS), ("DVO_ICP_OK", capi.DVO_ICP_OK), ("DVO_ICP_FEW", capi.DVO_ICP_FEW),
                        ("DVO_ICP_DEGENERATE", capi.DVO_ICP_DEGENERATE)):
        for src in (text, own):
            assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == value, name
    assert int(re.search(r"#define\s+DVO_ICP_LAUNCHES_PER_SWEEP\s+(\d+)", text).group(1)) == capi.DVO_ICP_LAUNCHES_PER_SWEEP
    launch = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_icp_launch.h")).read()
    assert int(re.search(r"kLaunchesPerSweep\s*=\s*(\d+)", launch).group(1)) == capi.DVO_ICP_LAUNCHES_PER_SWEEP
    # the two headers declare the structs with the same text
    block = lambda src: re.search(r"#ifndef DVO_ICP_TYPES_DEFINED_(.*?)#endif", src, flags=re.S).group(1).split()
    assert block(text) == block(own)
    for name in ("dvo_icp_params_default", "dvo_icp_align_host", "dvo_icp_create", "dvo_icp_destroy", "dvo_icp_last_error", "dvo_icp_align", "dvo_icp_stats"):
        assert name in capi.C_ABI_SYMBOLS and hasattr(load(), name)


def load():
    from rgbd_odometry_amd import capi
    return capi.load_library()


def test_struct_layout_matches_header(tmp_path):
    """the ctypes mirrors and the numpy record must have the layout the C compiler gives dvo_icp_params and dvo_icp_record"""
    from rgbd_odometry_amd import capi
    fields = [("dvo_icp_params", f) for f in ("iterations", "z_near", "z_far", "dist_max", "huber", "stop_norm", "min_pivot_ratio", "min_count")] + \
             [("dvo_icp_record", f) for f in ("iterations", "count", "reserved", "sum_r2", "rms", "info")]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu' + " %zu" * len(fields) + '", '
                   "sizeof(dvo_icp_params), sizeof(dvo_icp_record), " + ", ".join("offsetof(%s, %s)" % f for f in fields) + ");return 0;}")
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    P, R = capi.DvoIcpParams, capi.DvoIcpRecord
    assert [C.sizeof(P), C.sizeof(R)] + [getattr(P if s == "dvo_icp_params" else R, f).offset for s, f in fields] == got
    assert capi.ICP_RECORD_DTYPE.itemsize == C.sizeof(R)
    assert [capi.ICP_RECORD_DTYPE.fields[f][1] for _, f in fields[8:]] == got[10:]


def test_refusals_leave_the_outputs_untouched():
    from rgbd_odometry_amd import capi
    lib = load()
    views = ir.good_views(ir.SIZES[0])[:2]
    rows, cols = ir.SIZES[0]
    now = [np.ascontiguousarray(v["now_u16"]) for v in views]
    model = [np.ascontiguousarray(v["model_u16"]) for v in views]
    nrm = [np.ascontiguousarray(v["normals"]) for v in views]
    lists = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    half = lambda arrs: (C.c_void_p * 2)(arrs[0].ctypes.data, None)
    K = np.array([v["K"] for v in views])
    Pm, Ps = np.stack([v["model_pose"] for v in views]), np.stack([v["start_pose"] for v in views])
    poses = np.full((2, 12), -7.5)
    recs = np.zeros(2, capi.ICP_RECORD_DTYPE)
    recs.view(np.uint8)[:] = 0x5A
    prm = c_params()

    def raw(p=prm, count=2, nf=capi.DVO_DEPTH_U16, mf=capi.DVO_DEPTH_U16, r=rows, c=cols, k=K, n=lists(now), m=lists(model), q=lists(nrm), pm=Pm, ps=Ps,
            out=poses, rec=recs):
        ptr = lambda a: None if a is None else capi._ptr(a)
        return lib.dvo_icp_align_host(None if p is None else C.byref(p), count, nf, mf, r, c, ptr(k), n, m, q, ptr(pm), ptr(ps), ptr(out), ptr(rec))

    def untouched():
        return np.all(poses == -7.5) and np.all(recs.view(np.uint8) == 0x5A)

    nan, inf = float("nan"), float("inf")
    bad = [dict(p=None), dict(k=None), dict(n=None), dict(m=None), dict(q=None), dict(pm=None), dict(ps=None), dict(out=None), dict(rec=None),
           dict(n=half(now)), dict(m=half(model)), dict(q=half(nrm)), dict(count=0), dict(count=-3), dict(r=0), dict(c=0), dict(c=-4),
           dict(r=4097, c=4096), dict(r=1 << 16, c=1 << 16), dict(nf=2), dict(nf=-1), dict(mf=2), dict(mf=7)]
    bad += [dict(p=c_params(**kw)) for kw in (
        dict(levels=0), dict(levels=5), dict(iterations=(10, 5, -1)), dict(iterations=(65,)), dict(iterations=(1, 1, 1, 65)),
        dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=9.0), dict(z_near=nan), dict(z_far=inf), dict(z_far=nan), dict(dist_max=0.0),
        dict(dist_max=-0.1), dict(dist_max=nan), dict(dist_max=inf), dict(huber=-1e-3), dict(huber=nan), dict(huber=inf), dict(stop_norm=-1e-9),
        dict(stop_norm=nan), dict(min_pivot_ratio=0.0), dict(min_pivot_ratio=1.0), dict(min_pivot_ratio=-0.5), dict(min_pivot_ratio=nan),
        dict(min_count=0), dict(min_count=-6))]
    for j in range(4):
        for value in (nan, inf):
            Kb = K.copy()
            Kb[1, j] = value
            bad.append(dict(k=Kb))
    bad += [dict(k=np.array([[30.0, 30.0, 15.5, 11.5], [0.0, 30.0, 15.5, 11.5]])), dict(k=np.array([[30.0, -1.0, 15.5, 11.5], [30.0, 30.0, 15.5, 11.5]]))]
    for which in ("pm", "ps"):
        for j in (0, 8, 9, 11):
            for value in (nan, -inf):
                Pb = (Pm if which == "pm" else Ps).copy()
                Pb[1, j] = value
                bad.append({which: Pb})
    for kw in bad:
        assert raw(**kw) == capi.DVO_ERR_INVALID, kw
        assert untouched(), kw
    assert capi.DVO_ICP_MAX_PIXELS == 4096 * 4096
    assert raw() == capi.DVO_OK and not untouched()
    want_poses, want = host(views, "u16", "u16")
    assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes()
    # the handle's entry points without a handle
    assert lib.dvo_icp_destroy(None) == capi.DVO_ERR_INVALID and lib.dvo_icp_stats(None, None, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_icp_align(None, None, 1, 0, 0, 1, 1, None, None, None, None, None, None, None, None, 0) == capi.DVO_ERR_INVALID
    assert lib.dvo_icp_create(1, None) == capi.DVO_ERR_INVALID


def test_inputs_are_not_modified():
    views = ir.good_views(ir.SIZES[1])
    before = [(v["now_f32"].copy(), v["model_u16"].copy(), v["normals"].copy()) for v in views]
    host(views, "f32", "u16")
    for v, (a, b, c) in zip(views, before):
        assert same_bits(v["now_f32"], a) and same_bits(v["model_u16"], b) and same_bits(v["normals"], c)


# ---- the definition's own code under sanitizers, and the C++ mirror ----

def write_case(d, views, now_fmt, model_fmt, prm):
    paths = {k: str(d / (k + ".bin")) for k in ("params", "views")}
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


def parse_output(stdout, count):
    from rgbd_odometry_amd import capi
    lines = stdout.splitlines()
    assert lines[0].split() == ["poses", str(count)] and lines[2].split() == ["records", str(count)]
    poses = np.frombuffer(bytes.fromhex(lines[1]), ">u8").astype(np.uint64).view(np.float64).reshape(count, 12)
    recs = np.frombuffer(bytes.fromhex(lines[3]), capi.ICP_RECORD_DTYPE)
    return poses, recs, lines[4:]


def code_of(fmt):
    from rgbd_odometry_amd import capi
    return {"u16": capi.DVO_DEPTH_U16, "f32": capi.DVO_DEPTH_F32}.get(fmt, fmt)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("icp")
    exe = str(d / "icp_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "icp_main.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/icp_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def run_program(host_program, views, now_fmt, model_fmt, prm, rows, cols, count=None):
    d, exe = host_program
    p = write_case(d, views, now_fmt if isinstance(now_fmt, str) else "u16", model_fmt if isinstance(model_fmt, str) else "u16", prm)
    n = len(views) if count is None else count
    run = subprocess.run([exe, p["params"], p["views"], str(code_of(now_fmt)), str(code_of(model_fmt)), str(rows), str(cols), str(n)],
                         capture_output=True, text=True, timeout=300)
    if run.returncode == 3:
        assert run.stdout.strip() == "refused"
        return None
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    poses, recs, rest = parse_output(run.stdout, n)
    assert rest == []
    return poses, recs


@pytest.mark.parametrize("size", ir.SIZES + [ir.TREE_TOP])
def test_definition_under_sanitizers(host_program, size):
    """the same code the library compiles, with every buffer allocated to its exact size: the library's bytes, clean under
    -fsanitize=address,undefined.  At 481 x 545 -- TreeSum's rounds 3 and 4 -- the tree's setting and one with levels = 4"""
    views = ir.good_views(size) + ir.stopping_views(size)
    rows, cols = size
    cases = ((SETTINGS[0], "u16", "u16"), (SETTINGS[0], "f32", "f32"), (SETTINGS[4], "f32", "u16"))
    if size == ir.TREE_TOP:
        cases = ((ir.TREE_SETTING, "u16", "f32"), (ir.LEVEL3_CASES[2][1], "f32", "u16"))
        assert ir.LEVEL3_CASES[2][0] == size and cases[1][0]["levels"] == 4
    for setting, now_fmt, model_fmt in cases:
        got = run_program(host_program, views, now_fmt, model_fmt, c_params(**setting), rows, cols)
        assert got is not None
        want_poses, want = host(views, now_fmt, model_fmt, **setting)
        assert same_bits(got[0], want_poses) and got[1].tobytes() == want.tobytes(), (size, setting, now_fmt, model_fmt)


def test_program_refuses_what_the_definition_refuses(host_program):
    views = ir.good_views(ir.SIZES[0])[:1]
    rows, cols = ir.SIZES[0]
    assert run_program(host_program, views, "u16", "u16", c_params(), rows, cols) is not None
    for kw in (dict(prm=c_params(levels=0)), dict(prm=c_params(dist_max=0.0)), dict(prm=c_params(min_pivot_ratio=1.0)), dict(now_fmt=2), dict(model_fmt=-1),
               dict(rows=0), dict(cols=-1), dict(count=0), dict(count=-1)):
        args = dict(now_fmt="u16", model_fmt="u16", prm=c_params(), rows=rows, cols=cols)
        args.update(kw)
        assert run_program(host_program, views, **args) is None, kw
    bad = dict(views[0])
    bad["start_pose"] = views[0]["start_pose"].copy()
    bad["start_pose"][10] = np.nan
    assert run_program(host_program, [bad], "u16", "u16", c_params(), rows, cols) is None


def test_cpp_mirror(tmp_path):
    """include/dvo_amd.hpp's icpAlignHost and IcpAligner: tests/host/icp_hpp_main.cpp compiles with plain g++ and every warning on and
    links against the library; the host function gives the library's bytes, and on two cases IcpAligner is asked too: the same bytes
    where there is a device, a loud refusal where there is none"""
    import torch
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "icp_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "icp_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    for size, now_fmt, model_fmt, setting, on_device in ((ir.SIZES[0], "u16", "u16", SETTINGS[0], False), (ir.SIZES[1], "f32", "u16", SETTINGS[4], True),
                                                         (ir.SIZES[2], "f32", "f32", SETTINGS[0], True)):
        views = ir.good_views(size) + ir.stopping_views(size)
        rows, cols = size
        p = write_case(tmp_path, views, now_fmt, model_fmt, c_params(**setting))
        run = subprocess.run([exe, p["params"], p["views"], str(code_of(now_fmt)), str(code_of(model_fmt)), str(rows), str(cols), str(len(views))] +
                             (["device"] if on_device else []), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        poses, recs, rest = parse_output(run.stdout, len(views))
        want_poses, want = host(views, now_fmt, model_fmt, **setting)
        assert same_bits(poses, want_poses) and recs.tobytes() == want.tobytes(), (size, now_fmt, model_fmt)
        if not on_device:
            assert rest == []
        elif torch.cuda.is_available():
            assert rest[0] == "device equal 1", (size, rest)
        else:
            assert rest[0].startswith("device none") and "no CPU fallback" in rest[0]
    p = write_case(tmp_path, ir.good_views(ir.SIZES[0])[:1], "u16", "u16", c_params(dist_max=-1.0))
    run = subprocess.run([exe, p["params"], p["views"], "1", "1", "24", "32", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 3 and run.stdout.strip() == "refused"


def test_no_device_fails_loudly():
    import torch
    from rgbd_odometry_amd import capi
    if torch.cuda.is_available():
        with capi.DvoIcp(1) as h:
            assert h.stats() == (0, 0)
        return
    with pytest.raises(capi.DvoError) as ei:
        capi.DvoIcp(1)
    assert ei.value.code == capi.DVO_ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)
