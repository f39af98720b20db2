"""The launch planner of the fused alignment on the device (rgbd_odometry_amd/csrc/dvo_launch_plan.h, carried out by enqueue() of
dvo_capi.cpp): for every parameter that steers the plan, one alignment of the 320x240 scene with one pair and one with nine replicated
pairs launches the shape the planner's table promises, and computes the oracle's bits.

SHAPES holds (block_threads, team, packed) of dvo_get_last_launch_shape as recorded on an MI355X from the commit before the planner
existed; the string next to each triple is the origin of the matching row of tests/host/launch_plan_main.cpp."""
import numpy as np
import pytest

import oracle_lib
from oracle_lib import rot_angle

ITERS = [6, 0, 5, 4]

# case: (context parameters, align flag names, {n_pairs: ((block, team, packed), row of the CPU table)})
SHAPES = {
    "default": ({}, (), {1: ((512, 1, 1), "comment: 320x240x4x50, single pair -> 512 threads, no team below 5000 points"),
                         9: ((512, 1, 1), "320x240, 9 pairs")}),
    "block_threads=256": (dict(block_threads=256), (), {1: ((256, 1, 1), "320x240 single pair, block_threads 256"),
                                                        9: ((256, 1, 1), "320x240, 9 pairs, block_threads 256")}),
    "block_threads=512": (dict(block_threads=512), (), {1: ((512, 1, 1), "320x240 single pair, block_threads 512"),
                                                        9: ((512, 1, 1), "320x240, 9 pairs, block_threads 512")}),
    "block_threads=1024": (dict(block_threads=1024), (), {1: ((1024, 1, 1), "320x240 single pair, block_threads 1024"),
                                                          9: ((1024, 1, 1), "320x240, 9 pairs, block_threads 1024")}),
    "team_size=1": (dict(team_size=1), (), {1: ((512, 1, 1), "320x240 single pair, team_size 1"),
                                            9: ((512, 1, 1), "320x240, 9 pairs, team_size 1")}),
    "team_size=2": (dict(team_size=2), (), {1: ((512, 2, 1), "320x240 single pair, team_size 2 forced"),
                                            9: ((512, 2, 1), "320x240, 9 pairs, team_size 2 forced")}),
    "engine_variant=1": (dict(engine_variant=1), (), {1: ((512, 1, 0), "320x240 single pair, engine_variant 1 -> one-point-per-lane kernel, 16-byte texels"),
                                                      9: ((512, 1, 0), "320x240, 9 pairs, engine_variant 1")}),
    "normal_matrix": ({}, ("DVO_FLAG_NORMAL_MATRIX",), {1: ((512, 1, 1), "320x240 single pair, DVO_FLAG_NORMAL_MATRIX -> packed, 512 threads, no team"),
                                                        9: ((512, 1, 1), "320x240, 9 pairs, DVO_FLAG_NORMAL_MATRIX")}),
}


@pytest.fixture(scope="module")
def scene320(oracle):
    from rgbd_odometry_amd import SynthScene
    sc = SynthScene(320, 240, 4, 0)
    lv = oracle_lib.scene_levels(sc, oracle)
    ref = oracle.align_pyramid(ITERS, lv, sc.intrinsics, np.eye(3), np.zeros(3))
    return sc, lv, ref


def test_cpu_table_has_the_rows():
    """every triple names a row of the planner's table"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "launch_plan_main.cpp")).read()
    for kw, flags, per_n in SHAPES.values():
        for shape, row in per_n.values():
            assert '{"%s",' % row in src, row


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [1, 9])
@pytest.mark.parametrize("case", list(SHAPES))
def test_launch_shape_and_oracle_bits(scene320, case, n_pairs):
    from rgbd_odometry_amd import DvoContext, capi
    sc, lv, ref = scene320
    kw, flag_names, per_n = SHAPES[case]
    want_shape = per_n[n_pairs][0]
    flags = 0
    for name in flag_names:
        flags |= getattr(capi, name)
    with DvoContext(n_pairs, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        for l, L in enumerate(lv):
            ctx.set_ref_level(l, L["xyz"])
            ctx.set_now_level(l, L["dt"], L["gx"], L["gy"], L["rows"], L["cols"])
        if n_pairs > 1:
            ctx.replicate_pairs(1)
        assert ctx.n_points(0) < 5000                     # the rows' "no team below 5000 points"
        R, t = ctx.align_batch(ITERS, np.tile(np.eye(3), (n_pairs, 1, 1)), np.zeros((n_pairs, 3)), flags=flags)
        shape = tuple(int(v) for v in ctx.last_launch_shape())
        print(case, n_pairs, shape)
        assert shape == want_shape, (case, n_pairs, shape)
        for p in range(n_pairs):
            for l, rep in ref["levels"].items():
                e, b, ratio = ctx.level_report(p, l, ITERS[l])
                assert np.array_equal(e, rep["energy"]) and b == rep["best_idx"] and ratio == rep["visible_ratio"], (case, p, l)
            assert rot_angle(ref["R"], R[p]) <= 1e-5 and np.linalg.norm(ref["t"] - t[p]) <= 1e-4, (case, p)
