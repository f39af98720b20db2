"""Final outputs written by the last sweep of the last level in the packed fused kernel (rgbd_odometry_amd/csrc/dvo_fused.hip: RoundEF,
FinalAt).

The residual-only sweep of the last level's last iteration also projects every point at the best of the iterates before it and stores
finalEpsilons / finalReprojections; the separate pass over the level is skipped when that iterate is still the best after the loop
(dvo_get_level_final_fused says 1) and runs, overwriting them, when the last iterate won.  Nothing the caller sees may change: the bars
are those of test_gpu_last_sweep.py -- energies, best index, visible ratio and final outputs bit-equal to the oracle's, poses within
1e-5 rad / 1e-4 m -- on both classes of alignments (tests/test_final_fused_cpu.py pins them), every launch shape, texel source and point
form, and on the paths that must NOT take the fused outputs (early stop, one iteration, H per iterate, outputs not asked for).
"""
import numpy as np
import pytest

from test_final_fused_cpu import CASES, kept
from test_gpu_last_sweep import _align, _load, _ref, _scene

pytestmark = pytest.mark.gpu

FULL = (10, 10, 10, 10)
SHAPES = [dict(block_threads=256), dict(block_threads=512, team_size=1), dict(team_size=2), dict(team_size=4)]
TABLE = {(W, H, seed, iters): keep for iters, W, H, seed, sparse, _, keep in CASES if not sparse}


def _flags(ctx, pair):
    return [bool(ctx.level_final_fused(pair, l)) for l in range(4)]


def _check_flags(ctx, refs, iters):
    """1 at the last level exactly for the alignments whose best iterate is not the last one, 0 everywhere else"""
    for p, ref in enumerate(refs):
        want = [False] * 4
        want[ref["last_level"]] = kept(ref, iters)
        assert _flags(ctx, p) == want, (p, iters, _flags(ctx, p), want)


@pytest.mark.parametrize("size,seeds", [((160, 120), (1000, 1002)), ((320, 240), (1000, 1004, 1002))])
@pytest.mark.parametrize("kw", SHAPES)
def test_both_classes_on_every_launch_shape(kw, size, seeds):
    """every scene and schedule of the table: alone in a launch, and all scenes of a size -- both classes -- in one launch"""
    from rgbd_odometry_amd import DvoContext
    W, H = size
    schedules = [FULL] + ([(3, 0, 2, 1), (1, 1, 1, 1)] if size == (160, 120) else [])
    for group in [(s,) for s in seeds] + [seeds + seeds[:3 - len(seeds)]]:          # one pair; three pairs
        with DvoContext(len(group), **kw) as ctx:
            ctx.set_intrinsics(*_scene(W, H, group[0])[0].intrinsics)
            for p, seed in enumerate(group):
                _load(ctx, *_scene(W, H, seed), "native", pair=p)
            for iters in schedules:
                refs = [_ref(W, H, seed, iters) for seed in group]
                _align(ctx, refs, iters)
                blk, g, _ = ctx.last_launch_shape()
                assert blk == kw.get("block_threads", 512) and g == kw.get("team_size", 1), (blk, g)
                _check_flags(ctx, refs, iters)
                for p, seed in enumerate(group):
                    if (W, H, seed, iters) in TABLE:
                        assert ctx.level_final_fused(p, 0) == TABLE[(W, H, seed, iters)], (seed, iters)


@pytest.mark.parametrize("kw,form,points4", [
    (dict(block_threads=256, lds_point_bytes=16 * 1024), "native", True),       # 4-byte points: whole rounds in LDS, the rest streamed
    (dict(block_threads=512, team_size=1, lds_point_bytes=16 * 1024), "native", True),
    (dict(team_size=2, lds_point_bytes=16 * 1024), "native", False),            # a team reads 8-byte points: LDS part + streamed tail
    (dict(block_threads=256, lds_point_bytes=8 * 1024), "float", False),        # 16-byte texels gathered, 8-byte points streamed
    (dict(block_threads=256, lds_point_bytes=-1), "native", None),              # no LDS at all: every point streamed, 16-byte texels
    (dict(block_threads=256), "float", None), (dict(block_threads=512, team_size=1), "float", None), (dict(team_size=4), "float", None),
    (dict(block_threads=256), "lists", None), (dict(block_threads=512, team_size=1), "lists", None),
])
def test_point_forms_and_texel_sources(kw, form, points4):
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(320, 240, 1000)
    ref = _ref(320, 240, 1000, FULL)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, form)
        _align(ctx, [ref], FULL)
        if points4 is not None:
            assert ctx.level_points4(0, 0) == points4, kw
        if form != "native":
            assert ctx.level_texel_mode(0, 0) == 0
        assert _flags(ctx, 0) == [True, False, False, False]


def test_last_level_staged_in_lds():
    """a schedule that ends on the coarsest level, which one 512-thread workgroup stages into LDS, texels and points"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    iters = (0, 0, 0, 10)
    ref = _ref(160, 120, 1000, iters)
    assert ref["last_level"] == 3
    with DvoContext(1, block_threads=512, team_size=1) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "float")
        _align(ctx, [ref], iters)
        assert ctx.level_texel_mode(0, 3) == 1
        _check_flags(ctx, [ref], iters)


@pytest.mark.parametrize("kw", SHAPES)
def test_no_iterations_at_level_zero(kw):
    """iters[0] == 0: the last level is level 1 and the outputs are that level's"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    iters = (0, 10, 10, 10)
    ref = _ref(160, 120, 1000, iters)
    assert ref["last_level"] == 1 and kept(ref, iters)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        _align(ctx, [ref], iters)
        assert _flags(ctx, 0) == [False, True, False, False]


@pytest.mark.parametrize("kw", SHAPES[:3])
def test_early_stop_takes_the_separate_pass(kw):
    """psi_norm_stop = 1e-2: every level stops in iteration 0, no last sweep is reached"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    ref = _ref(160, 120, 1000, FULL, stop=1e-2)
    assert all(r["iters_run"] == 1 for r in ref["levels"].values())
    with DvoContext(1, psi_norm_stop=1e-2, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        _align(ctx, [ref], FULL)
        assert _flags(ctx, 0) == [False] * 4


@pytest.mark.parametrize("variant", [3, 5])
@pytest.mark.parametrize("kw", SHAPES[:3])
def test_literal_redo_and_exact_energy_sweep(kw, variant):
    """engine_variant = 3: every wave redoes every sweep with the literal-division code and keeps the outputs it has written;
    engine_variant = 5: the exact energy sweep runs after every sweep, the last one included"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    ref = _ref(160, 120, 1000, FULL)
    for form in ("native", "float"):
        with DvoContext(1, engine_variant=variant, **kw) as ctx:
            ctx.set_intrinsics(*sc.intrinsics)
            _load(ctx, sc, lv, form)
            _align(ctx, [ref], FULL)
            if variant == 3:
                assert all(ctx.level_exact_fallback(0, l) for l in range(4))
            else:
                assert [ctx.level_energy_sweeps(0, l) for l in range(4)] == list(FULL)
            assert _flags(ctx, 0) == [True, False, False, False]


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict()])
def test_partial_compact_form(kw):
    """level 0 of the sparse scene has a partial compact form; with [9, 1, 1, 1] its best iterate is the one before the last, so the
    outputs -- the NaN ranks patched from the 16-byte texels -- are the sweep's; with [10, 1, 1, 1] the last iterate wins"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(640, 480, 2000, sparse=True)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        assert ctx.now_compact_partial(0, 0)
        for iters, want in (((9, 1, 1, 1), True), ((10, 1, 1, 1), False)):
            ref = _ref(640, 480, 2000, iters, sparse=True)
            _align(ctx, [ref], iters)
            assert ctx.level_texel_mode(0, 0) == 2
            assert _flags(ctx, 0) == [want, False, False, False]


@pytest.mark.parametrize("kw", SHAPES)
def test_warm_start(kw):
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(320, 240, 1000)
    ref = _ref(320, 240, 1000, FULL, warm=True)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        _align(ctx, [ref], FULL, warm=True)
        _check_flags(ctx, [ref], FULL)


@pytest.mark.parametrize("block", [256, 512])
def test_normal_matrix_keeps_the_separate_pass(block):
    """DVO_FLAG_NORMAL_MATRIX: these instantiations have no residual-only sweep; outputs unchanged, flag 0"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_NORMAL_MATRIX
    sc, lv = _scene(160, 120, 1000)
    ref = _ref(160, 120, 1000, FULL)
    assert kept(ref, FULL)
    with DvoContext(1, block_threads=block, team_size=1) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        _align(ctx, [ref], FULL, flags=DVO_FLAG_NORMAL_MATRIX)
        assert _flags(ctx, 0) == [False] * 4


@pytest.mark.parametrize("kw", SHAPES[:3])
def test_without_final_outputs(kw):
    """without DVO_FLAG_FINAL_OUTPUTS nothing is written and nothing is reported, the alignment is the same"""
    from rgbd_odometry_amd import DvoContext
    from oracle_lib import rot_angle
    sc, lv = _scene(160, 120, 1000)
    ref = _ref(160, 120, 1000, FULL)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        R, t = ctx.align_batch(list(FULL), np.eye(3)[None], np.zeros((1, 3)), flags=0)
        for l, rep in ref["levels"].items():
            e, b, ratio = ctx.level_report(0, l, FULL[l])
            assert np.array_equal(e, rep["energy"]) and b == rep["best_idx"] and ratio == rep["visible_ratio"]
        assert rot_angle(ref["R"], R[0]) <= 1e-5 and np.linalg.norm(ref["t"] - t[0]) <= 1e-4
        assert _flags(ctx, 0) == [False] * 4
