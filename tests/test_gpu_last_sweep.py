"""The residual-only sweep of a level's LAST iteration in the packed fused kernel (rgbd_odometry_amd/csrc/dvo_fused.hip: RoundE, AccR).

runIterations sets the pose to the best iterate after its loop (SolveDVO.cpp:997-1005), so the update computed in the last iteration is
dead: that sweep gathers the centre rank word (or the DT dword) alone, adds sum eps^2 and the visible count, and wave 0 skips the
update.  Nothing the caller sees may change: energies of every iterate, best index, visible ratio and final outputs bit-equal to the
oracle's, poses within 1e-5 rad / 1e-4 m -- the bars of test_gpu_packed_kernel.py -- on the list lengths where the new loops take
another path (a partial round, a tail behind whole rounds, a half-filled round, the pipelined steady state), on every texel source and
point form, on every launch shape, and on the rare paths (literal-division redo, exact energy sweep, NaN rank of a partial compact form).
"""
import functools

import numpy as np
import pytest

import oracle_lib
from oracle_lib import rot_angle

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4
SCHEDULES = ([1, 1, 1, 1], [3, 0, 2, 1], [10, 10, 10, 10])     # every sweep residual-only; a skipped level; the bench's schedule


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _u8(a):
    return (np.asarray(a) != 0).astype(np.uint8) * 255


@functools.lru_cache(maxsize=None)
def _scene(W, H, seed, sparse=False):
    from rgbd_odometry_amd import SynthScene
    if sparse:          # the smallest scene of tests/test_gpu_sparse_scenes.py: level 0 gets a partial compact form
        sc = SynthScene(W, H, 4, seed, n_seg=max(2, int(round(0.005 * W * H / (70.0 * W / 320.0)))), x_frac=0.5)
    else:
        sc = SynthScene(W, H, 4, seed)
    return sc, oracle_lib.scene_levels(sc, oracle_lib.load())


@functools.lru_cache(maxsize=None)
def _ref(W, H, seed, iters, sparse=False, warm=False, stop=None):
    """the oracle's alignment, computed once per (scene, schedule, start, parameters) and shared"""
    oracle = oracle_lib.load()
    sc, lv = _scene(W, H, seed, sparse)
    R0, t0 = _start(warm)
    prm = None
    if stop is not None:
        prm = oracle.default_params()
        prm.psi_norm_stop = stop
    return oracle.align_pyramid(list(iters), lv, sc.intrinsics, R0, t0, params=prm)


def _start(warm):
    if not warm:
        return np.eye(3), np.zeros(3)
    R0, t0 = oracle_lib.load().se3_exp(np.array([0.01, -0.005, 0.008, 0.004, -0.01, 0.006]))
    return np.array(R0), np.array(t0)


def _load(ctx, sc, lv, form, pair=0):
    """native: engine-built lists + now levels written in the compact form by the engine's distance transform (the bench's path);
    float: engine-built lists + caller-supplied float images (16-byte texels; the coarse levels of a 512-thread workgroup are staged
    into LDS); lists: the reference's 3 x N float lists, which verify as enlistRefEdgePts lists, + float images"""
    for l, L in enumerate(sc.levels):
        if form == "lists":
            ctx.set_ref_level(l, lv[l]["xyz"], pair=pair)
        else:
            xyz, _ = ctx.set_ref_level_from_images(l, L.ref_edge, L.ref_depth, L.rows, L.cols, pair=pair)
            assert len(xyz) == len(lv[l]["xyz"])
        if form == "native":
            ctx.set_now_level_from_edges(l, _u8(L.now_edge), L.rows, L.cols, pair=pair)
        else:
            ctx.set_now_level(l, L.now_dt, L.now_gx, L.now_gy, L.rows, L.cols, pair=pair)


def _compare(ctx, ref, iters, pair=0):
    for l, rep in ref["levels"].items():
        e, b, ratio = ctx.level_report(pair, l, iters[l])
        assert np.array_equal(e, rep["energy"]), (pair, l, e, rep["energy"])
        assert b == rep["best_idx"] and ratio == rep["visible_ratio"], (pair, l, b, rep["best_idx"])
    last = ref["levels"][ref["last_level"]]
    feps, frep = ctx.final_outputs(pair, len(last["final_eps"]))
    assert _same(feps, last["final_eps"]) and _same(frep, last["final_reproj"]), pair


def _align(ctx, refs, iters, warm=False, flags=0):
    """one launch over all pairs of the context, every pair against its own oracle run"""
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    n = len(refs)
    R0, t0 = _start(warm)
    R, t = ctx.align_batch(list(iters), np.tile(R0, (n, 1, 1)), np.tile(t0, (n, 1)), flags=DVO_FLAG_FINAL_OUTPUTS | flags)
    assert ctx.last_launch_shape()[2], "the packed kernel is what this file tests"
    for p, ref in enumerate(refs):
        _compare(ctx, ref, iters, pair=p)
        assert rot_angle(ref["R"], R[p]) <= ROT_TOL and np.linalg.norm(ref["t"] - t[p]) <= TRANS_TOL, p
    return R, t


def test_scene_sizes_are_the_ones_the_loops_branch_on():
    """160x120: at rounds of 512 points two rounds with a partial second, one round plus a tail of 21, a round whose second half holds
    8 points, a half-filled first half; 320x240: several whole rounds (the pipelined steady state)"""
    assert [len(L["xyz"]) for L in _scene(160, 120, 1000)[1]] == [1013, 533, 264, 128]
    assert [len(L["xyz"]) for L in _scene(320, 240, 1000)[1]] == [3905, 2052, 998, 455]


@pytest.mark.parametrize("size", [(160, 120), (320, 240)])
@pytest.mark.parametrize("kw,n_pairs", [
    (dict(block_threads=256), 1), (dict(block_threads=512, team_size=1), 1),
    (dict(team_size=2), 1), (dict(team_size=2), 3), (dict(team_size=4), 1), (dict(team_size=4), 3),
])
def test_last_sweep_native_compact_levels(size, kw, n_pairs):
    """the throughput path (rank words + palette) through the launch shapes, all three schedules"""
    from rgbd_odometry_amd import DvoContext
    W, H = size
    with DvoContext(n_pairs, **kw) as ctx:
        sc0 = _scene(W, H, 1000)[0]
        ctx.set_intrinsics(*sc0.intrinsics)
        for p in range(n_pairs):
            sc, lv = _scene(W, H, 1000 + p)
            _load(ctx, sc, lv, "native", pair=p)
        for iters in SCHEDULES:
            _align(ctx, [_ref(W, H, 1000 + p, tuple(iters)) for p in range(n_pairs)], iters)
            blk, g, _ = ctx.last_launch_shape()
            assert blk == kw.get("block_threads", 512) and g == kw.get("team_size", 1), (blk, g)
            assert [ctx.level_texel_mode(0, l) for l in range(4) if iters[l]] == [2] * sum(1 for i in iters if i)
            assert not any(ctx.level_exact_fallback(0, l) for l in range(4))


@pytest.mark.parametrize("kw,form,points4", [
    (dict(block_threads=256, lds_point_bytes=16 * 1024), "native", True),       # 4-byte points: whole rounds in LDS, the rest streamed
    (dict(block_threads=512, team_size=1, lds_point_bytes=16 * 1024), "native", True),
    (dict(team_size=2, lds_point_bytes=16 * 1024), "native", False),            # a team reads 8-byte points: LDS part + streamed tail
    (dict(block_threads=256, lds_point_bytes=8 * 1024), "float", False),        # 16-byte texels gathered, 8-byte points streamed
    (dict(block_threads=256, lds_point_bytes=-1), "native", None),              # no LDS at all: every point streamed, 16-byte texels
])
def test_last_sweep_with_part_of_every_list_streamed(kw, form, points4):
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(320, 240, 1000)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, form)
        for iters in SCHEDULES:
            _align(ctx, [_ref(320, 240, 1000, tuple(iters))], iters)
            if points4 is not None:
                assert ctx.level_points4(0, 0) == points4, kw
                assert ctx.level_texel_mode(0, 0) == (2 if form == "native" else 0)


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict(team_size=4)])
@pytest.mark.parametrize("form", ["float", "lists"])
def test_last_sweep_float_images_and_float_lists(kw, form):
    """16-byte texels gathered from memory and -- one 512-thread workgroup, coarse levels -- from their LDS copy; reference lists given
    as 3 x N floats that verify"""
    from rgbd_odometry_amd import DvoContext
    for W, H in ((160, 120), (320, 240)):
        sc, lv = _scene(W, H, 1000)
        with DvoContext(1, **kw) as ctx:
            ctx.set_intrinsics(*sc.intrinsics)
            _load(ctx, sc, lv, form)
            for iters in SCHEDULES:
                _align(ctx, [_ref(W, H, 1000, tuple(iters))], iters)
                modes = [ctx.level_texel_mode(0, l) for l in range(4)]
                assert 2 not in modes, modes
                if kw.get("block_threads") == 512:
                    assert modes[3] == 1, modes                      # the coarsest level lives in LDS, texels and points


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict(team_size=2)])
@pytest.mark.parametrize("form", ["native", "float"])
def test_last_sweep_with_every_energy_from_the_exact_sweep(kw, form):
    """engine_variant = 5: the certificate is refused everywhere, so the exact-limb sweep runs after every sweep, residual-only ones
    included, and says so"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    with DvoContext(1, engine_variant=5, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, form)
        for iters in SCHEDULES:
            _align(ctx, [_ref(160, 120, 1000, tuple(iters))], iters)
            assert [ctx.level_energy_sweeps(0, l) for l in range(4) if iters[l]] == [i for i in iters if i]


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict(team_size=4)])
def test_last_sweep_through_the_literal_division_code(kw):
    """engine_variant = 3: every wave redoes every sweep with the literal-division code -- residual only in a last iteration"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    for form in ("native", "float"):
        with DvoContext(1, engine_variant=3, **kw) as ctx:
            ctx.set_intrinsics(*sc.intrinsics)
            _load(ctx, sc, lv, form)
            for iters in SCHEDULES:
                _align(ctx, [_ref(160, 120, 1000, tuple(iters))], iters)
                assert all(ctx.level_exact_fallback(0, l) for l in range(4) if iters[l])


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict()])
def test_partial_compact_form_in_a_last_iteration(kw):
    """level 0 of the sparse scene has a partial compact form: a centre rank that is its NaN entry sends the wave to the 16-byte
    texels, in a residual-only sweep as in a full one"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(640, 480, 2000, sparse=True)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        assert ctx.now_compact_partial(0, 0)
        for iters in ([1, 1, 1, 1], [3, 0, 2, 1]):
            _align(ctx, [_ref(640, 480, 2000, tuple(iters), sparse=True)], iters)
            assert [ctx.level_texel_mode(0, l) for l in range(4) if iters[l]] == [2] * sum(1 for i in iters if i)


def test_degenerate_depth_met_in_a_last_iteration(oracle):
    """the start translation EQUALS a reference point (z = 0 exactly, test_gpu_packed_kernel.py): with one iteration the only sweep
    is the residual-only one, and it must take the literal-division redo like a full sweep"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(320, 240, 1000)
    for kw, form in ((dict(), "float"), (dict(block_threads=256), "native"), (dict(block_threads=512, team_size=1), "native")):
        with DvoContext(1, **kw) as ctx:
            ctx.set_intrinsics(*sc.intrinsics)
            _load(ctx, sc, lv, form)
            for level in (0, 2):
                L = lv[level]
                xyz = np.asarray(L["xyz"]).reshape(-1, 3)
                for idx in (0, len(xyz) // 2, len(xyz) - 1):
                    t0 = xyz[idx].astype(np.float64)
                    for n_it in (1, 2):
                        ref = oracle.run_iterations(level, n_it, L["xyz"], L["dt"], L["gx"], L["gy"], L["rows"], L["cols"],
                                                    sc.intrinsics, np.eye(3), t0)
                        got = ctx.run_iterations(level, n_it, np.eye(3), t0)
                        assert ctx.level_exact_fallback(0, level), (kw, level, idx, n_it)
                        assert _same(ref["energy"], got["energy"]), (kw, level, idx, ref["energy"], got["energy"])
                        assert ref["best_idx"] == got["best_idx"] and ref["visible_ratio"] == got["visible_ratio"]
                        assert _same(ref["final_eps"], got["final_eps"]) and _same(ref["final_reproj"], got["final_reproj"])


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict(team_size=2)])
def test_early_stop_runs_no_residual_only_sweep(kw):
    """psi_norm_stop = 1e-2 is above the trust radius (3e-3): every level stops in iteration 0, whose sweep is a full one"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(160, 120, 1000)
    iters = [10, 10, 10, 10]
    ref = _ref(160, 120, 1000, tuple(iters), stop=1e-2)
    assert all(r["iters_run"] == 1 for r in ref["levels"].values())
    with DvoContext(1, psi_norm_stop=1e-2, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        _align(ctx, [ref], iters)


@pytest.mark.parametrize("kw", [dict(block_threads=256), dict(block_threads=512, team_size=1), dict(team_size=4)])
def test_last_sweep_from_a_warm_start(kw):
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(320, 240, 1000)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        for iters in SCHEDULES:
            _align(ctx, [_ref(320, 240, 1000, tuple(iters), warm=True)], iters, warm=True)


@pytest.mark.parametrize("block", [256, 512])
def test_normal_matrix_of_the_last_iterate_is_still_reported(oracle, block):
    """DVO_FLAG_NORMAL_MATRIX: H is reported for EVERY iterate, so these instantiations keep the full sweep in the last iteration"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_NORMAL_MATRIX
    sc, lv = _scene(160, 120, 1000)
    iters = [3, 0, 2, 1]
    with DvoContext(1, block_threads=block, team_size=1) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        _align(ctx, [_ref(160, 120, 1000, tuple(iters))], iters, flags=DVO_FLAG_NORMAL_MATRIX)
        Rc, tc = np.eye(3), np.zeros(3)
        for l in (3, 2, 0):
            L = lv[l]
            r = oracle.run_iterations(l, iters[l], L["xyz"], L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], sc.intrinsics, Rc, tc, trace=True)
            assert len(r["trace"]) == iters[l]
            for itr, tr in enumerate(r["trace"]):
                H = ctx.level_normal_matrix(0, l, itr)
                want = np.zeros((6, 6)); k = 0
                for i in range(6):
                    for j in range(i, 6):
                        want[i, j] = want[j, i] = tr["H"][k]; k += 1
                assert np.abs(want).max() > 0
                # the bar of tests/test_gpu_parity.py: same per-point products, the double sums added in another order
                np.testing.assert_allclose(H, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
            Rc, tc = r["R"], r["t"]
