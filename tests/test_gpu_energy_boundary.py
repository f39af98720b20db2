"""Energies ON the float rounding boundary, through every alignment path, against the CPU oracle and the definition itself.

tests/energy_boundary.py builds inputs whose first energy (iteration 0, identity pose, caller-supplied DT image) has its exact sum
of eps^2 within k double-ulps of the squared midpoint of two floats.  For |k| <= N/4 the packed fused kernel's certificate cannot
hold, whatever order it added in: the iteration must be settled by the exact sweep, entered NATURALLY (not by engine_variant = 5),
and level_energy_sweeps says so; at |k| = 8N the certificate must hold (it must not refuse everything).  In between nothing is
asserted about the count.  Plain double sums get more than half of these cases wrong (tests/test_energy_boundary_cpu.py), so
bit-equality here is not luck.

Every case runs with max_iters = 1 and again with 6 iterations (the later energies are ordinary and must match too): energy, best
index, visible ratio, finalEpsilons / finalReprojections bit-equal to the oracle's, energy[0] bit-equal to
np.float32(math.sqrt(math.fsum(eps^2))).  One context per configuration, the cases looped inside it; oracle runs are computed once
and shared.  Sizes 32x24, 64x48, 160x120 with every pixel a reference edge: N = 768 (below one round of a 512-thread workgroup at
two points per lane), 3072, 19200 (past half a CU's LDS in 8-byte points; above the wide schedule's solo limit).

lds_point_bytes = -1 gives the fused kernel no dynamic LDS at all, and the compact form's palette lives there (dvo_amd.h: "< 0 =
none"): the prepared flavour-B images are then read as 16-byte texels (mode 0) by design.  "Every point streamed" on the compact
form is the 256-thread shape with a budget that holds the palette but not one round of points.

A PARTIAL compact form cannot be made from caller-supplied images -- only the native builder writes one -- so the exact sweep on a
partial form stays covered by engine_variant = 5 on the sparse scenes (tests/test_gpu_sparse_scenes.py).
"""
import os
import threading

import numpy as np
import pytest

import energy_boundary as eb

pytestmark = pytest.mark.gpu

I3, Z3 = np.eye(3), np.zeros(3)
ITERS = (1, 6)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _install(ctx, c, state, pair=0, prepare=True):
    """case c as pair `pair`'s level 0: the reference list again only when the size changes; flavour B through dvo_now_prepare"""
    ctx.set_now_level(0, c.dt, c.gx, c.gy, c.rows, c.cols, pair=pair)
    if state.get(pair) != (c.rows, c.cols):
        xyz, _ = ctx.set_ref_level_from_images(0, c.edge, c.depth, c.rows, c.cols, pair=pair)
        assert np.array_equal(xyz, c.xyz)
        state[pair] = (c.rows, c.cols)
    compact = prepare and c.base.flavour == "B"
    if compact:
        ctx.now_prepare(pair, 1)
        assert ctx.now_compact_info(pair, 0) > 0, (c.id, "generic builder refused: reason", ctx.now_compact_info(pair, 0))
    return compact


def _check_report(c, ref, energy, best, ratio, what):
    assert _same(energy, ref["energy"]), (c.id, what, energy, ref["energy"])
    assert energy[0] == c.expected, (c.id, what, energy[0], c.expected)
    assert best == ref["best_idx"] and ratio == ref["visible_ratio"], (c.id, what, best, ratio)


def _check_run(c, ref, got, what):
    _check_report(c, ref, got["energy"], got["best_idx"], got["visible_ratio"], what)
    assert _same(got["final_eps"], ref["final_eps"]) and _same(got["final_reproj"], ref["final_reproj"]), (c.id, what)


def _check_sweeps(ctx, c, what, pair=0):
    n = ctx.level_energy_sweeps(pair, 0)
    if c.boundary:
        assert n == 1, (c.id, what, n, "the certificate held on a boundary energy")
    elif abs(c.k) == 8 * c.N:
        assert n == 0, (c.id, what, n, "the certificate refused an ordinary energy")


@pytest.mark.parametrize("kw", [
    dict(),                                          # auto: a single pair -> a team launch from 5000 points on
    dict(team_size=1, block_threads=512),
    dict(team_size=1, block_threads=256),            # N = 19200 does not fit half a CU's LDS: 4-byte points
    dict(lds_point_bytes=16 * 1024),                 # 2048 points resident, the rest streamed: the exact sweep crosses both
    dict(lds_point_bytes=-1),                        # every point streamed; no LDS at all, so no palette either: 16-byte texels
    dict(team_size=1, block_threads=256, lds_point_bytes=3000),      # the palette fits, not one round of points: streamed AND compact
    dict(engine_variant=1),                          # the one-point-per-lane kernel
], ids=["auto", "512", "256", "lds16k", "streamed", "256-streamed-compact", "one-point-per-lane"])
def test_fused_kernel_on_boundary_energies(oracle, kw):
    from rgbd_odometry_amd import DvoContext
    packed = kw.get("engine_variant", 0) != 1
    with DvoContext(1, **kw) as ctx:
        state = {}
        for c in eb.cases(oracle):
            ctx.set_intrinsics(*c.K)
            compact = _install(ctx, c, state, prepare=packed) and kw.get("lds_point_bytes", 0) >= 0
            for iters in ITERS:
                ref = eb.reference(oracle, c, iters)
                got = ctx.run_iterations(0, iters, I3, Z3)
                _check_run(c, ref, got, (kw, iters))
                if not packed:
                    continue
                assert ctx.last_launch_shape()[2], (c.id, "not the packed kernel")
                mode = ctx.level_texel_mode(0, 0)
                assert (mode == 2) if compact else (mode in (0, 1)), (c.id, kw, mode)
                if iters == 1:
                    _check_sweeps(ctx, c, kw)
                if not kw and c.N >= 5000:
                    assert ctx.last_launch_shape()[1] > 1, (c.id, "a single large pair is a team launch")
                if kw.get("block_threads") == 256 and c.N > 15000 and compact:
                    assert ctx.level_points4(0, 0), c.id


@pytest.mark.parametrize("team", [0, 1], ids=["auto", "no-teams"])
def test_batch_alternating_boundary_and_ordinary_pairs(oracle, team):
    """8 pairs in one launch, boundary and ordinary (|k| = 8N) cases alternating: the decision to sweep is taken per workgroup / per
    team -- the counts read 1,0,1,0,... and every pair has ITS oracle's result"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    groups = {}
    for c in eb.cases(oracle):
        if c.base.seed == 0:
            groups.setdefault((c.base.n_key, c.base.flavour), []).append(c)
    with DvoContext(8, team_size=team) as ctx:
        state = {}
        for (n_key, flavour), cs in sorted(groups.items()):
            hot = [c for c in cs if c.boundary]
            cold = [c for c in cs if abs(c.k) == 8 * c.N]
            assert len(hot) >= 4 and len(cold) == 2
            pairs = [hot[(3 * p // 2) % len(hot)] if p % 2 == 0 else cold[(p // 2) % 2] for p in range(8)]
            ctx.set_intrinsics(*pairs[0].K)
            for p, c in enumerate(pairs):
                _install(ctx, c, state, pair=p)
            for iters in ITERS:
                ctx.align_batch([iters], np.tile(I3, (8, 1, 1)), np.zeros((8, 3)), flags=DVO_FLAG_FINAL_OUTPUTS)
                for p, c in enumerate(pairs):
                    ref = eb.reference(oracle, c, iters)
                    _check_report(c, ref, *ctx.level_report(p, 0, iters), what=(team, p, iters))
                    fe, fr = ctx.final_outputs(p, c.N)
                    assert _same(fe, ref["final_eps"]) and _same(fr, ref["final_reproj"]), (c.id, p)
                if iters == 1:
                    assert [ctx.level_energy_sweeps(p, 0) for p in range(8)] == [1, 0] * 4, (n_key, flavour, team)


@pytest.mark.parametrize("shards", [1, 3])
def test_host_driven_iterations_on_boundary_energies(oracle, shards):
    """dvo_iter_*: the three limbs of every shard's exact sum ride in slots 29..31 and are added like an all-reduce would"""
    import torch
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.distributed import HipTiledEngine, shard_range
    with DvoContext(1) as ctx:
        eng = HipTiledEngine(ctx)
        state = {}
        parts = [eng.new_acc() for _ in range(shards)]
        for c in eb.cases(oracle):
            ctx.set_intrinsics(*c.K)
            _install(ctx, c, state, prepare=False)
            for iters in ITERS:
                ref = eb.reference(oracle, c, iters)
                eng.iter_begin(0, iters, I3, Z3)
                for itr in range(iters):
                    for r in range(shards):
                        eng.iter_accumulate(0, *shard_range(c.N, r, shards), parts[r].data_ptr())
                    total = parts[shards - 1].clone()
                    for r in range(shards - 2, -1, -1):
                        total = total + parts[r]
                    eng.iter_update(0, itr, c.N, total.data_ptr())
                    torch.cuda.synchronize()          # `total` must outlive the update kernel
                got = eng.iter_end(0)
                _check_report(c, ref, got["energy"], got["best_idx"], got["visible_ratio"], (shards, iters))


def test_accumulate_returns_the_exact_sum(oracle):
    """dvo_accumulate: acc[27] is math.fsum of the residuals' squares, exactly"""
    from rgbd_odometry_amd import DvoContext
    with DvoContext(1) as ctx:
        state = {}
        for c in eb.cases(oracle):
            ctx.set_intrinsics(*c.K)
            _install(ctx, c, state, prepare=False)
            acc = ctx.accumulate(0, I3, Z3)
            assert acc[27] == c.S, (c.id, acc[27], c.S)
            assert int(acc[28]) == c.n_visible, c.id


@pytest.mark.parametrize("with_h", [False, True], ids=["plain", "step-launches"])
def test_wide_schedule_on_boundary_energies(oracle, with_h):
    """dvo_align_pyramid_wide below and above the solo limit.  Plain: a level of at most 6144 points is ONE launch of one workgroup,
    a single larger level goes to the fused kernel's team launch.  With DVO_FLAG_NORMAL_MATRIX neither shortcut exists: every size
    runs the per-iteration step launches, whose limbs are added by the workgroup that arrives last"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS, DVO_FLAG_NORMAL_MATRIX
    default_limits = not any(os.environ.get(k) for k in ("DVO_TILED_SOLO_MAX", "DVO_TILED_PACKED", "DVO_WIDE_TEAM_MAX"))
    flags = DVO_FLAG_FINAL_OUTPUTS | (DVO_FLAG_NORMAL_MATRIX if with_h else 0)
    seen = set()
    with DvoContext(1) as ctx:
        state = {}
        for c in eb.cases(oracle):
            ctx.set_intrinsics(*c.K)
            _install(ctx, c, state)
            for iters in ITERS:
                ref = eb.reference(oracle, c, iters)
                ctx.align_pyramid_wide([iters], I3, Z3, flags=flags)
                _check_report(c, ref, *ctx.level_report(0, 0, iters), what=("wide", with_h, iters))
                fe, fr = ctx.final_outputs(0, c.N)
                assert _same(fe, ref["final_eps"]) and _same(fr, ref["final_reproj"]), (c.id, iters)
                if default_limits:
                    route = (ctx.wide_packed_levels(), ctx.wide_solo_levels(), ctx.wide_team_levels())
                    assert route == ((1, 0, 0) if with_h else ((1, 1, 0) if c.N <= 6144 else (0, 0, 1))), (c.id, with_h, route)
                seen.add(c.N <= 6144)
    assert seen == {True, False}


@pytest.mark.parametrize("world", [2, 3])
def test_tiled_ranks_on_boundary_energies(oracle, world):
    """dvo_align_pyramid_tiled with `world` host threads as ranks on one GPU (tests/loopback_collective stands in for ncclAllReduce):
    the ranks' limbs meet in the all-reduce; every rank reports the oracle's energies, the shards' final outputs are the oracle's"""
    import ctypes as C
    from test_gpu_tiled_ranks import LOOPBACK_SO, _loopback_library
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    lib = _loopback_library()
    comms = (C.c_void_p * world)()
    assert lib.loopback_create(world, comms) == 0
    ctxs, states = [], [dict() for _ in range(world)]
    calls = 0
    try:
        for r in range(world):
            ctxs.append(DvoContext(1))
        attached = False
        for c in eb.cases(oracle):
            for r in range(world):
                ctxs[r].set_intrinsics(*c.K)
                _install(ctxs[r], c, states[r])
                if not attached:
                    ctxs[r].tiled_attach(comms[r], r, world, LOOPBACK_SO)
            attached = True
            for iters in ITERS:
                ref = eb.reference(oracle, c, iters)
                out, err = [None] * world, [None] * world

                def run(r):
                    try:
                        out[r] = ctxs[r].align_pyramid_tiled([iters], I3, Z3, flags=DVO_FLAG_FINAL_OUTPUTS)
                    except Exception as e:          # a failing rank must not leave the others at the barrier: the library times out
                        err[r] = e
                th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
                for x in th:
                    x.start()
                for x in th:
                    x.join(120)
                assert not any(x.is_alive() for x in th) and err == [None] * world, (c.id, err)
                solo = ctxs[0].wide_solo_levels()
                calls += 0 if solo & 1 else iters
                eps_all, rep_all = np.full(c.N, np.nan, np.float32), np.full((c.N, 3), np.nan, np.float32)
                nxt = 0
                for r in range(world):
                    assert _same(out[r][0], out[0][0]) and _same(out[r][1], out[0][1]), (c.id, r)
                    assert ctxs[r].wide_solo_levels() == solo
                    assert lib.loopback_calls(comms[r]) == calls, (c.id, r, lib.loopback_calls(comms[r]), calls)
                    _check_report(c, ref, *ctxs[r].level_report(0, 0, iters), what=("tiled", world, r, iters))
                    first, count = ctxs[r].tiled_shard(0)
                    assert first == nxt
                    nxt = first + count
                    fe, fr = ctxs[r].final_outputs(0, c.N)
                    eps_all[first:nxt], rep_all[first:nxt] = fe[first:nxt], fr[first:nxt]
                assert nxt == c.N
                assert _same(eps_all, ref["final_eps"]) and _same(rep_all, ref["final_reproj"]), (c.id, iters)
        if not os.environ.get("DVO_TILED_SOLO_MAX") and not os.environ.get("DVO_TILED_PACKED"):
            assert calls > 0                       # the large level really met the collective
    finally:
        for ctx in ctxs:
            ctx.close()
        lib.loopback_destroy(comms, world)
