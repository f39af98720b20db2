"""The round counts at the edges of the fused kernel's three-deep gather pipeline (rgbd_odometry_amd/csrc/dvo_fused.hip:
accumulate_points2, DEPTH == 3), on the GPU.

The prologue now issues the first TWO rounds on every path -- a wave with a single round projects the list's last point once more and
puts its count back -- and the residual-only sweep that writes the final outputs runs its first trip of three rounds in front of its
loop.  What can go wrong sits where prologue, loop and tail meet, so one level of 96 x 128 carries a reference list of exactly N points,
N chosen so that the waves of a 256-thread workgroup (a round is 512 points; the waves start at points 0, 64, 128 and 192 of it) have
0, 1, 2, 3, 4, 5, 7, 8 and 9 rounds, lists that end exactly on a round included.  Every N runs 1, 2 and 3 iterations (the residual-only
sweep alone, behind one full sweep, behind two) with the final outputs on, on the 256-thread shape, on a team of two (two 512-thread
workgroups: the launch plan forms teams of those only) and with DVO_FLAG_NORMAL_MATRIX, and on the 256-thread shape in every point form: 8-byte points in LDS, 4-byte direct, 4-byte block-relative
(engine_variant = 6), and whole rounds in LDS with a streamed tail of 1, 2 and 5 rounds.  Against the oracle, by the bars of
tests/test_gpu_line_offset.py: every energy bit-equal, best index, visible ratio and final outputs equal, poses within 1e-5 rad /
1e-4 m.  And a point of z = 0 exactly as the list's LAST point -- the one a single-round wave reads again -- with N a multiple of 512
and N = 512 k + 1: the literal-division path runs, the energies are the oracle's; without such a point it does not run.
"""
import copy
import functools

import numpy as np
import pytest

import oracle_lib
from oracle_lib import rot_angle
from test_gpu_last_sweep import _compare, _load, _same
from test_gpu_line_offset import _compact_order
from test_gpu_points_direct import _bytes_whole_list_as_4_byte_points, _pal_words, _split

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4         # bench.py: PARITY_TOLERANCE
W, H, SEED = 128, 96, 1000
ROUND = 512                             # points per round of a 256-thread workgroup
NS = (1, 64, 65, 257, 512, 513, 1025, 2048, 2049, 2241, 3585, 4097)
ITERS = (1, 2, 3)


def _wave_rounds(n):
    return [max(0, (n - off + ROUND - 1) // ROUND) for off in (0, 64, 128, 192)]


def test_list_lengths_cover_the_round_counts():
    seen = set()
    for n in NS:
        seen.update(_wave_rounds(n))
    assert seen >= {0, 1, 2, 3, 4, 5, 7, 8, 9}, sorted(seen)
    assert any(n % ROUND == 0 for n in NS) and any(n % ROUND == 1 for n in NS)


@functools.lru_cache(maxsize=None)
def _scene(n):
    """the 96 x 128 scene with exactly n reference edge pixels: the first n pixels, in the order of the engine's compact list (16 x 16
    pixel blocks, block columns first, inside a block column by column), of the image's interior -- so a chunk of 64 points spans a
    block or two, as edges do, and the list has a 4-byte form"""
    from rgbd_odometry_amd import SynthScene
    oracle = oracle_lib.load()
    sc = SynthScene(W, H, 1, SEED)
    L0 = sc.levels[0]
    rows, cols = L0.rows, L0.cols
    assert (rows, cols) == (H, W)
    xx, yy = (a.reshape(-1) for a in np.meshgrid(np.arange(8, cols - 8), np.arange(8, rows - 8)))
    pick = np.lexsort((yy, xx & 15, yy >> 4, xx >> 4))[:n]
    edge = np.zeros(rows * cols, L0.ref_edge.dtype)
    edge[yy[pick] + xx[pick] * rows] = L0.ref_edge.max()
    assert np.all(np.asarray(L0.ref_depth)[yy[pick] + xx[pick] * rows] > 0)
    sc2 = copy.copy(sc)
    sc2.levels = [copy.copy(L0)]
    sc2.levels[0].ref_edge = edge
    lv = oracle_lib.scene_levels(sc2, oracle)
    assert len(lv[0]["xyz"]) == n, (n, len(lv[0]["xyz"]))
    return sc2, lv


@functools.lru_cache(maxsize=None)
def _ref(n, n_it):
    """the oracle's alignment, computed once and shared by every launch shape and point form"""
    sc, lv = _scene(n)
    return oracle_lib.load().align_pyramid([n_it], lv, sc.intrinsics, np.eye(3), np.zeros(3))


@functools.lru_cache(maxsize=None)
def _palette(n):
    """(palette entries, partial form?) of the level as the engine builds it"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(n)
    with DvoContext(1) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        assert ctx.n_points(0) == n
        return ctx.now_compact_info(0, 0), ctx.now_compact_partial(0, 0)


def _bytes_rounds_in_lds(k, pal, partial):
    """the smallest LDS budget under which k whole rounds of 4-byte points live in LDS"""
    return (4 * (_pal_words(pal, partial) + k * ROUND + 2) + 63) & ~63


def _forms(n):
    """(name, context settings, 4-byte points?, direct?, points in LDS) of every point form this list can be read in on the 256-thread shape"""
    pal, partial = _palette(n)
    assert pal > 0
    out = [("8-byte points in LDS", dict(), False, False, n)]
    whole = _bytes_whole_list_as_4_byte_points(n, pal, partial)
    if _split(whole, n, pal, partial, 256) == (True, n):
        out.append(("4-byte direct", dict(lds_point_bytes=whole), True, True, n))
        out.append(("4-byte block-relative", dict(lds_point_bytes=whole, engine_variant=6), True, False, n))
    total = (n + ROUND - 1) // ROUND
    for tail in (1, 2, 5):
        k = total - tail
        if k < 1:
            continue
        lds = _bytes_rounds_in_lds(k, pal, partial)
        if _split(lds, n, pal, partial, 256) != (True, k * ROUND):
            continue        # budgets are multiples of 64 bytes: a tail of a few points fits into the round-up
        assert (n - k * ROUND + ROUND - 1) // ROUND == tail
        out.append(("streamed tail of %d round(s)" % tail, dict(lds_point_bytes=lds), True, True, k * ROUND))
    return out


def _run(n, kw, flags=0, want=None):
    """1, 2 and 3 iterations of the list of n points on one context, each against the oracle"""
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    sc, lv = _scene(n)
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        for n_it in ITERS:
            ref = _ref(n, n_it)
            R, t = ctx.align_batch([n_it], np.eye(3)[None], np.zeros((1, 3)), flags=DVO_FLAG_FINAL_OUTPUTS | flags)
            blk, team, packed = ctx.last_launch_shape()
            assert packed and blk == kw.get("block_threads", 512) and team == kw.get("team_size", 1), (blk, team, packed)
            assert ctx.level_texel_mode(0, 0) == 2               # the compact form is what was read
            assert not ctx.level_exact_fallback(0, 0), (n, kw, n_it)
            if want is not None:
                assert (ctx.level_points4(0, 0), ctx.level_points4_direct(0, 0)) == want, (n, kw, want)
            _compare(ctx, ref, [n_it])       # energies, best index, visible ratio, final outputs
            assert rot_angle(ref["R"], R[0]) <= ROT_TOL and np.linalg.norm(ref["t"] - t[0]) <= TRANS_TOL, (n, kw, n_it)


@pytest.mark.parametrize("n", NS)
def test_every_point_form_on_the_256_thread_shape(n):
    forms = _forms(n)
    assert len(forms) >= (3 if n >= 64 else 1), [f[0] for f in forms]
    for name, kw, pt4, direct, n_lds in forms:
        _run(n, dict(block_threads=256, **kw), want=(pt4, direct))


def test_streamed_tails_of_one_two_and_five_rounds_were_run():
    tails = set()
    for n in NS:
        tails.update(f[0] for f in _forms(n) if f[0].startswith("streamed"))
    assert len(tails) == 3, tails


@pytest.mark.parametrize("n", NS)
def test_team_of_two(n):
    """each member sweeps its share of the list (8-byte points; teams are workgroups of 512 threads: the two-deep pipeline, whose rounds
    are 1024 points); with a small budget part of each share is streamed"""
    _run(n, dict(team_size=2))
    pal, partial = _palette(n)
    _run(n, dict(team_size=2, lds_point_bytes=(4 * _pal_words(pal, partial) + 8 * (2 * ROUND + 2) + 63) & ~63))


@pytest.mark.parametrize("n", NS)
def test_with_the_normal_matrix(n):
    from rgbd_odometry_amd.capi import DVO_FLAG_NORMAL_MATRIX
    _run(n, dict(block_threads=256, team_size=1), flags=DVO_FLAG_NORMAL_MATRIX)


@pytest.mark.parametrize("n", [512, 2048, 513, 2049])
def test_degenerate_depth_as_the_last_point_of_the_list(oracle, n):
    """N = 512 k: every wave's last round is whole, and with k = 1 it is every wave's only round -- the prologue's second issue reads
    the last point again in all four waves; N = 512 k + 1: the last point is alone in wave 0's last round"""
    from rgbd_odometry_amd import DvoContext
    sc, lv = _scene(n)
    L = lv[0]
    xyz = np.asarray(L["xyz"]).reshape(-1, 3)
    last = xyz[_compact_order(sc, L)[n - 1]].astype(np.float64)          # P - cT == 0 for this point, float-exactly
    for name, kw, pt4, direct, n_lds in _forms(n)[:2]:
        with DvoContext(1, block_threads=256, **kw) as ctx:
            ctx.set_intrinsics(*sc.intrinsics)
            _load(ctx, sc, lv, "native")
            for t0, fallback in ((last, True), (np.zeros(3), False)):
                for n_it in (1, 3):                              # the residual-only sweep alone; full sweeps first
                    ref = oracle.run_iterations(0, n_it, L["xyz"], L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], sc.intrinsics, np.eye(3), t0)
                    got = ctx.run_iterations(0, n_it, np.eye(3), t0)
                    assert ctx.last_launch_shape()[:2] == (256, 1) and ctx.level_texel_mode(0, 0) == 2
                    assert (ctx.level_points4(0, 0), ctx.level_points4_direct(0, 0)) == (pt4, direct), (n, name)
                    assert ctx.level_exact_fallback(0, 0) == fallback, (n, name, n_it, fallback)
                    assert _same(ref["energy"], got["energy"]), (n, name, n_it, ref["energy"], got["energy"])
                    assert ref["best_idx"] == got["best_idx"] and ref["visible_ratio"] == got["visible_ratio"], (n, name, n_it)
                    assert _same(ref["final_eps"], got["final_eps"]) and _same(ref["final_reproj"], got["final_reproj"]), (n, name, n_it)
