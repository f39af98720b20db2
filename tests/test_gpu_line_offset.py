"""The fused kernel's address of a pixel's rank words (dvo_palette.h: p4_line_offset) and its degenerate-z flag (dvo_fused.hip:
nvis_note_odd), on the GPU.

The offset is seven integer instructions now -- xx * 32 + (xx >> 2) * (column bytes - 128) + (yy + 26 (yy / 6)) * 4, counted from the
middle of the sentinel line -- and the wave's "some z is degenerate" flag rides in the top bit of its visible count.  Only integer
address arithmetic and a flag's storage changed, so nothing the caller sees may move: every energy bit-equal to the oracle's, best index
and visible ratio equal, final outputs bit for bit, poses within the bounds bench.py prints as PARITY_TOLERANCE (1e-5 rad / 1e-4 m).

Shapes are the ones where the address can go wrong: rows no multiple of 6 and cols no multiple of 4 (29 x 37, 61 x 83 with a coarser
level of 30 x 42), levels of a single tile row (5 x 9) and of a few (10 x 18, 21 x 37), 30 x 40, and 240 x 320 with 3 levels -- each on the
256-thread shape, on a team of two and with DVO_FLAG_NORMAL_MATRIX (the H-carrying instantiation).  The flag: a point of z = 0 exactly
(tests/test_gpu_packed_kernel.py::test_degenerate_depth_takes_the_exact_fallback) as the first point of a lane, as the second point only,
in the last, partial round of a wave and in a wave other than wave 0, in a full and in a residual-only sweep.  What the offset is on the
host: tests/test_line_offset_cpu.py.
"""
import functools

import numpy as np
import pytest

import oracle_lib
from oracle_lib import rot_angle
from test_gpu_last_sweep import _compare, _load, _same
from test_gpu_last_sweep import _scene as _scene4
from test_gpu_points_direct import _bytes_whole_list_as_4_byte_points, _level0

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4         # bench.py: PARITY_TOLERANCE

#: (W, H, levels) -> (rows, cols) of every level
SHAPES = {
    (37, 29, 1): [(29, 37)],
    (83, 61, 2): [(61, 83), (30, 42)],
    (37, 21, 3): [(21, 37), (10, 18), (5, 9)],         # the coarsest level is one tile row, and not a whole one
    (40, 30, 1): [(30, 40)],
    (320, 240, 3): [(240, 320), (120, 160), (60, 80)],
}
SEED = 1000


@functools.lru_cache(maxsize=None)
def _scene(W, H, n_levels):
    from rgbd_odometry_amd import SynthScene
    sc = SynthScene(W, H, n_levels, SEED)
    return sc, oracle_lib.scene_levels(sc, oracle_lib.load())


@functools.lru_cache(maxsize=None)
def _ref(W, H, n_levels):
    """the oracle's alignment of a shape, computed once and shared by the three launch shapes"""
    sc, lv = _scene(W, H, n_levels)
    return oracle_lib.load().align_pyramid([10] * n_levels, lv, sc.intrinsics, np.eye(3), np.zeros(3))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_level_sizes_are_the_ones_named(shape):
    sc, lv = _scene(*shape)
    assert [(L["rows"], L["cols"]) for L in lv] == SHAPES[shape]
    assert all(len(L["xyz"]) > 0 for L in lv), [len(L["xyz"]) for L in lv]


@pytest.mark.parametrize("launch", ["256", "team2", "normal_matrix"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_odd_level_sizes_against_the_oracle(shape, launch):
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS, DVO_FLAG_NORMAL_MATRIX
    kw = dict(team_size=2) if launch == "team2" else (dict(block_threads=256, team_size=1) if launch == "normal_matrix" else dict(block_threads=256))
    flags = DVO_FLAG_FINAL_OUTPUTS | (DVO_FLAG_NORMAL_MATRIX if launch == "normal_matrix" else 0)
    sc, lv = _scene(*shape)
    ref = _ref(*shape)
    iters = [10] * shape[2]
    with DvoContext(1, **kw) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        R, t = ctx.align_batch(iters, np.eye(3)[None], np.zeros((1, 3)), flags=flags)
        blk, team, packed = ctx.last_launch_shape()
        assert packed and team == kw.get("team_size", 1) and blk == kw.get("block_threads", blk), (blk, team, packed)
        assert [ctx.level_texel_mode(0, l) for l in range(shape[2])] == [2] * shape[2]         # the compact form is what was read
        assert not any(ctx.level_exact_fallback(0, l) for l in range(shape[2]))
        _compare(ctx, ref, iters)            # energies, best index, visible ratio, final outputs
        assert rot_angle(ref["R"], R[0]) <= ROT_TOL and np.linalg.norm(ref["t"] - t[0]) <= TRANS_TOL


def _compact_order(sc, L):
    """index in the oracle's list of the point at each position of the engine's compact list: 16 x 16 pixel blocks, block columns first,
    inside a block column by column (dvo_frames.hip: blk_entry)"""
    fx, fy, cx, cy = sc.intrinsics
    xyz = np.asarray(L["xyz"], np.float64).reshape(-1, 3)
    u, v = xyz[:, 0] / xyz[:, 2] * fx + cx, xyz[:, 1] / xyz[:, 2] * fy + cy
    xx, yy = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
    assert np.abs(u - xx).max() < 1e-2 and np.abs(v - yy).max() < 1e-2
    assert xx.min() >= 0 and xx.max() < L["cols"] and yy.min() >= 0 and yy.max() < L["rows"]
    assert len(set(zip(xx.tolist(), yy.tolist()))) == len(xx)
    return np.lexsort((yy, xx & 15, yy >> 4, xx >> 4))


def test_degenerate_depth_flag_wherever_the_point_sits(oracle):
    """one 256-thread workgroup over 3905 points in the direct 4-byte form: rounds of 512 points, lane j of a round takes positions j and
    256 + j of it, wave w the lanes 192 - 64 w .. 255 - 64 w; seven whole rounds and one of 321 points"""
    from rgbd_odometry_amd import DvoContext
    n, pal, partial = _level0(320, 240, SEED)
    assert n == 3905
    sc, lv = _scene4(320, 240, SEED)
    L = lv[0]
    order = _compact_order(sc, L)
    xyz = np.asarray(L["xyz"]).reshape(-1, 3)
    positions = {
        "first point of a lane (wave 0)": 199,
        "second point of a lane only (wave 0)": 256 + 199,
        "last, partial round of a wave (wave 2, one lane)": n - 1,
        "a wave other than wave 0 (wave 3)": 3 * 512 + 10,
    }
    assert (n - 1) // 512 == 7 and (n - 1) % 512 == 256 + 64
    with DvoContext(1, block_threads=256, lds_point_bytes=_bytes_whole_list_as_4_byte_points(n, pal, partial)) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        _load(ctx, sc, lv, "native")
        for where, pos in positions.items():
            t0 = xyz[order[pos]].astype(np.float64)          # P - cT == 0 for this point, float-exactly
            for n_it in (1, 3):                              # the residual-only sweep alone; full sweeps first
                ref = oracle.run_iterations(0, n_it, L["xyz"], L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], sc.intrinsics, np.eye(3), t0)
                got = ctx.run_iterations(0, n_it, np.eye(3), t0)
                assert ctx.last_launch_shape()[:2] == (256, 1) and ctx.level_texel_mode(0, 0) == 2 and ctx.level_points4_direct(0, 0)
                assert ctx.level_exact_fallback(0, 0), (where, n_it)
                assert _same(ref["energy"], got["energy"]), (where, n_it, ref["energy"], got["energy"])
                assert ref["best_idx"] == got["best_idx"] and ref["visible_ratio"] == got["visible_ratio"], (where, n_it)
                assert _same(ref["final_eps"], got["final_eps"]) and _same(ref["final_reproj"], got["final_reproj"]), (where, n_it)
        # and a pair without such a point: the literal-division code does not run
        for n_it in (1, 3):
            ref = oracle.run_iterations(0, n_it, L["xyz"], L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], sc.intrinsics, np.eye(3), np.zeros(3))
            got = ctx.run_iterations(0, n_it, np.eye(3), np.zeros(3))
            assert not ctx.level_exact_fallback(0, 0), n_it
            assert _same(ref["energy"], got["energy"]) and ref["visible_ratio"] == got["visible_ratio"], n_it
