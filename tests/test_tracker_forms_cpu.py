"""The inputs of tests/test_gpu_tracker_forms.py (tests/tracker_forms.py), pinned with the CPU oracle alone: a change to the frame
generator must not quietly turn the GPU tests into tests of the easy case -- the wide frames must keep a level beyond the reach of
the compact now form's ranks and one within it, the square its short lists, the pose sweep its empty, half-empty and border poses."""
import numpy as np
import pytest

import tracker_forms as F


@pytest.fixture(scope="module")
def wide(oracle):
    return [F.oracle_levels(oracle, F.wide_frame(s), F.WIDE, F.WIDE_K) for s in F.WIDE_SHIFTS]


def test_wide_frames_have_a_partial_and_a_complete_level(wide):
    for shift, levels in zip(F.WIDE_SHIFTS, wide):
        dims = [(L["rows"], L["cols"]) for L in levels]
        assert dims == [(50, 1282), (25, 641)] == [F.level_dims(F.WIDE, l) for l in range(2)]
        assert all(r % 6 and c % 4 for r, c in dims)                          # incomplete last tile row and column group on both
        far = [F.farthest_from_edges(L["edge"], L["rows"], L["cols"]) for L in levels]
        n = [len(L["xyz"]) for L in levels]
        print("shift", shift, "points", n, "farthest pixel", far)
        assert far[0] >= F.P4_RANK_REACH > far[1], far
        assert all(64 < k < 512 for k in n), n                                # more than one wave, less than one workgroup trip


def test_square_frame_lists_are_shorter_than_a_wave(oracle):
    for i, frame in enumerate(F.square_sequence()):
        levels = F.oracle_levels(oracle, frame, F.SQUARE, F.SQUARE_K)
        n = tuple(len(L["xyz"]) for L in levels)
        print("frame", i, "points", n)
        if i == 0:
            assert n == F.SQUARE_N
        assert 64 < n[0] < 128 and 6 < n[1] < 64 and 6 < n[2] < 64, n


def check_sweep(oracle, ref, now, level, K, what):
    rows, cols = now["rows"], now["cols"]
    poses, report = F.sweep(oracle, level, ref["xyz"], (now["dt"], now["gx"], now["gy"]), rows, cols, K)
    a, b, c = F.conditions(poses, report, len(ref["xyz"]))
    print(what, "N", len(ref["xyz"]), [(name, report[name]["visible"], report[name]["sides"]) for name, _, _ in poses])
    fixed = [p[0] for p in F.fixed_sweep()]
    assert len(fixed) == 14 and [p[0] for p in poses[:13]] == fixed[:13] and poses[-1][0] == fixed[-1]      # no pose is left out
    assert a and b and c, (what, a, b, c)


@pytest.mark.parametrize("level", [0, 2])
def test_sweep_conditions_at_even_geometry(oracle, level):
    """240 x 320, the sequence of tests/test_gpu_tracker_archive.py: stream 0's first frame as the key frame, its frame (3, -6) pixels
    away as the now frame"""
    import frame_gen
    geom = dict(rows=240, cols=320, nl=3, shift=0)
    ref = F.oracle_levels(oracle, frame_gen.camera_frame(900, 240, 320, shift=(0, 0), holes=True), geom, F.SQUARE_K)[level]
    now = F.oracle_levels(oracle, frame_gen.camera_frame(900, 240, 320, shift=(3, -6), holes=True), geom, F.SQUARE_K)[level]
    check_sweep(oracle, ref, now, level, F.SQUARE_K, ("even", level))


@pytest.mark.parametrize("level", [0, 1])
def test_sweep_conditions_in_the_wide_world(oracle, wide, level):
    check_sweep(oracle, wide[0][level], wide[2][level], level, F.WIDE_K, ("wide", level))


def test_aimed_rotations_are_needed_and_found(oracle, wide):
    """the wide world's points sit in the left quarter: no rotation of the fixed sweep carries one into the last column, the sweep
    must aim one there"""
    L = wide[0][0]
    poses, report = F.sweep(oracle, 0, L["xyz"], (L["dt"], L["gx"], L["gy"]), L["rows"], L["cols"], F.WIDE_K)
    fixed = [p[0] for p in F.fixed_sweep()]
    assert not any(report[n]["sides"]["last_col"] for n in fixed)
    assert any(report[p[0]]["sides"]["last_col"] for p in poses if p[0] not in fixed)
    assert len(poses) <= len(fixed) + 4 and np.array_equal(poses[-1][2], [100.0, 0.0, 0.0])


def test_far_guesses_land_on_unranked_pixels(oracle, wide):
    """at the far guesses, level 0 of the wide world is read where a partial compact form holds no rank: an alignment that starts there
    needs the level's 16-byte texels"""
    ref, now = wide[0][0], wide[2][0]
    assert len(np.unique(now["dt"])) > F.P4_PARTIAL_RANKS + 64
    R0, t0 = F.far_guesses()
    hits = [F.unranked_hits(oracle, 0, ref["xyz"], (now["dt"], now["gx"], now["gy"]), 50, 1282, F.WIDE_K, R, t) for R, t in zip(R0, t0)]
    print("points on unranked pixels at the far guesses", hits, "of", len(ref["xyz"]))
    assert all(h >= 32 for h in hits), hits
    assert F.unranked_hits(oracle, 0, ref["xyz"], (now["dt"], now["gx"], now["gy"]), 50, 1282, F.WIDE_K, np.eye(3), np.zeros(3)) == 0
