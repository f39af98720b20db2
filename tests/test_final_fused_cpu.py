"""The two classes of alignments the fused final outputs of the packed kernel distinguish (rgbd_odometry_amd/csrc/dvo_fused.hip: RoundEF),
pinned on the CPU oracle alone.

The last sweep of the last level writes finalEpsilons / finalReprojections at the best of the iterates BEFORE the last one; the separate
pass over the level is skipped when that iterate is still the best after the loop ("outputs kept"), and runs when the last iterate won
(energy <= best energy, SolveDVO.cpp:696) or when no earlier iterate exists.  tests/test_gpu_final_fused.py relies on the scenes and
schedules below falling into the class stated here.
"""
import functools

import numpy as np
import pytest

import oracle_lib

# (schedule, W, H, seed, sparse, best index of the last level that runs, outputs kept?)
CASES = [
    ((10, 10, 10, 10), 160, 120, 1000, False, 7, True),
    ((10, 10, 10, 10), 320, 240, 1000, False, 8, True),
    ((10, 10, 10, 10), 320, 240, 1002, False, 1, True),       # an early best iterate
    ((10, 10, 10, 10), 160, 120, 1002, False, 9, False),      # the last iterate wins
    ((10, 10, 10, 10), 320, 240, 1004, False, 9, False),
    ((3, 0, 2, 1), 160, 120, 1000, False, 2, False),
    ((1, 1, 1, 1), 160, 120, 1000, False, 0, False),          # one iteration: no best-so-far exists
    # the sparse scene, whose level 0 gets a partial compact form: with [10, 1, 1, 1] the last iterate wins (energies ... 25.94, 30.01,
    # 22.87), one iteration fewer keeps iterate 7
    ((10, 1, 1, 1), 640, 480, 2000, True, 9, False),
    ((9, 1, 1, 1), 640, 480, 2000, True, 7, True),
]


@functools.lru_cache(maxsize=None)
def scene(W, H, seed, sparse=False):
    from rgbd_odometry_amd import SynthScene
    if sparse:          # the smallest scene of tests/test_gpu_sparse_scenes.py
        sc = SynthScene(W, H, 4, seed, n_seg=max(2, int(round(0.005 * W * H / (70.0 * W / 320.0)))), x_frac=0.5)
    else:
        sc = SynthScene(W, H, 4, seed)
    return sc, oracle_lib.scene_levels(sc, oracle_lib.load())


@functools.lru_cache(maxsize=None)
def reference(W, H, seed, iters, sparse=False):
    sc, lv = scene(W, H, seed, sparse)
    return oracle_lib.load().align_pyramid(list(iters), lv, sc.intrinsics, np.eye(3), np.zeros(3))


def kept(ref, iters):
    """the kernel's rule: an iterate before the last exists, every iteration ran, and the last one did not become the best"""
    l = ref["last_level"]
    rep = ref["levels"][l]
    return iters[l] >= 2 and rep["iters_run"] == iters[l] and 0 <= rep["best_idx"] < iters[l] - 1


@pytest.mark.parametrize("iters,W,H,seed,sparse,best,keep", CASES)
def test_class_of_the_alignment(iters, W, H, seed, sparse, best, keep):
    ref = reference(W, H, seed, iters, sparse)
    assert ref["last_level"] == 0
    rep = ref["levels"][0]
    assert rep["best_idx"] == best
    assert kept(ref, iters) == keep
    if keep:        # strictly better than the last iterate: a tie would go to the last one (:696)
        e = np.asarray(rep["energy"])
        assert e[rep["best_idx"]] < e[iters[0] - 1]


def test_last_level_is_level_one_when_level_zero_has_no_iterations():
    iters = (0, 10, 10, 10)
    ref = reference(160, 120, 1000, iters)
    assert ref["last_level"] == 1 and 0 not in ref["levels"]
    assert len(ref["levels"][1]["final_eps"]) == 533
