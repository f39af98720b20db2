"""Scenes that do not flatter the engine (round 5): 0.5 - 2 % edge pixels, all in the left half of the frame, so
that the right half is hundreds of pixels from every edge (many distinct distances; at 1920x1080 and beyond, pixels 512 px or more
from every edge).  Rounds 3-4 refused such levels (16-byte texels for every look-up); since round 5 they get a PARTIAL compact form
(dvo_palette.h).  Whatever form each level ends up in, the results are the oracle's: energies / best index / visible ratio bit-equal,
pose within 1e-5 rad / 1e-4 m, final outputs bit-equal.  (`bench.py --full`'s `sparse_scenes` leg measures the same scenes at batch size.)"""
import numpy as np
import pytest

import oracle_lib
from oracle_lib import rot_angle

pytestmark = pytest.mark.gpu


def _u8(a):
    return (np.asarray(a) != 0).astype(np.uint8) * 255


@pytest.mark.parametrize("W,H,nl,dens", [(640, 480, 4, 0.005), (640, 480, 4, 0.02), (1920, 1080, 5, 0.005), (1920, 1080, 5, 0.02),
                                         (4096, 3072, 5, 0.01)])
def test_sparse_scene_matches_the_oracle_in_whatever_form_its_levels_get(oracle, W, H, nl, dens):
    from rgbd_odometry_amd import DvoContext, SynthScene
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS
    n_seg = max(2, int(round(dens * W * H / (70.0 * W / 320.0))))
    sc = SynthScene(W, H, nl, 2000, n_seg=n_seg, x_frac=0.5)
    e0 = (np.asarray(sc.levels[0].now_edge) != 0).reshape(sc.levels[0].cols, sc.levels[0].rows)
    assert not e0[int(0.55 * W):].any() and 0.3 * dens < e0.mean() < 1.5 * dens      # the right 45 % of the columns are empty
    lv = oracle_lib.scene_levels(sc, oracle)
    iters = [10] * nl
    ref = oracle.align_pyramid(iters, lv, sc.intrinsics, np.eye(3), np.zeros(3))
    with DvoContext(1) as ctx:
        ctx.set_intrinsics(*sc.intrinsics)
        for l, L in enumerate(sc.levels):
            xyz, _ = ctx.set_ref_level_from_images(l, L.ref_edge, L.ref_depth, L.rows, L.cols)
            assert len(xyz) == len(lv[l]["xyz"])
            ctx.set_now_level_from_edges(l, _u8(L.now_edge), L.rows, L.cols)
        info = [ctx.now_compact_info(0, l) for l in range(nl)]
        part = [ctx.now_compact_partial(0, l) for l in range(nl)]
        R, t = ctx.align_batch(iters, np.eye(3)[None], np.zeros((1, 3)), flags=DVO_FLAG_FINAL_OUTPUTS)
        modes = [ctx.level_texel_mode(0, l) for l in range(nl)]
        # round 5: no level is refused any more -- what the form cannot express (rounds 3-4: -2 too many distances, -3 a rank step,
        # -7 a far pixel) makes it PARTIAL, and the launch reads the compact form on every level
        assert all(v > 0 for v in info) and modes == [2] * nl, (info, part, modes)
        assert part[0] and not part[nl - 1], (info, part)                       # level 0 of these scenes is partial, the coarsest never
        for l, rep in ref["levels"].items():
            e, b, ratio = ctx.level_report(0, l, iters[l])
            assert np.array_equal(e, rep["energy"]) and b == rep["best_idx"] and ratio == rep["visible_ratio"], (l, info)
        assert rot_angle(ref["R"], R[0]) <= 1e-5 and np.linalg.norm(ref["t"] - t[0]) <= 1e-4
        last = ref["levels"][ref["last_level"]]
        feps, frep = ctx.final_outputs(0, len(last["final_eps"]))
        assert np.array_equal(feps, last["final_eps"]) and np.array_equal(frep, last["final_reproj"], equal_nan=True)
        # the images themselves, decoded from whatever form they are in
        for l in (0, nl - 1):
            dt, gx, gy = ctx.get_now_level(l)
            assert np.array_equal(dt, lv[l]["dt"]) and np.array_equal(gx, lv[l]["gx"]) and np.array_equal(gy, lv[l]["gy"]), l
