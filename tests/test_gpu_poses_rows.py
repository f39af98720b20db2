"""dvo_get_poses_rows delivers what dvo_get_poses delivers, with every rotation written row by row: the same bits, transposed --
for the whole range and for a sub-range -- and refuses the same arguments.  DvoContext.get_poses() rides on it."""
import ctypes as C

import numpy as np
import pytest

N_PAIRS = 5
ITERS = [3, 3, 3]


@pytest.fixture(scope="module")
def aligned():
    """five aligned pairs of three 160x120x3 scenes, poses resident on the device"""
    from rgbd_odometry_amd import DvoContext, SynthScene
    from rgbd_odometry_amd.capi import DVO_FLAG_IDENTITY_START
    ctx = DvoContext(N_PAIRS)
    scenes = [SynthScene(160, 120, 3, 70 + i) for i in range(3)]
    ctx.set_intrinsics(*scenes[0].intrinsics)
    for i, sc in enumerate(scenes):
        for l, L in enumerate(sc.levels):
            ctx.set_ref_level_from_images(l, L.ref_edge, L.ref_depth, L.rows, L.cols, pair=i)
            ctx.set_now_level_from_edges(l, (np.asarray(L.now_edge) != 0).astype(np.uint8) * 255, L.rows, L.cols, pair=i)
    ctx.replicate_pairs(3)
    ctx.enqueue(ITERS, flags=DVO_FLAG_IDENTITY_START)
    ctx.synchronize()
    yield ctx
    ctx.close()


def _raw(ctx, fn, first, n):
    R = np.full((n, 9), np.nan); t = np.full((n, 3), np.nan)
    rc = getattr(ctx.lib, fn)(ctx._h, first, n, R.ctypes.data, t.ctypes.data)
    return rc, R, t


@pytest.mark.gpu
@pytest.mark.parametrize("first,n", [(0, N_PAIRS), (2, 3), (4, 1)])
def test_rows_are_the_transposed_columns(aligned, first, n):
    rc_c, Rc, tc = _raw(aligned, "dvo_get_poses", first, n)
    rc_r, Rr, tr = _raw(aligned, "dvo_get_poses_rows", first, n)
    assert rc_c == 0 and rc_r == 0
    assert not np.isnan(Rc).any() and not np.isnan(Rr).any()
    assert not np.array_equal(Rc, Rr)                        # an aligned pose is no symmetric matrix
    want = np.ascontiguousarray(np.transpose(Rc.reshape(n, 3, 3), (0, 2, 1)))       # column-major -> element (i, j) at 3 i + j
    assert want.tobytes() == Rr.tobytes()
    assert tc.tobytes() == tr.tobytes()
    if first > 0:                                            # the sub-range is that part of the whole
        _, R_all, t_all = _raw(aligned, "dvo_get_poses_rows", 0, N_PAIRS)
        assert R_all[first:first + n].tobytes() == Rr.tobytes() and t_all[first:first + n].tobytes() == tr.tobytes()


@pytest.mark.gpu
def test_both_refuse_alike(aligned):
    R = np.zeros((N_PAIRS, 9)); t = np.zeros((N_PAIRS, 3))
    bad = [(-1, 1, R.ctypes.data, t.ctypes.data), (0, 0, R.ctypes.data, t.ctypes.data), (0, N_PAIRS + 1, R.ctypes.data, t.ctypes.data),
           (N_PAIRS, 1, R.ctypes.data, t.ctypes.data), (3, 3, R.ctypes.data, t.ctypes.data),
           (0, 1, None, t.ctypes.data), (0, 1, R.ctypes.data, None)]
    for first, n, pr, pt in bad:
        rc_c = aligned.lib.dvo_get_poses(aligned._h, first, n, pr, pt)
        rc_r = aligned.lib.dvo_get_poses_rows(aligned._h, first, n, pr, pt)
        assert rc_c == rc_r != 0, (first, n, pr is None, pt is None)
    assert aligned.lib.dvo_get_poses_rows(None, 0, 1, R.ctypes.data, t.ctypes.data) == aligned.lib.dvo_get_poses(None, 0, 1, R.ctypes.data, t.ctypes.data) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("first,n", [(0, None), (1, 3)])
def test_binding_returns_row_major_arrays(aligned, first, n):
    R, t = aligned.get_poses(first, n)
    n = N_PAIRS - first if n is None else n
    assert R.shape == (n, 3, 3) and t.shape == (n, 3)
    assert R.dtype == np.float64 and t.dtype == np.float64
    assert R.flags["C_CONTIGUOUS"] and t.flags["C_CONTIGUOUS"]
    _, Rc, tc = _raw(aligned, "dvo_get_poses", first, n)
    want = np.transpose(Rc.reshape(n, 3, 3), (0, 2, 1)).copy()          # what get_poses() returned before dvo_get_poses_rows
    assert want.tobytes() == R.tobytes() and tc.tobytes() == t.tobytes()
    assert np.allclose(R @ np.transpose(R, (0, 2, 1)), np.eye(3), atol=1e-9)
