"""Rows A14 / f4 on the GPU: the photometric Gauss-Newton engine behind RGBDOdometry (dvo_photo_*) against the oracle's
restatement of src/RGBDOdometry.cpp:363-746.  Everything is double precision on both sides; Eigen's products / QR are
restated, not bit-copied, so Jacobians agree to ~1e-15 relative and poses to 1e-9 (the north-star bar is 1e-5 rad / 1e-4)."""
import numpy as np
import pytest

import frame_gen
import oracle_lib
import photo_restatement as rs

pytestmark = pytest.mark.gpu

K640 = (525.0, 525.0, 319.5, 239.5)


def _pyr(oracle, bgr, depth_mm16):
    """RGBDOdometry::setRefFrame / setNowFrame (:296-357): 4 levels, INTER_NEAREST at 1, 1/2, 1/4, 1/8 of the full frame"""
    return [(oracle.bgr2gray(oracle.resize_nn(bgr, 0.5 ** l)), oracle.resize_nn(depth_mm16, 0.5 ** l)) for l in range(4)]


def _frames(seed, shift):
    bgr, depth_m = frame_gen.camera_frame(seed, 480, 640)
    bgr2, depth2_m = frame_gen.camera_frame(seed, 480, 640, shift=shift)
    to16 = lambda d: np.clip(np.nan_to_num(np.round(d * 1000.0), nan=0.0, posinf=65535, neginf=0), 1, 65535).astype(np.uint16)
    d16, d16b = to16(depth_m), to16(depth2_m)
    return (bgr, d16), (bgr2, d16b)


def _upload(ctx, frames):
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    ctx.frames_upload_cameras([f[0] for f in frames], [f[1].astype(np.float32) for f in frames], n_levels=4, first_shift=0,
                              flags=DVO_UPLOAD_DEPTH_RAW)


@pytest.mark.parametrize("fixed", [False, True])
def test_jacobians_and_normal_matrices(oracle, fixed):
    from rgbd_odometry_amd import DvoContext
    (bgr, d16), _ = _frames(3, (2, -3))
    pyr = _pyr(oracle, bgr, d16)
    with DvoContext(1) as ctx:
        _upload(ctx, [(bgr, d16)])
        for l in range(4):                                   # the store holds the node's pyramid
            grey, dep, _, _ = ctx.frame_level(0, l)
            assert np.array_equal(grey, pyr[l][0]) and np.array_equal(dep, pyr[l][1].astype(np.float32))
        ctx.photo_configure(K640, fixed=fixed)
        n = ctx.photo_set_ref(0, first_level=1)
        for l in (1, 2, 3):
            want = oracle.photo_jacobian(pyr[l][0], pyr[l][1], l, K640, fixed)
            got = ctx.photo_jacobian(l)
            assert got["n"] == want["n"] == n[l] and want["n"] > 100
            assert np.array_equal(got["sel_i"], want["sel_i"]) and np.array_equal(got["sel_j"], want["sel_j"])     # same pixels, same order
            assert np.array_equal(got["J"], want["J"])                    # identical double expressions, no contraction on either side
            np.testing.assert_allclose(got["A"], want["A"], rtol=1e-12)   # sums in another order


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("seed,shift", [(3, (2, -3)), (5, (0, 0)), (8, (-4, 1))])
def test_gauss_newton_matches_oracle(oracle, fixed, seed, shift):
    """eventLoop's per-frame work (:162-163): gaussNewtonIterations(3, T); gaussNewtonIterations(2, T)"""
    from rgbd_odometry_amd import DvoContext
    ref, now = _frames(seed, shift)
    pr, pn = _pyr(oracle, *ref), _pyr(oracle, *now)
    Tw, rep = oracle.photo_track(pr, pn, K640, fixed=fixed)
    with DvoContext(1) as ctx:
        _upload(ctx, [ref, now])
        ctx.photo_configure(K640, fixed=fixed)
        ctx.photo_set_ref(0)
        T, norms, upd = ctx.photo_align(1, np.eye(4), levels=(3, 2))
        for r, l in enumerate((3, 2)):
            assert upd[r] == rep[l]["updates"], (l, upd, rep[l])
            run = rep[l]["norms"] >= 0
            assert np.array_equal(norms[r] >= 0, run)
            assert norms[r][0] == rep[l]["norms"][0]                       # sqrt of a sum of integers: exact in any order
            np.testing.assert_allclose(norms[r][run], rep[l]["norms"][run], rtol=1e-9)
        assert np.abs(T - Tw).max() <= 1e-9 * max(1.0, np.abs(Tw).max()), np.abs(T - Tw).max()
        if shift == (0, 0):
            assert np.array_equal(T, np.eye(4)) and upd == [0, 0]          # |eps| < 200 at once: no update (:556)
        # warm start from the previous estimate, single level, more iterations
        ctx.photo_configure(K640, fixed=fixed, iterations=5)
        ctx.photo_set_ref(0)
        jac = oracle.photo_jacobian(pr[2][0], pr[2][1], 2, K640, fixed)
        T2w, n2, u2 = oracle.photo_gauss_newton(pr[2][0], pr[2][1], pn[2][0], 2, K640, jac, Tw, fixed, max_iters=5)
        T2, norms2, upd2 = ctx.photo_align(1, Tw, levels=(2,))
        assert upd2 == [u2]
        assert np.abs(T2 - T2w).max() <= 1e-8 * max(1.0, np.abs(T2w).max())


def test_photo_errors(oracle):
    from rgbd_odometry_amd import DvoContext, DvoError
    (bgr, d16), _ = _frames(3, (1, 1))
    with DvoContext(1) as ctx:
        with pytest.raises(DvoError):
            ctx.photo_align(0, np.eye(4))                        # no reference
        _upload(ctx, [(bgr, d16)])
        with pytest.raises(DvoError):
            ctx.photo_set_ref(0)                                 # camera matrix not configured
        ctx.photo_configure(K640, max_jacobian_size=200)
        with pytest.raises(DvoError):
            ctx.photo_set_ref(0)                                 # more selected pixels than const_maxJacobianSize (:464)
        ctx.photo_configure(K640, gradient_threshold=250)
        with pytest.raises(DvoError):
            ctx.photo_set_ref(0)                                 # too few points with good texture (:500)
        ctx.photo_configure(K640)
        ctx.photo_set_ref(0)
        with pytest.raises(DvoError):
            ctx.photo_align(0, np.eye(4), levels=(0,))           # level 0 has no Jacobian (:518)


# ---- shapes, levels, capacity, refusals and depth holes -------------------------------------------------------------------------
def _K(rows, cols):
    return (525.0 * cols / 640, 525.0 * cols / 640, (cols - 1) / 2.0, (rows - 1) / 2.0)


def _camera(seed, rows, cols, shift=(0, 0), holes=False):
    bgr, depth_m = frame_gen.camera_frame(seed, rows, cols, shift=shift, holes=holes)
    d = np.nan_to_num(np.round(depth_m * 1000.0), nan=0.0, posinf=65535, neginf=0)
    return bgr, (np.clip(d, 0 if holes else 1, 65535)).astype(np.uint16)


def _same_matrix(got, want, rtol):
    """equal where not finite (NaN, +-inf: equal_nan), rtol relative to the largest finite entry elsewhere"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(np.where(fin, 0.0, got), np.where(fin, 0.0, want), equal_nan=True)
    if fin.any():
        scale = np.abs(want[fin]).max()
        assert np.abs(got[fin] - want[fin]).max() <= rtol * scale, (np.abs(got[fin] - want[fin]).max(), scale)


def _check_jacobian(ctx, oracle, grey, dep, level, K, fixed, thr=5, cap=50000):
    want = oracle.photo_jacobian(grey, dep, level, K, fixed, grad_threshold=thr, capacity=cap)
    got = ctx.photo_jacobian(level, capacity=cap)
    assert got["n"] == want["n"], (level, got["n"], want["n"])
    assert np.array_equal(got["sel_i"], want["sel_i"]) and np.array_equal(got["sel_j"], want["sel_j"])
    assert np.array_equal(got["J"], want["J"], equal_nan=True)
    _same_matrix(got["A"], want["A"], 1e-12)
    return want


def _oracle_align(oracle, pr, pn, K, levels, T0, fixed, iters, thr=5, cap=50000):
    T, runs = np.array(T0, np.float64), []
    for l in levels:
        jac = oracle.photo_jacobian(pr[l][0], pr[l][1], l, K, fixed, grad_threshold=thr, capacity=cap)
        T, norms, u = oracle.photo_gauss_newton(pr[l][0], pr[l][1], pn[l][0], l, K, jac, T, fixed, max_iters=iters)
        runs.append((norms, u))
    return T, runs


def _check_align(ctx, oracle, pr, pn, K, levels, fixed, iters, T0=None, thr=5, cap=50000, now_slot=1):
    T0 = np.eye(4) if T0 is None else T0
    Tw, runs = _oracle_align(oracle, pr, pn, K, levels, T0, fixed, iters, thr, cap)
    T, norms, upd = ctx.photo_align(now_slot, T0, levels=levels)
    assert norms.shape == (len(levels), iters)
    for r, (wn, wu) in enumerate(runs):
        assert upd[r] == wu, (levels, r, upd, wu)
        assert np.array_equal(norms[r] >= 0, wn >= 0)
        assert norms[r][0] == wn[0]                                        # first |eps| of every level run: exact
        np.testing.assert_allclose(norms[r], wn, rtol=1e-9)
    assert np.isfinite(T).all() == np.isfinite(Tw).all()
    if np.isfinite(Tw).all():
        assert np.abs(T - Tw).max() <= 1e-9 * max(1.0, np.abs(Tw).max()), np.abs(T - Tw).max()
    return T


def _store_matches(ctx, oracle, pyr, slot=0):
    for l in range(4):
        grey, dep, _, _ = ctx.frame_level(slot, l)
        assert np.array_equal(grey, pyr[l][0]) and np.array_equal(dep, pyr[l][1].astype(np.float32))


# (rows, cols, gradient_threshold): 72 x 9 has levels 36 x 4 (round-half-even of 4.5), 18 x 2 and 9 x 1
@pytest.mark.parametrize("rows,cols,thr", [(481, 641, 5), (250, 330, 5), (97, 131, 5), (72, 9, 0), (40, 13, -2)])
@pytest.mark.parametrize("fixed", [False, True])
def test_odd_and_tiny_shapes(oracle, rows, cols, thr, fixed):
    from rgbd_odometry_amd import DvoContext
    K = _K(rows, cols)
    ref, now = _camera(7, rows, cols), _camera(7, rows, cols, shift=(2, -1))
    pr, pn = _pyr(oracle, *ref), _pyr(oracle, *now)
    with DvoContext(1) as ctx:
        _upload(ctx, [ref, now])
        _store_matches(ctx, oracle, pr)
        ctx.photo_configure(K, fixed=fixed, gradient_threshold=thr, min_required_pts=2)
        n = ctx.photo_set_ref(0, first_level=1)
        for l in (1, 2, 3):
            assert _check_jacobian(ctx, oracle, pr[l][0], pr[l][1], l, K, fixed, thr)["n"] == n[l]
        for levels in ((1, 2, 3), (3, 2), (2, 3, 1), (1,)):
            _check_align(ctx, oracle, pr, pn, K, levels, fixed, 3, thr=thr)
        cap = rows * cols + 1                                              # level 0: every pixel may be selected
        ctx.photo_configure(K, fixed=fixed, gradient_threshold=thr, min_required_pts=2, max_jacobian_size=cap)
        n = ctx.photo_set_ref(0, first_level=0)
        for l in range(4):
            assert _check_jacobian(ctx, oracle, pr[l][0], pr[l][1], l, K, fixed, thr, cap)["n"] == n[l]
        # Gauss-Newton from level 0 on frames of 64 pixels and more per side: the 72 x 9 frame's level-0 and level-1 normal matrices
        # have condition numbers near 1e13, where scaling A by (1 + 1e-15) alone moves the oracle's T by 2e-9 relative
        if min(rows, cols) >= 64:
            _check_align(ctx, oracle, pr, pn, K, (0, 1), fixed, 3, thr=thr, cap=cap)


@pytest.mark.parametrize("fixed", [False, True])
def test_level_wider_than_1024_columns(oracle, fixed):
    """1200 x 2112: level 1 is 600 x 1056, so the single-workgroup scan takes two columns per thread and the row count is not a
    multiple of 64; Gauss-Newton at level 1 over all its points"""
    from rgbd_odometry_amd import DvoContext
    rows, cols, cap = 1200, 2112, 400000
    K = _K(rows, cols)
    ref, now = _camera(12, rows, cols), _camera(12, rows, cols, shift=(-3, 4))
    pr, pn = _pyr(oracle, *ref), _pyr(oracle, *now)
    assert pr[1][0].shape == (600, 1056)
    with DvoContext(1) as ctx:
        _upload(ctx, [ref, now])
        ctx.photo_configure(K, fixed=fixed, max_jacobian_size=cap)
        n = ctx.photo_set_ref(0, first_level=1)
        for l in (1, 2, 3):
            assert _check_jacobian(ctx, oracle, pr[l][0], pr[l][1], l, K, fixed, cap=cap)["n"] == n[l]
        assert n[1] > 1024
        _check_align(ctx, oracle, pr, pn, K, (1,), fixed, 3, cap=cap)
        _check_align(ctx, oracle, pr, pn, K, (3, 2, 1), fixed, 3, cap=cap)


def test_iteration_budget(oracle):
    """it x n_run <= 64 norms fit the engine's buffer: 21 x 3 and 32 x 2 run, 33 x 2 is refused"""
    from rgbd_odometry_amd import DvoContext, DvoError
    ref, now = _frames(8, (-4, 1))
    pr, pn = _pyr(oracle, *ref), _pyr(oracle, *now)
    with DvoContext(1) as ctx:
        _upload(ctx, [ref, now])
        for it, levels in ((21, (1, 2, 3)), (32, (2, 1))):
            ctx.photo_configure(K640, iterations=it)
            ctx.photo_set_ref(0)
            _check_align(ctx, oracle, pr, pn, K640, levels, False, it)
        ctx.photo_configure(K640, iterations=33)
        ctx.photo_set_ref(0)
        with pytest.raises(DvoError):
            ctx.photo_align(1, np.eye(4), levels=(3, 2))
        _check_align(ctx, oracle, pr, pn, K640, (1,), False, 33)


def _capacity_outcome(fn):
    try:
        return fn()
    except (RuntimeError, rs.CapacityAssert):
        return None


def test_capacity_boundary(oracle):
    """:464 asserts before every scanned pixel: at level 1, n - 1 and n are refused, n + 1 is accepted; when the last scanned
    pixel (rows-1, cols-1) is selected, n itself is accepted.  GPU, oracle and restatement give the same answer."""
    from rgbd_odometry_amd import DvoContext, DvoError
    (bgr, d16), _ = _frames(3, (0, 0))
    bgr_last = bgr.copy()
    r, c = 2 * (240 - 1), 2 * (320 - np.arange(3, 0, -1))           # level 1 samples the full frame at (2i, 2j) (INTER_NEAREST)
    bgr[r, c] = np.array([0, 90, 200], np.uint8)[:, None]           # last row of level 1 ends 0, 90, 200: gx = 90, 110, -110
    bgr_last[r, c] = np.array([0, 200, 90], np.uint8)[:, None]      # 0, 200, 90: gx = 200, -110, 110 (reflect-101)
    p, p_last = _pyr(oracle, bgr, d16), _pyr(oracle, bgr_last, d16)
    g, g_last, dep = p[1][0], p_last[1][0], p[1][1]
    assert list(g[-1, -3:]) == [0, 90, 200] and list(g_last[-1, -3:]) == [0, 200, 90]
    n = rs.photo_jacobian(g, dep, 1, K640)["n"]
    assert rs.photo_jacobian(g_last, dep, 1, K640)["n"] == n
    cases = [(0, n - 1, False), (0, n, False), (0, n + 1, True), (1, n, True)]
    with DvoContext(1) as ctx:
        _upload(ctx, [(bgr, d16), (bgr_last, d16)])
        for slot, cap, ok in cases:
            img = (g, g_last)[slot]
            want = _capacity_outcome(lambda: rs.photo_jacobian(img, dep, 1, K640, capacity=cap))
            orc = _capacity_outcome(lambda: oracle.photo_jacobian(img, dep, 1, K640, capacity=cap))
            ctx.photo_configure(K640, max_jacobian_size=cap)
            try:
                sel = ctx.photo_set_ref(slot)
                gpu_ok = True
            except DvoError:
                gpu_ok = False
            assert (want is not None, orc is not None, gpu_ok) == (ok, ok, ok), (slot, cap, n)
            if ok:
                assert sel[1] == n
                _check_jacobian(ctx, oracle, img, dep, 1, K640, False, cap=cap)


def test_refusals_change_nothing(oracle):
    """a refused dvo_photo_set_ref leaves the previous reference in force: refused at the coarsest level after the finer ones
    passed, and refused at its first level"""
    from rgbd_odometry_amd import DvoContext, DvoError
    ref, now = _frames(3, (2, -3))
    rng = np.random.default_rng(5)
    patch = np.full((480, 640, 3), 128, np.uint8)                    # flat grey with one 96 x 96 noise patch
    patch[200:296, 300:396] = rng.integers(0, 256, (96, 96, 1), dtype=np.uint8)
    flat = np.full((480, 640, 3), 128, np.uint8)                     # no texture: refused at its first level
    pr, pp = _pyr(oracle, *ref), _pyr(oracle, patch, ref[1])
    n_ref = [oracle.photo_jacobian(pr[l][0], pr[l][1], l, K640)["n"] for l in range(4)]
    n_patch = [oracle.photo_jacobian(pp[l][0], pp[l][1], l, K640)["n"] for l in range(4)]
    m = n_patch[3]                                                   # min_required_pts: the patch passes at levels 1, 2 only
    assert n_patch[1] > m and n_patch[2] > m and min(n_ref[1:]) > m
    with DvoContext(1) as ctx:
        _upload(ctx, [ref, now, (patch, ref[1]), (flat, ref[1])])
        ctx.photo_configure(K640, min_required_pts=m)
        ctx.photo_set_ref(0)
        T0 = ctx.photo_align(1, np.eye(4), levels=(3, 2))
        T1 = ctx.photo_align(1, np.eye(4), levels=(2,))
        jac0 = [ctx.photo_jacobian(l) for l in (1, 2, 3)]
        for slot in (2, 3):
            with pytest.raises(DvoError):
                ctx.photo_set_ref(slot)
            for got, want in ((ctx.photo_align(1, np.eye(4), levels=(3, 2)), T0), (ctx.photo_align(1, np.eye(4), levels=(2,)), T1)):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
            for l, want in zip((1, 2, 3), jac0):
                got = ctx.photo_jacobian(l)
                assert all(np.array_equal(got[k], want[k]) for k in ("J", "sel_i", "sel_j", "A", "n")), (slot, l)


@pytest.mark.parametrize("fixed", [False, True])
def test_depth_holes(oracle, fixed):
    """raw depth with zeros (holes) at selected pixels: the rows of J there hold inf / NaN as the reference computes them, and the
    GPU agrees with the oracle on J, A (NaN / inf in place) and on whether T stays finite"""
    from rgbd_odometry_amd import DvoContext
    ref, now = _camera(3, 480, 640, holes=True), _camera(3, 480, 640, shift=(2, -3), holes=True)
    pr, pn = _pyr(oracle, *ref), _pyr(oracle, *now)
    holes = 0
    with DvoContext(1) as ctx:
        _upload(ctx, [ref, now])
        _store_matches(ctx, oracle, pr)
        ctx.photo_configure(K640, fixed=fixed)
        ctx.photo_set_ref(0)
        for l in (1, 2, 3):
            jac = _check_jacobian(ctx, oracle, pr[l][0], pr[l][1], l, K640, fixed)
            holes += int(np.count_nonzero(pr[l][1][jac["sel_i"], jac["sel_j"]] == 0))
        T = _check_align(ctx, oracle, pr, pn, K640, (3, 2), fixed, 3)
        _check_align(ctx, oracle, pr, pn, K640, (1,), fixed, 3)
    assert holes > 0 and not np.isfinite(T).all()
