"""CPU properties of the photometric Gauss-Newton oracle (oracle/dvo_oracle_photo.cpp; RGBDOdometry.cpp:363-746)."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import frame_gen
import photo_restatement as rs

K = (525.0, 525.0, 319.5, 239.5)


def _pyr(oracle, bgr, d16):
    return [(oracle.bgr2gray(oracle.resize_nn(bgr, 0.5 ** l)), oracle.resize_nn(d16, 0.5 ** l)) for l in range(4)]


def test_solver_and_exponential_map(oracle):
    rng = np.random.default_rng(0)
    for _ in range(50):
        A = rng.standard_normal((40, 6)); A = A.T @ A
        b = rng.standard_normal(6)
        np.testing.assert_allclose(oracle.photo_solve6(A, b), np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)
    # rank-deficient: colPivHouseholderQr's basic solution (free components zero) still satisfies A x = b for consistent b
    A = np.zeros((6, 6)); A[:3, :3] = np.diag([4.0, 2.0, 1.0])
    x = oracle.photo_solve6(A, np.array([4.0, 2.0, 1.0, 0, 0, 0]))
    np.testing.assert_allclose(x, [1, 1, 1, 0, 0, 0], atol=1e-14)
    psi = np.array([1.0, -2.0, 0.5, 0.01, -0.02, 0.03])
    E = oracle.photo_exponential_map(psi)
    np.testing.assert_allclose(E[:3, :3], Rotation.from_rotvec(psi[3:]).as_matrix(), atol=1e-15)
    assert np.array_equal(E[3], [0, 0, 0, 1])
    # defect D7 (:727-731): a pure translation is dropped unless fixed
    assert np.array_equal(oracle.photo_exponential_map([1, 2, 3, 0, 0, 0]), np.eye(4))
    np.testing.assert_allclose(oracle.photo_exponential_map([1, 2, 3, 0, 0, 0], fixed=True)[:3, 3], [1, 2, 3])


def test_jacobian_definition_and_defects(oracle):
    bgr, depth = frame_gen.camera_frame(3, 480, 640)
    d16 = np.clip(np.nan_to_num(np.round(depth * 1000.0), nan=0.0, posinf=65535, neginf=0), 1, 65535).astype(np.uint16)
    grey, dep = _pyr(oracle, bgr, d16)[2]
    jac = oracle.photo_jacobian(grey, dep, 2, K)
    rows, cols = grey.shape
    g = grey.astype(np.float64)
    gx = np.empty_like(g); gx[:, :-1] = g[:, 1:] - g[:, :-1]; gx[:, -1] = g[:, -2] - g[:, -1]          # [0 -1 1], reflect-101
    gy = np.empty_like(g); gy[:-1] = g[1:] - g[:-1]; gy[-1] = g[-2] - g[-1]
    sel = np.argwhere((gx >= 5).T)                     # column-major scan: (j, i) pairs in order
    assert jac["n"] == len(sel) and np.array_equal(jac["sel_j"], sel[:, 0]) and np.array_equal(jac["sel_i"], sel[:, 1])
    i, j = jac["sel_i"], jac["sel_j"]
    Z = dep[i, j].astype(np.float64)
    fx, fy, cx, cy = K
    np.testing.assert_allclose(jac["J"][:, 0], fx * fx / Z, rtol=1e-15)                               # D1 reproduced
    np.testing.assert_allclose(jac["J"][:, 1], fy * gy[i, j] / Z, rtol=1e-15)
    np.testing.assert_allclose(jac["A"], jac["J"].T @ jac["J"], rtol=1e-12)
    fixed = oracle.photo_jacobian(grey, dep, 2, K, fixed=True)
    s = 0.25
    np.testing.assert_allclose(fixed["J"][:, 0], (fx * s) * gx[i, j] / Z, rtol=1e-15)                 # D1 + D4 corrected


def test_identical_frames_stop_at_once(oracle):
    bgr, depth = frame_gen.camera_frame(4, 480, 640)
    d16 = np.clip(np.nan_to_num(np.round(depth * 1000.0), nan=0.0, posinf=65535, neginf=0), 1, 65535).astype(np.uint16)
    pyr = _pyr(oracle, bgr, d16)
    T, rep = oracle.photo_track(pyr, pyr, K)
    assert np.array_equal(T, np.eye(4))
    for l in (3, 2):
        assert rep[l]["updates"] == 0 and rep[l]["norms"][0] < 200 and rep[l]["norms"][1] == -1      # :556


# ---- the oracle pinned to an independent restatement (tests/photo_restatement.py) --------------------------------------------
def _to16(depth_m):
    return np.clip(np.nan_to_num(np.round(depth_m * 1000.0), nan=0.0, posinf=65535, neginf=0), 1, 65535).astype(np.uint16)


def _pair(oracle, seed, shift, rows=480, cols=640):
    bgr, d = frame_gen.camera_frame(seed, rows, cols)
    bgr2, d2 = frame_gen.camera_frame(seed, rows, cols, shift=shift)
    return _pyr(oracle, bgr, _to16(d)), _pyr(oracle, bgr2, _to16(d2))


def _same_jacobian(got, want):
    assert got["n"] == want["n"]
    assert np.array_equal(got["sel_i"], want["sel_i"]) and np.array_equal(got["sel_j"], want["sel_j"])
    assert np.array_equal(got["J"], want["J"])                                   # the same expressions in the same order
    np.testing.assert_allclose(got["A"], want["A"], rtol=1e-12, atol=1e-12 * np.abs(want["A"]).max())


def _same_gauss_newton(oracle, ref, now, level, jac, T0, fixed, iters):
    """oracle and restatement from T0: eps of the first iteration and its norm exactly, the rest to 1e-9 relative"""
    eps_o, n0_o = oracle.photo_epsilon(ref[0], ref[1], now[0], level, K, jac, T0, fixed)
    To, no, uo = oracle.photo_gauss_newton(ref[0], ref[1], now[0], level, K, jac, T0, fixed, max_iters=iters)
    Tr, nr, ur, eps_r = rs.photo_gauss_newton(ref[0], ref[1], now[0], level, K, jac, T0, fixed, max_iters=iters)
    assert np.array_equal(eps_o, eps_r)                          # differences of two u8 values, or 0
    assert n0_o == no[0] == nr[0]                                # sqrt of a sum of integers: exact in any order
    assert uo == ur
    assert np.array_equal(no >= 0, nr >= 0)
    np.testing.assert_allclose(no, nr, rtol=1e-9)
    assert np.abs(To - Tr).max() <= 1e-9 * max(1.0, np.abs(Tr).max()), np.abs(To - Tr).max()
    return To, no, uo


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (5, 2), (2, 9), (13, 11)])
@pytest.mark.parametrize("thr", [-300, 0, 5])
def test_borders_and_tiny_images_match_restatement(oracle, shape, thr):
    """filter2D's BORDER_REFLECT_101 on every edge, a length-1 axis (OpenCV maps it to index 0) and length 2; thr = -300 selects
    every pixel, so every border case is in J"""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    grey = rng.integers(0, 256, shape).astype(np.uint8)
    dep = rng.integers(500, 4000, shape).astype(np.uint16)
    for level in (1, 3):
        for fixed in (False, True):
            want = rs.photo_jacobian(grey, dep, level, K, fixed, grad_threshold=thr)
            _same_jacobian(oracle.photo_jacobian(grey, dep, level, K, fixed, grad_threshold=thr), want)
            if thr == -300:
                assert want["n"] == grey.size
    assert np.array_equal(rs.reflect101(np.array([-1, 0, 1]), 1), [0, 0, 0])
    assert np.array_equal(rs.reflect101(np.array([-1, 2]), 2), [1, 0])


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("seed,shift", [(3, (2, -3)), (8, (-4, 1)), (11, (6, 5)), (21, (0, 3))])
def test_oracle_matches_restatement(oracle, seed, shift, fixed):
    """computeJacobian, computeEpsilon and gaussNewtonIterations at levels 1, 2 and 3: the reference's 3 iterations and a longer
    run of 8 without the |eps| < 200 stop"""
    pr, pn = _pair(oracle, seed, shift)
    for level in (1, 2, 3):
        jac = oracle.photo_jacobian(pr[level][0], pr[level][1], level, K, fixed)
        _same_jacobian(jac, rs.photo_jacobian(pr[level][0], pr[level][1], level, K, fixed))
        T, _, _ = _same_gauss_newton(oracle, pr[level], pn[level], level, jac, np.eye(4), fixed, 3)
        eps_o, _ = oracle.photo_epsilon(pr[level][0], pr[level][1], pn[level][0], level, K, jac, T, fixed)
        eps_r, _, _ = rs.photo_epsilon(pr[level][0], pr[level][1], pn[level][0], level, K, jac, T, fixed)
        assert np.count_nonzero(eps_o != eps_r) <= 1                # T agrees to ~1e-15, a floor() may fall either way
        To, no, uo = oracle.photo_gauss_newton(pr[level][0], pr[level][1], pn[level][0], level, K, jac, np.eye(4), fixed,
                                               max_iters=8, eps_stop=0.0)
        Tr, nr, ur, _ = rs.photo_gauss_newton(pr[level][0], pr[level][1], pn[level][0], level, K, jac, np.eye(4), fixed,
                                              max_iters=8, eps_stop=0.0)
        assert uo == ur == 8 and no[0] == nr[0]
        np.testing.assert_allclose(no, nr, rtol=1e-9)
        assert np.abs(To - Tr).max() <= 1e-9 * max(1.0, np.abs(Tr).max())


T_FAR = np.eye(4)
T_FAR[:3, :3] = Rotation.from_rotvec([1.11, 0.54, 0.1]).as_matrix()
T_FAR[:3, 3] = [-892.0, -1357.0, 1880.0]                        # mm, like the depth (D5)


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("seed", [3, 11])
def test_far_start_pose(oracle, seed, fixed):
    """a start pose that turns by 70 degrees and moves nearly 2.5 m: most points leave the image (eps 0, :683) and some land
    behind the camera (out(2) <= 0, projected through a negative depth)"""
    pr, pn = _pair(oracle, seed, (2, -3))
    updated = 0
    for level in (1, 2, 3):
        jac = oracle.photo_jacobian(pr[level][0], pr[level][1], level, K, fixed)
        eps, _, o2 = rs.photo_epsilon(pr[level][0], pr[level][1], pn[level][0], level, K, jac, T_FAR, fixed)
        assert np.count_nonzero(o2 <= 0) > 0 and np.count_nonzero(eps == 0) > jac["n"] // 2
        _, _, u = _same_gauss_newton(oracle, pr[level], pn[level], level, jac, T_FAR, fixed, 3)
        updated += u
    assert updated > 0


@pytest.mark.parametrize("fixed", [False, True])
def test_pure_translation_step(oracle, fixed):
    """D7 inside gaussNewtonIterations: with the rotation columns of J zero, the rank-3 solve leaves w = 0 exactly, so every step is
    a pure translation -- the reference's exponentialMap drops it (T stays put, yet each iteration counts), fixed applies it"""
    pr, pn = _pair(oracle, 8, (-4, 1))
    level = 2
    jac = oracle.photo_jacobian(pr[level][0], pr[level][1], level, K, fixed)
    J = jac["J"].copy()
    J[:, 3:] = 0.0
    jt = dict(jac, J=J, A=J.T @ J)
    psi = rs.solve_colpiv_qr(jt["A"], -J.T @ rs.photo_epsilon(pr[level][0], pr[level][1], pn[level][0], level, K, jt, np.eye(4), fixed)[0])
    assert np.array_equal(psi[3:], [0.0, 0.0, 0.0]) and np.abs(psi[:3]).max() > 0
    np.testing.assert_allclose(oracle.photo_solve6(jt["A"], -J.T @ rs.photo_epsilon(pr[level][0], pr[level][1], pn[level][0], level, K, jt,
                                                                                       np.eye(4), fixed)[0]), psi, rtol=1e-9)
    T, norms, upd = _same_gauss_newton(oracle, pr[level], pn[level], level, jt, np.eye(4), fixed, 3)
    assert upd == 3
    assert np.array_equal(T[:3, :3], np.eye(3))
    if fixed:
        assert np.abs(T[:3, 3]).max() > 0
    else:
        assert np.array_equal(T, np.eye(4)) and norms[0] == norms[1] == norms[2]
    for f in (False, True):
        np.testing.assert_array_equal(oracle.photo_exponential_map([3.0, -1.0, 2.0, 0, 0, 1e-13], fixed=f),
                                      rs.exponential_map([3.0, -1.0, 2.0, 0, 0, 1e-13], fixed=f))


def _capacity_outcome(fn):
    try:
        return fn()
    except (RuntimeError, rs.CapacityAssert):
        return None


def test_capacity_rule(oracle):
    """:464 asserts xc < const_maxJacobianSize before every scanned pixel: n == cap passes only when the cap-th selected pixel is the
    last pixel scanned, (rows-1, cols-1); n > cap never passes"""
    pr, _ = _pair(oracle, 3, (0, 0))
    grey, dep = pr[2][0].copy(), pr[2][1]
    rows, cols = grey.shape
    grey[rows - 1, cols - 3:] = 0, 90, 200        # gx along the last row (reflect-101 at the end): 90, 110, -110
    n = rs.photo_jacobian(grey, dep, 2, K)["n"]
    last = grey.copy()
    last[rows - 1, cols - 3:] = 0, 200, 90        # 200, -110, 110: the last scanned pixel is selected
    n_last = rs.photo_jacobian(last, dep, 2, K)["n"]
    assert n_last == n
    cases = [(grey, n - 1, False), (grey, n, False), (grey, n + 1, True), (last, n_last, True), (last, n_last - 1, False)]
    for img, cap, ok in cases:
        got = _capacity_outcome(lambda: oracle.photo_jacobian(img, dep, 2, K, capacity=cap))
        want = _capacity_outcome(lambda: rs.photo_jacobian(img, dep, 2, K, capacity=cap))
        assert (got is not None) == (want is not None) == ok, (cap, n, got is not None, want is not None)
        if ok:
            _same_jacobian(got, want)
            assert got["n"] == (n if img is grey else n_last)
