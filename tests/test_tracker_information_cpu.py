"""CPU checks of the tracker's pose information (include/dvo_amd.h: dvo_tracker_set_information / dvo_tracker_get_information): the
header, the binding and the library agree on the two calls, and the covariance helper of the C++ mirror (dvo_amd::poseCovariance,
include/dvo_amd.hpp) computes C = s^2 H^-1, s^2 = sum_eps2 / (n_visible - 6) -- as does its Python twin."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvo_tracker_set_information", "dvo_tracker_get_information"]

PROGRAM = r"""
#include <cstdio>
#include "dvo_amd.hpp"
int main() {
    double H[36], C[36], e2;
    int n;
    for (int k = 0; k < 36; k++) if (std::scanf("%lf", &H[k]) != 1) return 2;
    if (std::scanf("%lf %d", &e2, &n) != 2) return 2;
    for (int k = 0; k < 36; k++) C[k] = -7.0;
    const bool ok = dvo_amd::poseCovariance(H, e2, n, C);
    std::printf("%d\n", ok ? 1 : 0);
    for (int k = 0; k < 36; k++) std::printf("%.17g\n", C[k]);
    return 0;
}
"""


def spd_matrix():
    """a fixed symmetric positive definite 6 x 6 matrix with the spread of a pose information matrix (translations against rotations)"""
    rng = np.random.default_rng(7)
    A = rng.standard_normal((40, 6)) * np.array([30.0, 25.0, 8.0, 300.0, 350.0, 120.0])
    return A.T @ A


def test_header_library_and_binding_have_the_calls():
    from rgbd_odometry_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dvo_[a-z0-9_]+)\s*\(", src))
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared and name in capi.C_ABI_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("set_information", "information", "covariance"):
        assert callable(getattr(capi.DvoTracker, name)), name
    hpp = open(os.path.join(ROOT, "include", "dvo_amd.hpp")).read()
    for name in ("void enableInformation(bool", "lastInformation(int", "inline bool poseCovariance(const double H36[36], double sum_eps2, int n_visible, double C36[36])"):
        assert name in hpp, name
    # refused before anything is touched
    assert lib.dvo_tracker_set_information(None, 1) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_get_information(None, 0, None, None, None, None, None) == capi.DVO_ERR_INVALID


def test_pose_covariance_host_helper(tmp_path):
    """dvo_amd::poseCovariance compiled into a small host program: a fixed SPD matrix against s^2 numpy.linalg.inv(H); false, C
    untouched, for a singular H and for n_visible = 6"""
    from rgbd_odometry_amd import capi
    src, exe = tmp_path / "cov.cpp", tmp_path / "cov"
    src.write_text(PROGRAM)
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", lib, "-ldvo_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def call(H, e2, n):
        text = " ".join(repr(float(x)) for x in np.asarray(H).ravel()) + " %r %d\n" % (float(e2), n)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        v = out.stdout.split()
        return v[0] == "1", np.array([float(x) for x in v[1:]]).reshape(6, 6)

    H, e2, n = spd_matrix(), 1234.5, 4321
    want = (e2 / (n - 6)) * np.linalg.inv(H)
    ok, C = call(H, e2, n)
    assert ok
    assert np.abs(C - want).max() <= 1e-10 * np.abs(want).max(), np.abs(C - want).max() / np.abs(want).max()
    np.testing.assert_allclose(C, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
    assert np.array_equal(C, C.T)
    # the Python helper: the same formula
    P = capi.pose_covariance(H, e2, n)
    np.testing.assert_allclose(P, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
    np.testing.assert_allclose(P, C, rtol=1e-13, atol=1e-13 * np.abs(want).max())
    # singular (a direction nothing constrains), indefinite, too few points, not finite
    S = H.copy(); S[:, 5] = 0.0; S[5, :] = 0.0
    N = H.copy(); N[2, 2] = -N[2, 2]
    F = H.copy(); F[0, 0] = np.inf
    for bad, m in ((S, n), (N, n), (H, 6), (H, 0), (F, n), (np.zeros((6, 6)), n)):
        ok, C = call(bad, e2, m)
        assert not ok and np.all(C == -7.0)
        assert capi.pose_covariance(bad, e2, m) is None
    ok, _ = call(H, e2, 7)
    assert ok and capi.pose_covariance(H, e2, 7) is not None
