"""CPU checks of per-stream camera calibration (include/dvo_amd.h: dvo_tracker_set_stream_intrinsics / _undistort / clear_stream_camera,
dvo_photo_streams_set_stream_intrinsics): the header declares the functions, the library exports them, the binding lists them, the C++
mirror builds with its new methods, and without a HIP device the handles still fail loudly at creation."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["dvo_tracker_set_stream_intrinsics", "dvo_tracker_set_stream_undistort", "dvo_tracker_clear_stream_camera",
           "dvo_photo_streams_set_stream_intrinsics"]


def _declared():
    src = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    return set(re.findall(r"\b(dvo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


def test_header_declares_and_library_exports():
    from rgbd_odometry_amd import capi
    declared = _declared()
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_binding_lists_the_symbols():
    from rgbd_odometry_amd import DvoPhotoStreams, DvoTracker, capi
    for name in SYMBOLS:
        assert name in capi.C_ABI_SYMBOLS, name
    for m in ("set_stream_intrinsics", "set_stream_undistort", "clear_stream_camera"):
        assert callable(getattr(DvoTracker, m))
    assert callable(DvoPhotoStreams.set_stream_intrinsics)


def test_null_handles_are_refused():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    assert lib.dvo_tracker_set_stream_intrinsics(None, 0, 1.0, 1.0, 0.0, 0.0) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_set_stream_undistort(None, 0, None, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_clear_stream_camera(None, 0) == capi.DVO_ERR_INVALID
    assert lib.dvo_photo_streams_set_stream_intrinsics(None, 0, 1.0, 1.0, 0.0, 0.0) == capi.DVO_ERR_INVALID


def test_calibration_argument_checks_without_a_device():
    """what dvo_frames_set_undistort / dvo_tracker_set_stream_undistort refuse is decided before any device work, by the host map
    builder they share (dvo_undistort_map_host): NaN or infinity anywhere in K4 / D5, fx or fy zero, an empty image, a missing array
    -> DVO_ERR_INVALID and nothing written.  A finite calibration that leaves the int range is accepted (cvRound saturates)"""
    import numpy as np
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    assert "dvo_undistort_map_host" in _declared() and "dvo_undistort_map_host" in capi.C_ABI_SYMBOLS
    rows, cols = 6, 8
    xy, frac = np.full(2 * rows * cols, -5, np.int16), np.full(rows * cols, 9, np.uint16)
    good = np.array([10.0, 11.0, 3.5, 2.5, 0.1, -0.02, 0.001, 0.001, 0.0])

    def call(v, r=rows, c=cols, k_null=False, d_null=False):
        K, D = v[:4].copy(), v[4:].copy()
        return lib.dvo_undistort_map_host(r, c, None if k_null else capi._ptr(K), None if d_null else capi._ptr(D), capi._ptr(xy), capi._ptr(frac))
    for k in range(9):
        for bad in (float("nan"), float("inf"), float("-inf")):
            v = good.copy(); v[k] = bad
            assert call(v) == capi.DVO_ERR_INVALID, (k, bad)
    for v, kw in ((good * [0, 1, 1, 1, 1, 1, 1, 1, 1], {}), (good * [1, 0, 1, 1, 1, 1, 1, 1, 1], {}), (good, dict(r=0)), (good, dict(c=0)),
                  (good, dict(k_null=True)), (good, dict(d_null=True))):
        assert call(np.asarray(v, np.float64), **kw) == capi.DVO_ERR_INVALID
    assert lib.dvo_undistort_map_host(rows, cols, capi._ptr(good[:4].copy()), capi._ptr(good[4:].copy()), None, capi._ptr(frac)) == capi.DVO_ERR_INVALID
    assert (xy == -5).all() and (frac == 9).all()
    assert call(good) == capi.DVO_OK and not (xy == -5).any()
    huge = good.copy(); huge[4] = 1e12
    assert call(huge) == capi.DVO_OK
    far = np.hypot((np.arange(cols) - 3.5) / 10.0, 0.25)[None, :] > 0.3           # r2 > 0.09: u*32 beyond int -> INT_MIN -> (0, 0), fraction 0
    m = xy.reshape(rows, cols, 2)
    assert (m[0][far[0]] == 0).all() and (frac.reshape(rows, cols)[0][far[0]] == 0).all()
    # NULL handles are refused before the calibration is looked at
    K, D = good[:4].copy(), good[4:].copy()
    assert lib.dvo_tracker_set_stream_undistort(None, 0, capi._ptr(K), capi._ptr(D)) == capi.DVO_ERR_INVALID


def test_mirror_header_compiles(tmp_path):
    """dvo_amd::SolveDVOStreams / RGBDOdometryStreams with their per-stream calibration methods build into a program that links the
    library; the calibration XML is read like SolveDVO::setCameraMatrix(const char *)"""
    xml = tmp_path / "cam1.xml"
    xml.write_text('<?xml version="1.0"?>\n<opencv_storage>\n<cameraMatrix type_id="opencv-matrix"><rows>3</rows><cols>3</cols>'
                   '<dt>d</dt>\n<data>\n 5.2e+02 0. 3.2e+02 0. 5.3e+02 2.4e+02 0. 0. 1.</data></cameraMatrix>\n</opencv_storage>\n')
    src = tmp_path / "m.cpp"
    src.write_text('#include "dvo_amd.hpp"\n#include <cstdio>\nint main(int argc, char **argv) {\n'
                   '  double k[9]; dvo_amd::readCameraMatrix(argv[1], k);\n'
                   '  std::printf("%g %g %g %g\\n", k[0], k[4], k[2], k[5]);\n'
                   '  if (argc > 2) {\n'
                   '    dvo_amd::SolveDVOStreams s(4); s.setCameraMatrix(525, 525, 319.5, 239.5);\n'
                   '    s.setStreamCameraMatrix(1, argv[1]); s.setStreamCameraMatrix(2, 530.f, 531.f, 320.f, 240.f);\n'
                   '    const double K4[4] = {530, 531, 320, 240}, D5[5] = {-0.1, 0.01, 0, 0, 0};\n'
                   '    s.setStreamUndistort(2, 480, 640, K4, D5); s.clearStreamCamera(3);\n'
                   '    dvo_amd::RGBDOdometryStreams r(2); r.setCameraMatrix(525, 525, 319.5, 239.5); r.setStreamCameraMatrix(1, 530, 531, 320, 240);\n'
                   '  }\n'
                   '  std::puts("ok"); return 0; }\n')
    exe = tmp_path / "m"
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", lib, "-ldvo_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe), str(xml)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.split() == ["520", "530", "320", "240", "ok"], (run.stdout, run.stderr)


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    from rgbd_odometry_amd import DvoError, DvoPhotoStreams, DvoTracker
    from rgbd_odometry_amd.capi import DVO_ERR_NO_DEVICE
    for make in (lambda: DvoTracker(4), lambda: DvoPhotoStreams(4, (525.0, 525.0, 319.5, 239.5))):
        with pytest.raises(DvoError) as ei:
            make()
        assert ei.value.code == DVO_ERR_NO_DEVICE
