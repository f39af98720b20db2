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
