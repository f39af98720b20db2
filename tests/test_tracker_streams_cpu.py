"""CPU checks of the multi-stream tracker (include/dvo_amd.h, "many camera streams"): the header declares it, the library
exports it, the Python binding and the C++ mirror exist and build, and without a HIP device it fails loudly."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACKER_SYMBOLS = ["dvo_tracker_params_default", "dvo_tracker_create", "dvo_tracker_destroy", "dvo_tracker_last_error",
                   "dvo_tracker_set_intrinsics", "dvo_tracker_reset_stream", "dvo_tracker_step", "dvo_tracker_step_pyramids",
                   "dvo_tracker_get_signals", "dvo_tracker_get_stats", "dvo_tracker_context"]


def _declared():
    src = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    return set(re.findall(r"\b(dvo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


def test_header_library_and_binding_have_the_tracker():
    from rgbd_odometry_amd import capi
    declared = _declared()
    lib = capi.load_library()
    for name in TRACKER_SYMBOLS:
        assert name in declared, name
        assert name in capi.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    assert hasattr(capi, "DvoTracker")
    from rgbd_odometry_amd import DvoTracker  # noqa: F401


def test_tracker_param_defaults_and_layout(tmp_path):
    """defaults are the reference's literals; the ctypes mirror has the C layout"""
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    tp = capi.DvoTrackerParams()
    assert lib.dvo_tracker_params_default(ctypes.byref(tp)) == 0
    assert list(tp.iters) == [50] * capi.DVO_MAX_LEVELS and tp.key_frame_every == 5 and tp.adaptive == 0
    assert tp.laplacian_b_thresh == 3.0 and abs(tp.visible_ratio_thresh - 0.8) < 1e-7 and tp.min_points == 50
    assert (tp.rows, tp.cols, tp.n_levels, tp.first_shift) == (480, 640, 4, 1)
    assert list(tp.points_capacity) == [0] * capi.DVO_MAX_LEVELS
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu", sizeof(dvo_tracker_params), '
                   'offsetof(dvo_tracker_params, rows), offsetof(dvo_tracker_params, points_capacity));return 0;}')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, rows_off, cap_off = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert ctypes.sizeof(capi.DvoTrackerParams) == size
    assert capi.DvoTrackerParams.rows.offset == rows_off and capi.DvoTrackerParams.points_capacity.offset == cap_off


def test_multi_track_demo_compiles(tmp_path):
    """examples/multi_track_demo.cpp builds against the C++ mirror (dvo_amd::SolveDVOStreams) and links the library"""
    exe = tmp_path / "multi_track_demo"
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "multi_track_demo.cpp"), "-o", str(exe), "-L", lib, "-ldvo_amd",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    usage = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert usage.returncode == 2 and "usage" in usage.stderr
    # a complete argument list is accepted (it then fails on the missing frame file, before any device work)
    full = subprocess.run([str(exe), "2", str(tmp_path / "a"), str(tmp_path / "b"), "0", "9", "1", "3", "262.5", "262.5", "159.75",
                           "119.75", "8", str(tmp_path / "out_")], capture_output=True, text=True, timeout=60)
    assert full.returncode == 1 and "cannot read" in full.stderr, full.stderr


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    from rgbd_odometry_amd import DvoError, DvoTracker
    from rgbd_odometry_amd.capi import DVO_ERR_NO_DEVICE
    with pytest.raises(DvoError) as ei:
        DvoTracker(4)
    assert ei.value.code == DVO_ERR_NO_DEVICE
    assert "no CPU fallback" in str(ei.value)


def test_refusals_before_any_device_work():
    """bad creation arguments are refused with DVO_ERR_INVALID (checked before the device is touched)"""
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    h = ctypes.c_void_p()
    tp = capi.DvoTrackerParams()
    lib.dvo_tracker_params_default(ctypes.byref(tp))
    assert lib.dvo_tracker_create(None, 0, ctypes.byref(tp), ctypes.byref(h)) == capi.DVO_ERR_INVALID
    for l in range(capi.DVO_MAX_LEVELS):
        tp.iters[l] = 0
    assert lib.dvo_tracker_create(None, 4, ctypes.byref(tp), ctypes.byref(h)) == capi.DVO_ERR_INVALID
    assert b"no iterations" in lib.dvo_tracker_last_error(None)
    assert lib.dvo_tracker_step(None, 1, None, None, None, 0, 0, 0, None, None, None) == capi.DVO_ERR_INVALID
