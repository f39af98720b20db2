"""CPU checks of the camera sensor formats (mono8 / RGB8 images, 16-bit depth): the binding exposes the new entry points, its format
enums are the header's, the C++ mirror and its demo compile against them, and the mirror no longer widens depth frames on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NEW_SYMBOLS = ("dvo_frames_upload_cameras_fmt", "dvo_tracker_step_fmt", "dvo_photo_streams_step_fmt")


def _header(name):
    return open(os.path.join(INCLUDE, name)).read()


def test_binding_exposes_the_new_symbols():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in capi.C_ABI_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    # same arguments as the entry point each generalises, plus the two formats
    assert len(lib.dvo_frames_upload_cameras_fmt.argtypes) == len(lib.dvo_frames_upload_cameras.argtypes) + 2
    assert len(lib.dvo_tracker_step_fmt.argtypes) == len(lib.dvo_tracker_step.argtypes) + 2
    assert len(lib.dvo_photo_streams_step_fmt.argtypes) == len(lib.dvo_photo_streams_step.argtypes) + 2


def test_format_enums_equal_the_header():
    from rgbd_odometry_amd import capi
    src = re.sub(r"/\*.*?\*/", "", _header("dvo_amd.h"), flags=re.S)
    found = dict((k, int(v)) for k, v in re.findall(r"\b(DVO_(?:CAM|DEPTH)_[A-Z0-9]+)\s*=\s*(\d+)", src))
    assert sorted(found) == ["DVO_CAM_BGR8", "DVO_CAM_MONO8", "DVO_CAM_RGB8", "DVO_DEPTH_F32", "DVO_DEPTH_U16"]
    for name, value in found.items():
        assert getattr(capi, name) == value, name
    assert found["DVO_CAM_BGR8"] == 0 and found["DVO_DEPTH_F32"] == 0          # the existing entry points' formats


def test_arrays_name_their_format():
    """what the Python methods pass on: uint16 depth stays 16-bit, a 2-D image is mono8, rgb=True marks RGB8, defaults as before"""
    from rgbd_odometry_amd import capi
    bgr, grey = np.zeros((4, 8, 3), np.uint8), np.zeros((4, 8), np.uint8)
    d16, df = np.zeros((4, 8), np.uint16), np.zeros((4, 8), np.float64)
    ifmt, il, dfmt, dl = capi._camera_arrays([bgr], [df], False, 0)
    assert (ifmt, dfmt) == (capi.DVO_CAM_BGR8, capi.DVO_DEPTH_F32) and dl[0].dtype == np.float32
    ifmt, il, dfmt, dl = capi._camera_arrays([bgr], [d16], True, 0)
    assert (ifmt, dfmt) == (capi.DVO_CAM_RGB8, capi.DVO_DEPTH_U16) and dl[0].dtype == np.uint16 and np.shares_memory(dl[0], d16)
    ifmt, il, dfmt, dl = capi._camera_arrays([grey], None, False, 0)
    assert (ifmt, dfmt, dl) == (capi.DVO_CAM_MONO8, capi.DVO_DEPTH_F32, None) and np.shares_memory(il[0], grey)
    assert capi._camera_arrays([bgr], [d16, df], False, 0)[2] == capi.DVO_DEPTH_F32        # mixed dtypes: all taken as float
    for bad in (([grey, bgr], None, False), ([grey], None, True), ([np.zeros((4, 8, 4), np.uint8)], None, False)):
        with pytest.raises(ValueError):
            capi._camera_arrays(bad[0], bad[1], bad[2], 0)


def _syntax_check(tmp_path, name, source):
    src = tmp_path / name
    src.write_text(source)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_cpp_mirror_and_demo_compile(tmp_path):
    """the mirror's 16-bit paths are templates of nothing: a translation unit that calls them must compile, and so must the demo"""
    _syntax_check(tmp_path, "mirror.cpp", """
#include "dvo_amd.hpp"
std::vector<dvo_amd::Pose> tracker(dvo_amd::SolveDVOStreams &t, const std::vector<int> &s, const std::vector<const unsigned char *> &b,
                                   const std::vector<const unsigned short *> &d16, const std::vector<const float *> &dm) {
    t.processCameraFrames(s, b, dm);
    return t.processCameraFrames(s, b, d16, DVO_UPLOAD_DEPTH_RAW);
}
std::vector<dvo_amd::Pose> photo(dvo_amd::RGBDOdometryStreams &p, const std::vector<int> &s, const std::vector<const unsigned char *> &b,
                                 const std::vector<const unsigned short *> &d16) { return p.processFrames(s, b, d16); }
dvo_amd::Pose one(dvo_amd::RGBDOdometry &o, const unsigned char *b, const unsigned short *d) { o.setRcvdFrame(b, d, 480, 640); return o.processFrame(); }
int formats() { return DVO_CAM_BGR8 + DVO_CAM_RGB8 + DVO_CAM_MONO8 + DVO_DEPTH_F32 + DVO_DEPTH_U16; }
""")
    _syntax_check(tmp_path, "demo.cpp", '#include "%s"\n' % os.path.join(ROOT, "examples", "rgbd_odometry_demo.cpp"))


def test_mirror_no_longer_widens_depth_on_the_host():
    hpp = re.sub(r"/\*.*?\*/", "", _header("dvo_amd.hpp"), flags=re.S)
    assert "depthF_" not in hpp
    assert not re.search(r"std::vector<float>\s+\w+\(rcvd_depth_", hpp)                       # RGBDOdometry::upload's float copy
    for cls, call in (("class RGBDOdometry ", "dvo_frames_upload_cameras_fmt("), ("class RGBDOdometryStreams ", "dvo_photo_streams_step_fmt(")):
        body = hpp[hpp.index(cls):]
        body = body[:body.index("\n};")]
        assert call in body and "DVO_DEPTH_U16" in body, cls
        assert not re.search(r"std::copy\(\s*depth", body), cls
