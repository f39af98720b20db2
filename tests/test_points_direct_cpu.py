"""The direct 4-byte form of a reference point (rgbd_odometry_amd/csrc/dvo_points_direct.h): column | row << 10 | millimetres << 19.

The fused kernel re-encodes the block-relative 4-byte points of a level into this form while it stages them into LDS, and falls back to
the block-relative words when a point does not fit.  The pack / fits / unpack helpers are host-compilable: the stand-alone program
tests/host/points_direct_main.cpp runs them over every depth below 8192 mm at a grid of pixels with the corners, and over the refusal
boundaries, under the address and undefined-behaviour sanitizers.  CPU test; what the kernel does with the form is
tests/test_gpu_points_direct.py.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd_odometry_amd", "csrc")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_direct")
    exe = str(d / "points_direct_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "points_direct_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/points_direct_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return exe


def test_pack_unpack_and_refusals_under_sanitizers(host_program):
    run = subprocess.run([host_program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    m = re.fullmatch(r"ok (\d+)\n", run.stdout)
    assert m, run.stdout
    assert int(m.group(1)) >= 30 * 20 * 8192            # the grid really was walked


def test_field_constants_are_the_documented_ones():
    """10 + 9 + 13 bits, compile-time constants; the header and the C API's description agree"""
    text = open(os.path.join(CSRC, "dvo_points_direct.h")).read()
    for name, value in (("PT4D_X_BITS", 10), ("PT4D_Y_BITS", 9), ("PT4D_D_BITS", 13)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    api = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    assert "dvo_get_level_points4_direct" in api and "8192 mm" in api and "1024 columns and 512 rows" in api


def test_only_the_integer_helpers_live_in_the_header():
    """the header is not among the kernel sources bench.py hashes: nothing hot belongs in it (no float code, no device-only code)"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(CSRC, "dvo_points_direct.h")).read(), flags=re.S)
    assert "float" not in text and "__device__ __forceinline__" not in text and "DVO_DEV" not in text
