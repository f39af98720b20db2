"""p4_line_offset (rgbd_odometry_amd/csrc/dvo_palette.h): the byte offset at which the fused kernel gathers the rank words of a pixel.

The kernel's form of the offset -- xx * 32 + (xx >> 2) * (column bytes - 128) + yy * 4 + (yy / 6) * 104, counted from the first real line
-- must name the very dword the layout's definition p4_slot names.  tests/host/line_offset_main.cpp walks every pixel of every level
size with rows in 1..64 and {120, 240, 480, 1080, 3072} and cols in 1..40 and {160, 320, 640, 1920, 4096}; it is built once plainly and
once under the address and undefined-behaviour sanitizers, a stand-alone program both times.  CPU test; what the kernel does with the
offset is tests/test_gpu_line_offset.py.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd_odometry_amd", "csrc")
PIXELS = (sum(range(1, 65)) + 120 + 240 + 480 + 1080 + 3072) * (sum(range(1, 41)) + 160 + 320 + 640 + 1920 + 4096)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("line_offset_" + request.param)
    exe = str(d / "line_offset_main")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                           ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", CSRC,
                            "-o", exe, os.path.join(ROOT, "tests", "host", "line_offset_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/line_offset_main.cpp did not build (the sanitized build needs g++ with libasan and libubsan):\n" + build.stderr
    return exe


def test_every_pixel_of_every_size_names_the_slot_of_the_layout(host_program):
    run = subprocess.run([host_program], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    m = re.fullmatch(r"ok (\d+)\n", run.stdout)
    assert m, run.stdout
    assert int(m.group(1)) == PIXELS            # every pixel of every size really was walked


def test_the_fused_kernel_addresses_the_compact_form_through_it_alone():
    """every look-up of dvo_fused.hip goes through p4_line_offset; the helper it replaced is gone"""
    text = open(os.path.join(CSRC, "dvo_fused.hip")).read()
    assert "p4_byte_offset" not in text and "p4_line_offset<" in text
    header = open(os.path.join(CSRC, "dvo_palette.h")).read()
    assert header.count("v_mad_u32_u24") >= 2 and "__umul24" in header       # the multiplies stay 24-bit ones
