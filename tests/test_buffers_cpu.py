"""The owning device and pinned buffers of the host layer (rgbd_odometry_amd/csrc/dvo_buffers.h): ownership, moves and the failure
paths of the grow sites, walked by the stand-alone program tests/host/buffers_main.cpp over counting fakes of the HIP allocation calls,
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffers_own_and_fail_empty(tmp_path):
    exe = str(tmp_path / "buffers_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"),
                            "-o", exe, os.path.join(ROOT, "tests", "host", "buffers_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
