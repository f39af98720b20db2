"""The landing pipeline of the frame uploads (rgbd_odometry_amd/csrc/dvo_upload_ring.h): two landing buffers, their pinned mirrors,
two copy streams and the events between them and the consumer stream as one owning type with named transitions, and the address table
of the sources that are read in place, walked by the stand-alone program tests/host/upload_ring_main.cpp over fakes of the HIP calls
that record a call log, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_upload_ring_protocol(tmp_path):
    exe = str(tmp_path / "upload_ring_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"),
                            "-o", exe, os.path.join(ROOT, "tests", "host", "upload_ring_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
