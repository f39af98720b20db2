"""The scaffold of the stand-alone handles (rgbd_odometry_amd/csrc/dvo_handle.h): the staging pair, the device guard, the mapping of
HIP errors to status codes with its check macro, the creation-time device check and the bracket of a call's stats, walked by the
stand-alone program tests/host/handle_main.cpp over counting fakes of the HIP calls, under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_scaffold(tmp_path):
    exe = str(tmp_path / "handle_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"),
                            "-o", exe, os.path.join(ROOT, "tests", "host", "handle_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
