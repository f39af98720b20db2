"""The upload planner of the frame store (rgbd_odometry_amd/csrc/dvo_upload_plan.h): level sizes, strides, the route of the sources,
the chunk size, the gather's workgroups, the submission order and the argument refusals of both upload entry points are pure
functions of a few integers, walked by the stand-alone program tests/host/upload_plan_main.cpp (a table of named rows, then a sweep of
the arithmetic invariants) under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_upload_plan_table(tmp_path):
    exe = str(tmp_path / "upload_plan_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "upload_plan_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: 86400 sweep cases"), run.stdout
