"""The launch planner of the fused alignment (rgbd_odometry_amd/csrc/dvo_launch_plan.h): kernel, block size, LDS budget, team size,
the tiers of the wide / tiled schedule, the epoch of the team exchange records and the launch order are pure functions of a few
integers, walked by the stand-alone program tests/host/launch_plan_main.cpp under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_table(tmp_path):
    exe = str(tmp_path / "launch_plan_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "launch_plan_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
