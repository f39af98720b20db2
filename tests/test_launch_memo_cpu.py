"""The key of enqueue()'s memo (rgbd_odometry_amd/csrc/dvo_launch_memo.h): which request and which host state a remembered
launch stands for, and which passes are never remembered, are pure host code, walked by the stand-alone program
tests/host/launch_memo_main.cpp -- built plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_launch_memo_key(tmp_path, flags):
    exe = str(tmp_path / "launch_memo_main")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                           ["-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "launch_memo_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
