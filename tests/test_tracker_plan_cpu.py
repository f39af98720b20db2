"""The two pure host headers of the multi-stream tracker (rgbd_odometry_amd/csrc): dvo_tracker_plan.h -- banks, first / align split,
upload runs, key-frame flags and the per-stream counters of a tick -- and dvo_key_ring.h -- ids, slots, refusals, evictions and
counters of the key-frame ring, for the step's store and the import alike.

tests/host/tracker_plan_main.cpp walks both against naive restatements of its own: every subset and order of 4 streams in every
started / bank state, the flags over n_frame - last_ref, the clock's transitions; rings of capacity 1, 2 and 3 through sequences of
three calls of 0 .. 2 * capacity + 1 candidates with every pattern of refusals (capacity 3: the first call stops at 3 candidates).  It is built once plainly and once under the address
and undefined-behaviour sanitizers, a stand-alone program both times.  CPU test; the device twins are test_ring_evicts_the_oldest of
tests/test_gpu_tracker_archive.py and tests/test_gpu_archive_blob.py.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd_odometry_amd", "csrc")
# 64 lists x 256 states, 4 named cases, the flags (every + 2 distances x 3 bases for every in 1, 2, 5), 8 clock cases
PLAN_CASES = 64 * 256 + 4 + 3 * sum(every + 2 for every in (1, 2, 5)) + 8


def _calls(capacity):
    kinds = sum(2 ** n for n in range(2 * capacity + 2))
    first = kinds if capacity < 3 else sum(2 ** n for n in range(capacity + 1))     # capacity 3: the first call stops at capacity candidates
    return first * (1 + kinds + kinds * kinds)


RING_CALLS = sum(_calls(c) for c in (1, 2, 3))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("tracker_plan_" + request.param)
    exe = str(d / "tracker_plan_main")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tracker_plan_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/tracker_plan_main.cpp did not build (the sanitized build needs g++ with libasan and libubsan):\n" + build.stderr
    return exe


def test_plan_and_ring_agree_with_their_naive_restatements(host_program):
    run = subprocess.run([host_program], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    m = re.fullmatch(r"ok (\d+) (\d+)\n", run.stdout)
    assert m, run.stdout
    assert (int(m.group(1)), int(m.group(2))) == (PLAN_CASES, RING_CALLS)       # every case really was walked


def test_the_ring_arithmetic_lives_in_one_header():
    """id -> slot is decided in dvo_key_ring.h and nowhere else in csrc/; both headers stay free of HIP and of the context"""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".cpp", ".hip")) and name != "dvo_key_ring.h":
            text = open(os.path.join(CSRC, name)).read()
            assert not re.search(r"%\s*(A\.|ring\.|tr->ar\.)?(ring\.)?capacity", text), name
    for name in ("dvo_key_ring.h", "dvo_tracker_plan.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert re.findall(r'#include\s+"([^"]+)"', text) == ["../../include/dvo_amd.h"] and "<hip" not in text and "getenv" not in text, name
