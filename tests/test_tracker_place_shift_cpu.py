"""Shift search on place descriptors and the pose guess (include/dvo_amd.h: dvo_tracker_place_shifts, dvo_tracker_place_guess): what
can be checked without a GPU -- the symbols, the record's layout against the C compiler's, the guess's double arithmetic, and the
INPUTS of tests/test_gpu_tracker_place_shift.py, asserted on the numpy reference alone (tests/place_shift_reference.py on descriptors
from tests/frame_reference.py's restatement of the frame stage), so that a change of the frame generator that spoils them fails where
it can be seen.

The guess: dvo_tracker_place_guess needs a tracker, and a tracker needs a device.  Its arithmetic is the host function
dvo_host::place_guess (rgbd_odometry_amd/csrc/dvo_place_guess.h) that the library compiles; the stand-alone program
tests/host/place_guess_main.cpp runs that function here, under the address and undefined-behaviour sanitizers, and the GPU file repeats
the comparison through the C ABI."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import frame_gen
import place_shift_reference as ps
import places_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvo_amd.h")
NEW = ["dvo_tracker_place_shifts", "dvo_tracker_place_guess"]
ROWS, COLS, LEVEL, SHIFT = 240, 320, 2, 0                 # the geometry of the places tests: level 2 = 60 x 80, D = 4800
LR, LC = 60, 80
K = (262.5, 262.5, 159.75, 119.75)
RADIUS = 6
# frames shifted by this many camera pixels register at this shift of the level (the frame generator moves the scene by -shift)
REVISITS = {(8, -12): (-2, 3), (-16, 4): (4, -1), (-16, 16): (4, -4)}
SEEDS = (900, 901, 70)                                    # the scene of each is compared with that of seed + 1


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/dvo_amd.h" % name
        assert name in capi.C_ABI_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
    assert callable(capi.DvoTracker.place_shifts) and callable(capi.DvoTracker.place_shifts_raw) and callable(capi.DvoTracker.place_guess)
    assert re.search(r"#define DVO_TRACKER_PLACE_SHIFT_LAUNCHES 1\b", text) and capi.DVO_TRACKER_PLACE_SHIFT_LAUNCHES == 1
    assert re.search(r"#define DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS 8\b", text) and capi.DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS == 8 == ps.MAX_RADIUS
    # without a handle both refuse
    assert lib.dvo_tracker_place_shifts(None, 0, None, None, 0, None) != 0 and lib.dvo_tracker_place_guess(None, 0, 0, 0, None, None) != 0


def test_struct_layout_matches_header():
    """size and offsets of the ctypes mirror against what the C compiler gives the header's struct"""
    from rgbd_odometry_amd import capi
    cname, mirror = "dvo_tracker_place_shift", capi.DvoTrackerPlaceShift
    items = ["sizeof(%s)" % cname] + ["offsetof(%s, %s)" % (cname, f[0]) for f in mirror._fields_]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%s", %s);return 0;}'
                             % (" ".join(["%zu"] * len(items)), ", ".join("(size_t)" + i for i in items)))
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert got == want, (items, got, want)
    assert tuple(f[0] for f in mirror._fields_) == ps.FIELDS == capi.DvoTracker.PLACE_SHIFT_FIELDS
    assert C.sizeof(mirror) == 24 and np.dtype(mirror).itemsize == 24


@pytest.fixture(scope="module")
def host_guesses(tmp_path_factory):
    """{(dy, dx): (R0 as a matrix, t0)} of dvo_host::place_guess for K, level 2, first_shift 0 over [-8, 8]^2"""
    d = tmp_path_factory.mktemp("place_guess")
    exe = str(d / "place_guess_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "place_guess_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/place_guess_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    run = subprocess.run([exe, repr(K[0]), repr(K[1]), str(SHIFT + LEVEL), str(ps.MAX_RADIUS)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for ln in run.stdout.splitlines():
        w = ln.split()
        v = [float.fromhex(x) for x in w[2:]]
        out[(int(w[0]), int(w[1]))] = (np.array(v[:9]).reshape(3, 3).T, np.array(v[9:]))      # column-major -> the matrix
    assert len(out) == 17 * 17
    return out


def test_guess_against_the_reference(host_guesses):
    """a few dozen double operations on values <= 1 (divisions, one square root, sums of at most three products): each entry is within
    a few units of 2^-53 of the exact value in either implementation, far below 1e-14"""
    worst = 0.0
    for (dy, dx), (R0, t0) in host_guesses.items():
        Rw, tw = ps.guess(K, LEVEL, SHIFT, dy, dx)
        worst = max(worst, float(np.abs(R0 - Rw).max()))
        assert np.abs(R0 - Rw).max() <= 1e-14 and np.array_equal(t0, tw), (dy, dx, R0, Rw)
    print("largest difference of an entry: %.3g" % worst)


def test_guess_properties(host_guesses):
    sc = 2.0 ** -(SHIFT + LEVEL)
    fx, fy = K[0] * sc, K[1] * sc
    for (dy, dx), (R0, t0) in host_guesses.items():
        assert np.abs(R0.T @ R0 - np.eye(3)).max() <= 1e-14, (dy, dx)
        assert np.linalg.det(R0) > 0
        d = R0.T @ np.array([0.0, 0.0, 1.0])                                # the key frame's optical axis in the current camera
        assert d[2] > 0 and abs(fx * d[0] / d[2] - dx) <= 1e-9 and abs(fy * d[1] / d[2] - dy) <= 1e-9, (dy, dx, d)
        assert not t0.any()
    R0, t0 = host_guesses[(0, 0)]
    assert np.array_equal(R0, np.eye(3)) and np.array_equal(t0, np.zeros(3))
    for f in (ps.guess,):                                                    # ... and so does the reference
        assert np.array_equal(f(K, LEVEL, SHIFT, 0, 0)[0], np.eye(3))


def descriptor(seed, shift):
    return ps.level_descriptor(frame_gen.camera_frame(seed, ROWS, COLS, shift=shift, holes=True)[0], SHIFT + LEVEL)


def test_input_conditions():
    """what makes the feature's point, on the reference alone: shifted revisits register exactly where they were moved to, by a
    unique and deep minimum, while the whole-descriptor distance cannot tell the revisit from a different scene"""
    for seed in SEEDS:
        key, other = descriptor(seed, (0, 0)), descriptor(seed + 1, (0, 0))
        for moved, want in REVISITS.items():
            q = descriptor(seed, moved)
            rec, ties = ps.record_of_table(ps.sad_table(key, q, LR, LC, RADIUS), LR, LC)
            print(seed, moved, rec, "ties", ties, "distance", pr.distance(key, q))
            assert (rec["dy"], rec["dx"]) == want and ties == 1, (seed, moved, rec, ties)
            assert rec["area"] == (LR - 2 * RADIUS) * (LC - 2 * RADIUS) == 3264
            assert rec["sad"] <= rec["area"] and rec["sad_second"] >= 20000 and rec["sad_zero"] > rec["sad_second"], (seed, moved, rec)
        far = descriptor(seed, (-16, 16))
        revisit, stranger = ps.record(key, far, LR, LC, RADIUS), ps.record(key, other, LR, LC, RADIUS)
        print(seed, "revisit", pr.distance(key, far), revisit, "different scene", pr.distance(key, other), stranger)
        assert pr.distance(key, far) >= 0.9 * pr.distance(key, other), seed
        assert stranger["sad"] >= 5 * revisit["sad"] and stranger["sad"] >= 20000, (seed, stranger, revisit)
    # the figures of the issue for seed 900
    key = descriptor(900, (0, 0))
    assert pr.distance(key, descriptor(900, (-16, 16))) == 86147 and pr.distance(key, descriptor(901, (0, 0))) == 88060
    assert ps.record(key, descriptor(900, (-16, 16)), LR, LC, RADIUS) == dict(dy=4, dx=-4, sad=0, sad_zero=64837, sad_second=28168, area=3264)
    assert ps.record(key, descriptor(901, (0, 0)), LR, LC, RADIUS)["sad"] == 60349


def test_radius_zero_is_the_distance():
    key, q = descriptor(900, (0, 0)), descriptor(901, (0, 0))
    assert ps.record(key, q, LR, LC, 0) == dict(dy=0, dx=0, sad=pr.distance(key, q), sad_zero=pr.distance(key, q), sad_second=ps.NONE, area=LR * LC)
    # radius 1: no shift is two away from the centre, every shift is two away from a corner
    t = np.full((3, 3), 9, np.int64)
    t[1, 1] = 1
    assert ps.record_of_table(t, LR, LC)[0]["sad_second"] == ps.NONE
    t[0, 0] = 0
    assert ps.record_of_table(t, LR, LC)[0] == dict(dy=-1, dx=-1, sad=0, sad_zero=1, sad_second=9, area=58 * 78)


def test_tie_inputs():
    """the constructed frames have more than one minimum in the reference, and each tier of the order decides at least once"""
    frames = ps.tie_frames(ROWS, COLS, SHIFT + LEVEL)
    assert sorted(frames) == ["cols_tie", "flat", "rows_tie", "stripes"]
    minima = {}
    for name, (key, query, radius, want) in frames.items():
        t = ps.sad_table(ps.level_descriptor(key, SHIFT + LEVEL), ps.level_descriptor(query, SHIFT + LEVEL), LR, LC, radius)
        rec, ties = ps.record_of_table(t, LR, LC)
        minima[name] = sorted((dy - radius, dx - radius) for dy, dx in zip(*np.nonzero(t == rec["sad"])))
        print(name, rec, "ties", ties, minima[name])
        assert ties > 1 and (rec["dy"], rec["dx"]) == want, (name, rec, ties)
    assert len(minima["flat"]) == 49                                                     # every SAD equal: |dy| + |dx| decides
    assert minima["stripes"] == [(0, -2), (0, 0), (0, 2)]                                # |dy| + |dx| decides
    assert minima["rows_tie"] == [(-1, 0), (1, 0)]                                       # equal SAD and |dy| + |dx|: dy decides
    assert minima["cols_tie"] == [(0, -1), (0, 1)]                                       # ... and equal dy: dx decides
