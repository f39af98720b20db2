"""Ignore masks on the CPU (include/dvo_amd.h, "ignore masks"): dvo_mask_levels_host against the numpy restatement of the definition
(tests/mask_reference.py), the footprint against the INTER_NEAREST pyramid's sampling (tests/frame_reference.py), every refusal, and
the builder's own code (rgbd_odometry_amd/csrc/dvo_mask_levels.h) as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/host/mask_levels_main.cpp).  No GPU: the builder needs neither a device nor a context."""
import os
import re
import subprocess

import numpy as np
import pytest

import frame_reference as fr
import mask_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (rows, cols, first_shift, n_levels)
GEOMETRIES = [
    (96, 128, 1, 3),
    (75, 101, 1, 3),          # 38x50, 19x25, 9x13: a size rounded up (37.5 -> 38, 18.75 -> 19), one rounded down (9.375 -> 9, 12.625 -> 13)
    (100, 100, 3, 1),         # 12x12: the last four camera rows and columns belong to no level pixel
    (37, 53, 0, 2),           # first_shift 0: the footprint of level 0 is one pixel
]
MARGINS = [0, 1, 2, 8]


def masks_of(rows, cols):
    out = {"zero": np.zeros((rows, cols), np.uint8), "set": np.full((rows, cols), 255, np.uint8), "scene": mr.scene_mask(rows, cols, 3)}
    for name, (y, x) in {"tl": (0, 0), "tr": (0, cols - 1), "bl": (rows - 1, 0), "br": (rows - 1, cols - 1)}.items():
        m = np.zeros((rows, cols), np.uint8)
        m[y, x] = 1                                          # any non-zero byte counts
        out["corner_" + name] = m
    rng = np.random.default_rng(rows * 1000 + cols)
    out["sparse"] = (rng.random((rows, cols)) < 0.002).astype(np.uint8) * 7
    return out


def test_level_sizes_are_the_engines():
    assert [(mr.level_size(75, s), mr.level_size(101, s)) for s in (1, 2, 3)] == [(38, 50), (19, 25), (9, 13)]
    assert mr.level_size(100, 3) == 12
    for n in list(range(1, 300)) + [479, 480, 481, 640, 1080, 1920]:
        for s in range(0, 7):
            assert mr.level_size(n, s) == fr.level_size(n, s) == int(np.rint(n * 2.0 ** -s))


@pytest.mark.parametrize("rows,cols,first_shift,n_levels", GEOMETRIES)
def test_footprint_starts_at_the_pixel_the_pyramid_samples(rows, cols, first_shift, n_levels):
    """resize_nn of an image that holds its own pixel index gives, per level pixel, the camera pixel the pyramid samples: it must be
    the first pixel of the footprint, and the footprint must stay inside the image and never be empty"""
    index = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    for l in range(n_levels):
        s = first_shift + l
        sampled = fr.resize_nn(index, s)
        R, C = sampled.shape
        assert (R, C) == (mr.level_size(rows, s), mr.level_size(cols, s))
        y0, y1 = mr.footprint_ranges(rows, R, s)
        x0, x1 = mr.footprint_ranges(cols, C, s)
        assert np.array_equal(sampled, index[y0][:, x0])
        assert np.all(y0 < y1) and np.all(x0 < x1) and y1.max() <= rows and x1.max() <= cols
        assert np.all(y1 - y0 <= 1 << s) and np.all(x1 - x0 <= 1 << s)
    # 100 x 100 at shift 3: camera rows and columns 96..99 are in no footprint
    if (rows, cols, first_shift) == (100, 100, 3):
        assert mr.footprint_ranges(100, 12, 3)[1].max() == 96


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("rows,cols,first_shift,n_levels", GEOMETRIES)
def test_host_builder_equals_the_restatement(rows, cols, first_shift, n_levels, margin):
    from rgbd_odometry_amd import capi
    for name, mask in masks_of(rows, cols).items():
        got = capi.mask_levels_host(mask, n_levels, first_shift, margin)
        want = mr.keep_levels(mask, n_levels, first_shift, margin)
        assert len(got) == n_levels
        for l in range(n_levels):
            assert got[l].shape == want[l].shape and got[l].dtype == np.uint8, (name, l)
            assert np.array_equal(got[l], want[l]), (name, l, int((got[l] != want[l]).sum()))
        if name == "zero":
            assert all(np.all(k == 255) for k in got)
        if name == "set":
            assert all(np.all(k == 0) for k in got)


def test_restatement_properties():
    """what the definition implies, on the restatement alone: a pixel outside every footprint changes nothing; a corner pixel drops a
    (margin + 1)-square at the level's corner; a larger margin only drops more"""
    m = np.zeros((100, 100), np.uint8)
    m[96:, :] = 1
    m[:, 96:] = 1
    assert np.all(mr.keep_levels(m, 1, 3, 8)[0] == 255)
    c = np.zeros((75, 101), np.uint8)
    c[74, 100] = 1
    for margin in MARGINS:
        k = mr.keep_levels(c, 3, 1, margin)
        # level 0 (38 x 50, shift 1): row 37 covers 74, but the 50 columns cover 0..99 -> column 100 belongs to no level pixel
        assert np.all(k[0] == 255)
        # level 1 (19 x 25, shift 2): row 18 covers 72..74, column 24 covers 96..99 -> not column 100
        assert np.all(k[1] == 255)
        # level 2 (9 x 13, shift 3): rows 0..8 cover 0..71 -> row 74 belongs to no level pixel
        assert np.all(k[2] == 255)
    d = np.zeros((96, 128), np.uint8)
    d[0, 0] = 1
    prev = None
    for margin in MARGINS:
        k = mr.keep_levels(d, 3, 1, margin)
        for l in range(3):
            want = np.full(k[l].shape, 255, np.uint8)
            want[:margin + 1, :margin + 1] = 0
            assert np.array_equal(k[l], want)
        if prev is not None:
            assert all(np.all(a <= b) for a, b in zip(k, prev))
        prev = k


def test_refusals_of_the_host_builder():
    import ctypes as C
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    mask = np.zeros((24, 32), np.uint8)
    planes = [np.full(24 * 32, 77, np.uint8) for _ in range(capi.DVO_MAX_LEVELS)]
    keep = (C.c_void_p * capi.DVO_MAX_LEVELS)(*[p.ctypes.data for p in planes])
    lr, lc = (C.c_int * 8)(*[-5] * 8), (C.c_int * 8)(*[-5] * 8)

    def call(rows=24, cols=32, m=mask, n_levels=2, first_shift=1, margin=2, k=keep):
        return lib.dvo_mask_levels_host(rows, cols, None if m is None else m.ctypes.data_as(C.c_void_p), n_levels, first_shift, margin, k, lr, lc)

    assert call() == capi.DVO_OK and list(lr)[:2] == [12, 6] and list(lc)[:2] == [16, 8]
    for p in planes:
        p[:] = 77
    lr[0] = lc[0] = -5
    bad = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(m=None), dict(k=None), dict(n_levels=0), dict(n_levels=capi.DVO_MAX_LEVELS + 1),
           dict(first_shift=-1), dict(margin=-1), dict(margin=capi.DVO_MASK_MAX_MARGIN + 1),
           dict(n_levels=6, first_shift=1),          # 24 * 2^-6 = 0.375 -> an empty level
           dict(first_shift=40), dict(first_shift=2 ** 31 - 1)]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
    one_null = (C.c_void_p * capi.DVO_MAX_LEVELS)(planes[0].ctypes.data, None)
    assert call(k=one_null) == capi.DVO_ERR_INVALID
    assert all(np.all(p == 77) for p in planes) and lr[0] == -5 and lc[0] == -5, "a refused call must write nothing"
    assert call(margin=capi.DVO_MASK_MAX_MARGIN, n_levels=5) == capi.DVO_OK          # 24 * 2^-5 = 0.75 -> 1: the last level is 1 x 1
    assert (lr[4], lc[4]) == (1, 1)
    with pytest.raises(capi.DvoError) as ei:
        capi.mask_levels_host(mask, 2, 1, 9)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.mask_levels_host(np.zeros(5, np.uint8), 1, 0, 0)


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in ("dvo_mask_levels_host", "dvo_frames_set_pair_mask", "dvo_frames_get_pair_mask_level", "dvo_tracker_set_stream_mask"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    for macro, value in (("DVO_MASK_MAX_MARGIN", capi.DVO_MASK_MAX_MARGIN), ("DVO_FRAMES_MASK_LAUNCHES", capi.DVO_FRAMES_MASK_LAUNCHES)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == value
    assert capi.DVO_MASK_MAX_MARGIN == mr.MAX_MARGIN and capi.DVO_MAX_LEVELS == mr.MAX_LEVELS


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mask_levels")
    exe = str(d / "mask_levels_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "mask_levels_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/mask_levels_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def run_program(host_program, mask, n_levels, first_shift, margin):
    d, exe = host_program
    path = str(d / "mask.bin")
    np.ascontiguousarray(mask, np.uint8).tofile(path)
    run = subprocess.run([exe, path, str(mask.shape[0]), str(mask.shape[1]), str(n_levels), str(first_shift), str(margin)],
                         capture_output=True, text=True, timeout=60)
    if run.returncode == 3:
        assert run.stdout.strip() == "refused"
        return None
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    out = []
    for l in range(n_levels):
        tag, ll, r, c = lines[2 * l].split()
        assert tag == "level" and int(ll) == l
        plane = np.frombuffer(bytes.fromhex(lines[2 * l + 1]), np.uint8)
        out.append(plane.reshape(int(c), int(r)).T.copy())       # column-major -> (rows, cols)
    return out


@pytest.mark.parametrize("rows,cols,first_shift,n_levels", GEOMETRIES)
def test_builder_under_sanitizers(host_program, rows, cols, first_shift, n_levels):
    """the same code the library compiles, with every plane allocated to its exact size: byte-equal to the restatement and clean
    under -fsanitize=address,undefined"""
    masks = masks_of(rows, cols)
    for name in ("scene", "corner_br", "set", "sparse"):
        for margin in (0, 2, 8):
            got = run_program(host_program, masks[name], n_levels, first_shift, margin)
            want = mr.keep_levels(masks[name], n_levels, first_shift, margin)
            assert got is not None and all(np.array_equal(g, w) for g, w in zip(got, want)), (name, margin)


def test_program_refuses_what_the_builder_refuses(host_program):
    m = np.zeros((24, 32), np.uint8)
    assert run_program(host_program, m, 2, 1, 2) is not None
    for n_levels, first_shift, margin in ((0, 1, 2), (9, 0, 2), (2, -1, 2), (2, 1, 9), (2, 1, -1), (6, 1, 0), (1, 31, 0), (1, 63, 0)):
        assert run_program(host_program, m, n_levels, first_shift, margin) is None
