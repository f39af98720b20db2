"""Depth registration on the CPU (include/dvo_amd.h, "depth registration"): dvo_depth_register_host against the numpy restatement of
the definition (tests/depth_register_reference.py) on every case, for 16-bit and float input, the properties the definition promises,
every refusal, and the builder's own code (rgbd_odometry_amd/csrc/dvo_depth_register.h) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/host/depth_register_main.cpp).  No GPU: the builder needs neither a device nor a context.
All comparisons are byte equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_register_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(96, 128), (75, 101), (60, 80)]          # 75 x 101: an odd pixel count


def c_rig(g):
    from rgbd_odometry_amd import capi
    return capi.DvoDepthRig.make(g["depth_shape"], g["Kd4"], g["Kc4"], R=g["R"], t=g["t"], Dc5=g["Dc5"])


def formats_of(depth):
    """the inputs one case stands for: (tag, image)"""
    return [("f32", depth)] if depth.dtype == np.float32 else [("u16", depth), ("f32", dr.as_f32(depth))]


@pytest.mark.parametrize("rows,cols", SIZES)
def test_host_builder_equals_the_restatement(rows, cols):
    from rgbd_odometry_amd import capi
    for name, g, depth in dr.cases(rows, cols):
        for tag, d in formats_of(depth):
            got = capi.depth_register_host(c_rig(g), d, rows, cols)
            want = dr.register(g, d, rows, cols)
            assert got.shape == (rows, cols) and got.dtype == np.uint16
            assert np.array_equal(got, want), (name, tag, int((got != want).sum()))


@pytest.mark.parametrize("rows,cols", SIZES)
def test_properties(rows, cols):
    """what the definition promises, on the host builder's output"""
    from rgbd_odometry_amd import capi
    by_name = {name: (g, d) for name, g, d in dr.cases(rows, cols)}

    def run(name, depth=None):
        g, d = by_name[name]
        return capi.depth_register_host(c_rig(g), d if depth is None else depth, rows, cols)

    g, d = by_name["identity"]
    assert np.array_equal(run("identity"), d)                                   # byte for byte, holes included
    assert np.array_equal(run("identity", dr.as_f32(d)), d)                     # millimetre-valued metres come back as they were
    assert 0.05 < (d == 0).mean() < 0.15
    for name in ("plane_60x80", "plane_96x128"):                                # up- and down-scaled: no hole
        out = run(name)
        assert np.all(out == 1500), (name, int((out == 0).sum()))
    # a 50 mm baseline: the box wins where both land, and leaves an occlusion shadow
    g, d = by_name["baseline_box"]
    _, box = dr.box_scene((rows, cols))
    only_box, only_back = np.where(box, d, 0).astype(np.uint16), np.where(box, 0, d).astype(np.uint16)
    out, ob, ok = run("baseline_box"), run("baseline_box", only_box), run("baseline_box", only_back)
    both = (ob != 0) & (ok != 0)
    assert both.any() and np.array_equal(out[both], ob[both]) and np.all(ob[both] < ok[both])
    assert np.array_equal(out, np.where(ob != 0, ob, ok))
    share = (out == 0).mean()
    print("baseline_box %dx%d: hole share %.4f" % (rows, cols, share))
    assert 0 < share < 0.05
    # the clamp: four pixels, 12 colour pixels wide each, write 8 x 8 each
    out = run("clamp_12x")
    assert int((out != 0).sum()) == 4 * dr.SPLAT_MAX * dr.SPLAT_MAX and np.all(out[out != 0] == 2000)
    for name in ("behind", "f32_far", "outside", "all_zero"):
        assert not run(name).any(), name
    # NaN, +-inf, 0 and negative values are no measurements: the same image with zeros in their place registers alike
    g, d = by_name["f32_specials"]
    bad = ~(np.isfinite(d) & (d > 0))
    assert np.isnan(d).any() and np.isposinf(d).any() and (d == 0).any() and (d < 0).any() and bad.mean() > 0.2
    assert np.array_equal(run("f32_specials"), run("f32_specials", np.where(bad, np.float32(0), d)))
    assert run("f32_specials").any()
    # 65.535 m + 1 m does not fit 16 bits, 64 m + 1 m does
    out = run("q_beyond")
    assert set(np.unique(out)) == {0, 65000}
    out = run("partly_outside")
    assert 0.1 < (out == 0).mean() < 0.9


def test_refusals_of_the_host_builder():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    rows, cols = 24, 32
    K = dr.colour_K(rows, cols)
    depth = np.full((rows, cols), 1000, np.uint16)
    out = np.full((rows, cols), 0xABCD, np.uint16)

    def call(rig_edit=None, rig_null=False, depth_null=False, out_null=False, fmt=capi.DVO_DEPTH_U16, r=rows, c=cols):
        g = capi.DvoDepthRig.make((rows, cols), K, K, Dc5=[0.1, 0, 0, 0, 0])
        if rig_edit:
            rig_edit(g)
        return lib.dvo_depth_register_host(None if rig_null else C.byref(g), None if depth_null else capi._ptr(depth), fmt, r, c,
                                           None if out_null else capi._ptr(out))

    def setter(field, index, value):
        def edit(g):
            if index is None:
                setattr(g, field, value)
            else:
                getattr(g, field)[index] = value
        return edit

    assert call() == capi.DVO_OK and out[12, 16] == 1000
    out[:] = 0xABCD
    bad = [dict(rig_null=True), dict(depth_null=True), dict(out_null=True), dict(r=0), dict(c=0), dict(r=-3), dict(fmt=2), dict(fmt=-1),
           dict(rig_edit=setter("depth_rows", None, 0)), dict(rig_edit=setter("depth_cols", None, -1)),
           dict(rig_edit=setter("has_Dc5", None, 2)), dict(rig_edit=setter("has_Dc5", None, -1))]
    for field, index in (("Kd4", 0), ("Kd4", 1), ("Kc4", 0), ("Kc4", 1)):
        bad += [dict(rig_edit=setter(field, index, 0.0)), dict(rig_edit=setter(field, index, -100.0))]
    for field, n in (("Kd4", 4), ("R", 9), ("t", 3), ("Kc4", 4), ("Dc5", 5)):
        for index in range(n):
            for value in (float("nan"), float("inf"), float("-inf")):
                bad.append(dict(rig_edit=setter(field, index, value)))
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
    assert np.all(out == 0xABCD), "a refused call must write nothing"
    with pytest.raises(capi.DvoError) as ei:
        capi.depth_register_host(capi.DvoDepthRig.make((rows, cols), [0, 1, 0, 0], K), depth, rows, cols)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.depth_register_host(capi.DvoDepthRig.make((rows, cols + 1), K, K), depth, rows, cols)
    # R is taken as given: a matrix that is no rotation is not refused
    assert call(rig_edit=setter("R", 0, 2.0)) == capi.DVO_OK


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in ("dvo_depth_register_host", "dvo_frames_set_pair_depth_rig", "dvo_frames_register_depth", "dvo_frames_get_registered_depth",
                 "dvo_tracker_set_stream_depth_rig", "dvo_tracker_step_raw_depth"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    for macro, value in (("DVO_DEPTH_SPLAT_MAX", capi.DVO_DEPTH_SPLAT_MAX), ("DVO_DEPTH_REGISTER_LAUNCHES", capi.DVO_DEPTH_REGISTER_LAUNCHES)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == value
    assert capi.DVO_DEPTH_SPLAT_MAX == dr.SPLAT_MAX
    # the rig is declared twice under one guard (the public header and the definition's own): the two texts must be the same
    own = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_depth_register.h")).read(), flags=re.S)
    pat = r"typedef struct dvo_depth_rig \{.*?\} dvo_depth_rig;"
    assert re.search(pat, text, re.S).group(0).split() == re.search(pat, own, re.S).group(0).split()


def test_rig_layout_matches_header(tmp_path):
    """the ctypes mirror must have the layout the C compiler gives dvo_depth_rig"""
    from rgbd_odometry_amd import capi
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu", '
                   'sizeof(dvo_depth_rig), offsetof(dvo_depth_rig, Kd4), offsetof(dvo_depth_rig, t), offsetof(dvo_depth_rig, has_Dc5), '
                   'offsetof(dvo_depth_rig, Dc5));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, kd, t, has, dc = (int(x) for x in subprocess.check_output([exe]).split())
    R = capi.DvoDepthRig
    assert (C.sizeof(R), R.Kd4.offset, R.t.offset, R.has_Dc5.offset, R.Dc5.offset) == (size, kd, t, has, dc)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_register")
    exe = str(d / "depth_register_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "depth_register_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/depth_register_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def run_program(host_program, rig, depth, fmt, rows, cols):
    d, exe = host_program
    rig_path, depth_path = str(d / "rig.bin"), str(d / "depth.bin")
    open(rig_path, "wb").write(bytes(rig))
    np.ascontiguousarray(depth).tofile(depth_path)
    run = subprocess.run([exe, rig_path, depth_path, str(fmt), str(rows), str(cols)], capture_output=True, text=True, timeout=60)
    if run.returncode == 3:
        assert run.stdout.strip() == "refused"
        return None
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    tag, r, c = lines[0].split()
    assert tag == "image" and (int(r), int(c)) == (rows, cols)
    return np.frombuffer(bytes.fromhex(lines[1]), ">u2").astype(np.uint16).reshape(rows, cols)


@pytest.mark.parametrize("rows,cols", SIZES)
def test_builder_under_sanitizers(host_program, rows, cols):
    """the same code the library compiles, with the depth image and the output allocated to their exact sizes: byte-equal to the
    restatement and clean under -fsanitize=address,undefined"""
    from rgbd_odometry_amd import capi
    for name, g, depth in dr.cases(rows, cols):
        for tag, d in formats_of(depth):
            got = run_program(host_program, c_rig(g), d, capi.DVO_DEPTH_U16 if tag == "u16" else capi.DVO_DEPTH_F32, rows, cols)
            assert got is not None and np.array_equal(got, dr.register(g, d, rows, cols)), (name, tag)


def test_program_refuses_what_the_builder_refuses(host_program):
    from rgbd_odometry_amd import capi
    rows, cols = 24, 32
    K = dr.colour_K(rows, cols)
    depth = np.full((rows, cols), 1000, np.uint16)
    mk = lambda **kw: capi.DvoDepthRig.make((rows, cols), kw.get("Kd", K), kw.get("Kc", K), t=kw.get("t"), Dc5=kw.get("Dc5"))
    assert run_program(host_program, mk(), depth, 1, rows, cols) is not None
    for rig in (mk(Kd=[0, 1, 0, 0]), mk(Kc=[1, -1, 0, 0]), mk(t=[float("nan"), 0, 0]), mk(Dc5=[0, 0, float("inf"), 0, 0])):
        assert run_program(host_program, rig, depth, 1, rows, cols) is None
    g = mk()
    g.has_Dc5 = 3
    assert run_program(host_program, g, depth, 1, rows, cols) is None
    g = mk()
    g.depth_rows = 0
    assert run_program(host_program, g, depth, 1, rows, cols) is None
    for fmt, r, c in ((2, rows, cols), (1, 0, cols), (1, rows, -1)):
        assert run_program(host_program, mk(), depth, fmt, r, c) is None
