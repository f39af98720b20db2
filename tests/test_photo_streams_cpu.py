"""CPU checks of the multi-stream photometric engine (include/dvo_amd.h, "many camera streams on the photometric engine"): the header
declares it, the library exports it, the binding mirrors its parameter struct, the C++ mirror builds, and without a HIP device it
fails loudly."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["dvo_photo_streams_params_default", "dvo_photo_streams_create", "dvo_photo_streams_destroy", "dvo_photo_streams_last_error",
           "dvo_photo_streams_reset_stream", "dvo_photo_streams_step", "dvo_photo_streams_get_jacobian", "dvo_photo_streams_get_stats",
           "dvo_photo_streams_context"]


def _declared():
    src = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    return set(re.findall(r"\b(dvo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


def test_header_library_and_binding_have_photo_streams():
    from rgbd_odometry_amd import capi
    declared = _declared()
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in capi.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    from rgbd_odometry_amd import DvoPhotoStreams  # noqa: F401


def test_param_defaults_are_the_reference_literals():
    """ref_every 10000 (RGBDOdometry.cpp:146), first_level 1 (:373), levels 3 then 2 (:162-163), the photometric constants (:32-34)"""
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    p = capi.DvoPhotoStreamsParams()
    assert lib.dvo_photo_streams_params_default(ctypes.byref(p)) == 0
    assert p.ref_every == 10000 and p.first_level == 1
    assert p.n_run == 2 and list(p.levels)[:2] == [3, 2] and list(p.levels)[2:] == [0] * (capi.DVO_MAX_LEVELS - 2)
    assert (p.rows, p.cols) == (480, 640)
    q = p.photo
    assert (q.gradient_threshold, q.max_jacobian_size, q.min_required_pts, q.iterations) == (5, 50000, 100, 3)
    assert q.eps_norm_stop == 200.0 and q.fixed == 0


def test_params_layout_matches_c(tmp_path):
    from rgbd_odometry_amd import capi
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu", sizeof(dvo_photo_streams_params), '
                   'offsetof(dvo_photo_streams_params, ref_every), offsetof(dvo_photo_streams_params, first_level), '
                   'offsetof(dvo_photo_streams_params, n_run), offsetof(dvo_photo_streams_params, levels), '
                   'offsetof(dvo_photo_streams_params, rows), offsetof(dvo_photo_streams_params, cols));return 0;}')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = capi.DvoPhotoStreamsParams
    assert got == [ctypes.sizeof(P), P.ref_every.offset, P.first_level.offset, P.n_run.offset, P.levels.offset, P.rows.offset,
                   P.cols.offset]


def test_mirror_header_compiles(tmp_path):
    """dvo_amd::RGBDOdometryStreams builds into a small program that links the library"""
    src = tmp_path / "m.cpp"
    src.write_text('#include "dvo_amd.hpp"\n#include <cstdio>\nint main(int argc, char **) {\n'
                   '  if (argc > 1) { dvo_amd::RGBDOdometryStreams s(2); s.refEvery = 5; s.setCameraMatrix(525, 525, 319.5, 239.5);\n'
                   '    std::vector<dvo_amd::Pose> p = s.processFrames({}, {}, {}); std::printf("%zu\\n", p.size()); }\n'
                   '  std::puts("ok"); return 0; }\n')
    exe = tmp_path / "m"
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", lib, "-ldvo_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    from rgbd_odometry_amd import DvoError, DvoPhotoStreams
    from rgbd_odometry_amd.capi import DVO_ERR_NO_DEVICE
    with pytest.raises(DvoError) as ei:
        DvoPhotoStreams(4, (525.0, 525.0, 319.5, 239.5))
    assert ei.value.code == DVO_ERR_NO_DEVICE
    assert "no CPU fallback" in str(ei.value)


def test_refusals_before_any_device_work():
    """bad creation arguments are refused with DVO_ERR_INVALID before the device is touched"""
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    h = ctypes.c_void_p()

    def params(**kw):
        p = capi.DvoPhotoStreamsParams()
        lib.dvo_photo_streams_params_default(ctypes.byref(p))
        p.photo.fx, p.photo.fy, p.photo.cx, p.photo.cy = 525.0, 525.0, 319.5, 239.5
        for k, v in kw.items():
            if k == "levels":
                p.n_run = len(v)
                for r, l in enumerate(v):
                    p.levels[r] = l
            elif k in ("iterations", "fx"):
                setattr(p.photo, k, v)
            else:
                setattr(p, k, v)
        return p

    bad = [(params(), 0), (params(fx=0.0), 4), (params(ref_every=0), 4), (params(first_level=4), 4), (params(levels=(3, 0)), 4),
           (params(first_level=2, levels=(3, 1)), 4), (params(levels=(4,)), 4), (params(iterations=33), 4), (params(rows=0), 4)]
    for p, k in bad:
        assert lib.dvo_photo_streams_create(ctypes.byref(p), k, ctypes.byref(h)) == capi.DVO_ERR_INVALID
        assert lib.dvo_photo_streams_last_error(None)
    assert lib.dvo_photo_streams_create(None, 4, ctypes.byref(h)) == capi.DVO_ERR_INVALID
    assert lib.dvo_photo_streams_step(None, 1, None, None, None, 0, 0, 0, None, None, None, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_photo_streams_context(None) is None
