"""Ray casting of fused volumes on the CPU (include/dvo_amd.h, "from the map back to depth"): dvo_raycast_host against the numpy
restatement of the definition (tests/tsdf_raycast_reference.py) on every volume, view and setting and in both depth formats, conditions
that keep those cases from being vacuous, the accuracy of the definition against a plane whose place is known, the round trip depth ->
volume -> depth, every refusal, the layout of the mirrors, the definition's own code (rgbd_odometry_amd/csrc/dvo_tsdf_raycast.h) as a
stand-alone program under the address and undefined-behaviour sanitizers (tests/host/tsdf_raycast_main.cpp) and the C++ mirror
(tests/host/tsdf_raycast_hpp_main.cpp).  No GPU.  Comparisons are byte equality unless a bound is stated."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_map_reference as tr
import tsdf_raycast_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["u16", "f32"]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_volumes = {}


def volumes():
    """[(name, volume, words)]: the four volumes fused as the fusion tests fuse them (by the host definition), and volume 1 with random
    words; computed once"""
    from rgbd_odometry_amd import capi
    if not _volumes:
        imgs, poses = tr.frame_list("u16")
        out = []
        for vi, vol in enumerate(tr.VOLUMES):
            idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
            w = capi.tsdf_integrate_host(c_volume(vol), None, [imgs[i] for i in idx], tr.K4, poses[idx])
            out.append(("volume%d" % vi, vol, w))
        out.append(("random1", tr.VOLUMES[1], rr.random_words(tr.VOLUMES[1])))
        for _, _, w in out:
            w.setflags(write=False)
        _volumes["all"] = out
    return _volumes["all"]


def host(vol, words, K, poses, rows, cols, fmt, normals, **params):
    from rgbd_odometry_amd import capi
    return capi.tsdf_raycast_host(c_volume(vol), words, K, poses, rows, cols, capi.DvoRaycastParams.default(**params), fmt, normals)


@pytest.mark.parametrize("name", ["volume0", "volume1", "volume2", "volume3", "random1"])
def test_host_equals_the_restatement(name):
    """every view and setting at 24 x 32, the default setting at 37 x 53; both formats, normals on and off"""
    _, vol, words = next(v for v in volumes() if v[0] == name)
    views = rr.view_list(vol)
    poses = np.stack([p for _, p in views])
    kinds = np.zeros(3, np.int64)
    for (rows, cols), settings in ((rr.SIZES[0], rr.SETTINGS), (rr.SIZES[1], rr.SETTINGS[:1])):
        K = rr.k4_for(rows, cols)
        for setting in settings:
            ref = [rr.raycast_view(vol, words, K, p, rows, cols, **setting) for p in poses]
            for v in ref:
                kinds += np.bincount(v["kind"].ravel(), minlength=3)
            for fmt in FORMATS:
                depth, nrm = host(vol, words, K, poses, rows, cols, fmt, True, **setting)
                alone = host(vol, words, K, poses, rows, cols, fmt, False, **setting)
                assert same_bits(depth, alone)
                for i, (view, _) in enumerate(views):
                    where = (name, view, rows, cols, setting, fmt)
                    assert same_bits(depth[i], ref[i][fmt]), where + (int((depth[i] != ref[i][fmt]).sum()),)
                    assert same_bits(nrm[i], ref[i]["normals_" + fmt]), where
    print("%s: rays that ended in a hit %d, at a back face or inside %d, at z_far %d" % (name, kinds[rr.HIT], kinds[rr.BACK], kinds[rr.FAR]))


def test_cases_are_not_vacuous():
    """conditions on the cases, met by the host definition alone"""
    by_name = {name: (vol, words) for name, vol, words in volumes()}
    rows, cols = rr.SIZES[0]
    vol, words = by_name["volume1"]
    depth, nrm = host(vol, words, tr.K4, np.stack(tr.POSES), rows, cols, "f32", True)
    for i in range(len(tr.POSES)):
        hits = int((depth[i] > 0).sum())
        with_normal = int(np.any(nrm[i] != 0, axis=-1).sum())
        print("fused volume 1, fusion pose %d: %d of %d pixels hit, %d with a normal" % (i, hits, rows * cols, with_normal))
        assert 2 * hits >= rows * cols and 2 * with_normal >= hits
        assert not np.any(nrm[i][depth[i] == 0])
    extra = dict(rr.extra_views(vol))
    assert not host(vol, words, tr.K4, extra["looking_away"][None], rows, cols, "f32", False).any()
    back = host(vol, words, tr.K4, extra["three_metres_back"][None], rows, cols, "f32", False)
    assert (back > 3.0).sum() >= 20, "the camera 3 m back still sees the surface"
    # (1, 1, 1) has no cell of eight voxels: no valid sample, nothing but holes, from any view and in any setting
    vol3, words3 = by_name["volume3"]
    assert words3.any()
    for setting in rr.SETTINGS:
        d, n = host(vol3, words3, tr.K4, np.stack([p for _, p in rr.view_list(vol3)]), rows, cols, "u16", True, **setting)
        assert not d.any() and not n.any()
    # (5, 3, 2) is one layer of 4 x 2 cells between its z planes at 0.8 and 0.9 m.  Fused from frame 3, the far plane's middle voxels lie
    # more than trunc behind the scene's box and were never seen (w = 0), and every cell has one of them as a corner: no valid sample,
    # every ray runs to z_far -- in any setting
    vol2, words2 = by_name["volume2"]
    assert (tr.word_w(words2) == 0).any() and (tr.word_w(words2) > 0).sum() >= 15
    for setting in rr.SETTINGS:
        for _, pose in rr.view_list(vol2):
            assert not host(vol2, words2, tr.K4, pose[None], rows, cols, "f32", False, **setting).any()
            assert np.all(rr.raycast_view(vol2, words2, tr.K4, pose, rows, cols, **setting)["kind"] == rr.FAR)
    # the same layer with q = +16384 in the near plane and -16384 in the far one is a surface at exactly 0.85 m: with a quarter-band
    # step the identity camera samples it at 0.8125, 0.85 and 0.8875 m and hits where the ray stays inside the layer's 0.4 x 0.2 m
    crafted = tr.make_words(np.repeat([16384, -16384], 15), np.ones(30, np.int64))
    d = host(vol2, crafted, tr.K4, tr.pose12()[None], rows, cols, "f32", False, step_trunc=0.25)
    print("(5, 3, 2) crafted: %d pixels hit, depths %.9f .. %.9f m" % ((d > 0).sum(), d[d > 0].min(), d[d > 0].max()))
    assert (d > 0).sum() >= 50 and np.all(np.abs(d[d > 0].astype(np.float64) - 0.85) <= 1.2e-7)
    assert np.array_equal(d, rr.raycast_view(vol2, crafted, tr.K4, tr.pose12(), rows, cols, step_trunc=0.25)["f32"][None])
    # the random volume: hits, holes by back face or invalid neighbour, holes by z_far -- each many times; and both weights matter
    vol, words = by_name["random1"]
    kinds = np.zeros(3, np.int64)
    for _, pose in rr.view_list(vol):
        kinds += np.bincount(rr.raycast_view(vol, words, tr.K4, pose, rows, cols)["kind"].ravel(), minlength=3)
    print("random words: hits %d, back faces %d, z_far %d" % (kinds[rr.HIT], kinds[rr.BACK], kinds[rr.FAR]))
    assert kinds[rr.HIT] >= 100 and kinds[rr.BACK] >= 100 and kinds[rr.FAR] >= 100
    a = host(vol, words, tr.K4, tr.POSES[0][None], rows, cols, "u16", False, min_weight=1)
    b = host(vol, words, tr.K4, tr.POSES[0][None], rows, cols, "u16", False, min_weight=2)
    assert not np.array_equal(a, b) and b.any()


PLANE_POSES = [tr.pose12(), tr.pose12(tr.rot(1, 0.15), (0.10, 0.02, 0.0)), tr.pose12(tr.rot(0, -0.2), (0.0, -0.1, 0.05))]


def test_accuracy_of_the_definition():
    """A fronto-parallel plane at 873 mm fused into volume 1 at the identity, ray-cast to f32 from three poses: every hit's world point
    lies within trunc / 32767 + 1.2e-7 m of the plane -- the field is exactly linear in world z inside the band, a trilinear value is a
    convex combination of values with at most half a unit of error each, and 1.2e-7 is the float rounding of a depth near 1 m -- and
    every normal within 2 trunc / (65534 voxel_size) + 1e-6 of (0, 0, -1): each gradient component carries at most one unit of error
    against |G| = 65534 voxel_size / trunc.
    Measured (host definition): worst distance 5.8e-7 m against the bound 1.95e-6 m; every normal is exactly (0, 0, -1), the bound being
    9.3e-5: a plane fused at the identity gives a field that depends on world z alone, so Gx = Gy = 0."""
    from rgbd_odometry_amd import capi
    vol = tr.VOLUMES[1]
    rows, cols = rr.SIZES[0]
    depth = np.full((rows, cols), 873, np.uint16)
    words = capi.tsdf_integrate_host(c_volume(vol), None, [depth], tr.K4, tr.pose12()[None])
    bound = vol["trunc"] / 32767.0 + 1.2e-7
    nbound = 2.0 * vol["trunc"] / (65534.0 * vol["voxel_size"]) + 1e-6
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    xn, yn = (u - tr.K4[2]) / tr.K4[0], (v - tr.K4[3]) / tr.K4[1]
    worst, nworst = 0.0, 0.0
    for step_trunc in (0.5, 0.25):
        d, nrm = host(vol, words, tr.K4, np.stack(PLANE_POSES), rows, cols, "f32", True, step_trunc=step_trunc)
        for i, pose in enumerate(PLANE_POSES):
            hit = d[i] > 0
            Z = d[i].astype(np.float64)
            world_z = pose[2] * (xn * Z) + pose[5] * (yn * Z) + pose[8] * Z + pose[11]
            err = np.abs(world_z[hit] - 0.873).max()
            has_normal = hit & np.any(nrm[i] != 0, axis=-1)
            nerr = np.abs(nrm[i][has_normal].astype(np.float64) - np.array([0.0, 0.0, -1.0])).max()
            print("step_trunc %.2f pose %d: %d of %d pixels hit, worst distance to the plane %.3e m (bound %.3e), %d normals, worst "
                  "deviation %.3e (bound %.3e)" % (step_trunc, i, hit.sum(), rows * cols, err, bound, has_normal.sum(), nerr, nbound))
            assert 2 * hit.sum() >= rows * cols and 2 * has_normal.sum() >= hit.sum()
            assert err <= bound
            assert nerr <= nbound
            worst, nworst = max(worst, err), max(nworst, nerr)
    print("worst distance %.3e m, worst normal deviation %.3e" % (worst, nworst))


def test_round_trip():
    """volume 1 fused from its frames and ray-cast at those frames' poses in u16: over the pixels valid in both images the median of
    |rendered - input| is at most one voxel (the maximum is printed: a pixel at the box's edge sees the other surface)"""
    vol, words = next((vol, w) for name, vol, w in volumes() if name == "volume1")
    imgs, poses = tr.frame_list("u16")
    idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == 1]
    rows, cols = rr.SIZES[0]
    d = host(vol, words, tr.K4, poses[idx], rows, cols, "u16", False)
    for j, i in enumerate(idx):
        both = (d[j] > 0) & (imgs[i] > 0)
        diff = np.abs(d[j].astype(np.int64) - imgs[i].astype(np.int64))[both] / 1000.0
        print("frame %d: %d pixels valid in both, median |rendered - input| %.4f m, maximum %.4f m" % (i, both.sum(), np.median(diff), diff.max()))
        assert 2 * both.sum() >= rows * cols
        assert np.median(diff) <= vol["voxel_size"]


def test_refusals_of_the_host_definition():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol = tr.VOLUMES[0]
    words = next(w for name, _, w in volumes() if name == "volume0")
    rows, cols = rr.SIZES[0]
    depth = np.full((rows, cols), 0x5A5A, np.uint16)
    depth32 = np.full((rows, cols), -7.5, np.float32)
    nrm = np.full((rows, cols, 3), -7.5, np.float32)
    out, out32, none_out, nout = (C.c_void_p * 1)(depth.ctypes.data), (C.c_void_p * 1)(depth32.ctypes.data), (C.c_void_p * 1)(None), (C.c_void_p * 1)(nrm.ctypes.data)

    def call(vol_edit=None, prm_edit=None, K=tr.K4, pose=None, count=1, fmt=capi.DVO_DEPTH_U16, r=rows, c=cols, null=()):
        v, p = c_volume(vol), capi.DvoRaycastParams.default()
        if vol_edit:
            vol_edit(v)
        if prm_edit:
            prm_edit(p)
        Kd = np.array(K, np.float64)
        Pd = tr.POSES[0].copy() if pose is None else np.array(pose, np.float64)
        return lib.dvo_raycast_host(None if "vol" in null else C.byref(v), None if "voxels" in null else capi._ptr(words),
                                    None if "params" in null else C.byref(p), count, fmt, r, c,
                                    None if "K4" in null else capi._ptr(Kd), None if "poses" in null else capi._ptr(Pd),
                                    None if "depth" in null else (none_out if "image" in null else (out32 if fmt == capi.DVO_DEPTH_F32 else out)),
                                    none_out if "normal" in null else nout)

    def setter(field, value, index=None):
        def edit(o):
            if index is None:
                setattr(o, field, value)
            else:
                getattr(o, field)[index] = value
        return edit

    untouched = lambda: np.all(depth == 0x5A5A) and np.all(depth32 == -7.5) and np.all(nrm == -7.5)
    assert call() == capi.DVO_OK and depth.any() and not np.all(depth == 0x5A5A) and not np.all(nrm == -7.5) and np.all(depth32 == -7.5)
    assert call(fmt=capi.DVO_DEPTH_F32) == capi.DVO_OK and not np.all(depth32 == -7.5)
    depth[:], depth32[:], nrm[:] = 0x5A5A, -7.5, -7.5
    nan, inf = float("nan"), float("inf")
    bad = [dict(null=(k,)) for k in ("vol", "voxels", "params", "depth", "image", "normal", "K4", "poses")]
    bad += [dict(count=0), dict(count=-1), dict(r=0), dict(c=0), dict(r=-2), dict(c=-1), dict(fmt=2), dict(fmt=-1)]
    for field in ("nx", "ny", "nz"):
        bad += [dict(vol_edit=setter(field, 0)), dict(vol_edit=setter(field, -1)), dict(vol_edit=setter(field, capi.DVO_TSDF_MAX_DIM + 1))]
    for field in ("voxel_size", "trunc"):
        bad += [dict(vol_edit=setter(field, value)) for value in (0.0, -0.1, nan, inf)]
    bad += [dict(vol_edit=setter("origin", value, k)) for k in range(3) for value in (nan, inf, -inf)]
    bad += [dict(prm_edit=setter("z_near", value)) for value in (0.0, -1.0, 8.0, 9.0, nan, inf)]
    bad += [dict(prm_edit=setter("z_far", value)) for value in (0.1, 0.05, nan, inf)]
    bad += [dict(prm_edit=setter("step_trunc", value)) for value in (0.0, -0.5, float(np.nextafter(1.0, 2.0)), 2.0, nan, inf)]
    bad += [dict(prm_edit=setter("min_weight", value)) for value in (0, -1, 65536)]
    # the march has (8 - 0.1) / (step_trunc * trunc) samples
    bad += [dict(prm_edit=setter("step_trunc", 1e-5)), dict(prm_edit=setter("step_trunc", 5e-324)), dict(vol_edit=setter("trunc", 1e-6))]
    for k in range(4):
        bad += [dict(K=[value if j == k else tr.K4[j] for j in range(4)]) for value in (nan, inf, -inf)]
    bad += [dict(K=[0.0, 30.0, 15.5, 11.5]), dict(K=[30.0, -30.0, 15.5, 11.5])]
    for k in range(12):
        bad += [dict(pose=[value if j == k else tr.pose12()[j] for j in range(12)]) for value in (nan, inf)]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
        assert untouched(), kw
    # the limit of the march itself: z_near + step k <= z_far for exactly 65536 values of k is taken, for 65537 refused
    step = 2.0 ** -13
    for z_far, want in ((1.0 + step * 65535, capi.DVO_OK), (1.0 + step * 65536, capi.DVO_ERR_INVALID)):
        def edit(p, z_far=z_far):
            p.z_near, p.z_far, p.step_trunc = 1.0, z_far, 1.0
        assert call(vol_edit=setter("trunc", step), prm_edit=edit) == want, z_far
    depth[:], nrm[:] = 0x5A5A, -7.5
    # R is taken as given; normals_out may be NULL as a whole
    assert call(pose=[2.0] + list(tr.pose12()[1:])) == capi.DVO_OK
    v, p = c_volume(vol), capi.DvoRaycastParams.default()
    assert lib.dvo_raycast_host(C.byref(v), capi._ptr(words), C.byref(p), 1, capi.DVO_DEPTH_U16, rows, cols, capi._ptr(np.array(tr.K4)),
                                capi._ptr(tr.pose12()), out, None) == capi.DVO_OK
    with pytest.raises(capi.DvoError) as ei:
        capi.tsdf_raycast_host(c_volume(dict(vol, trunc=0.0)), words, tr.K4, tr.pose12()[None], rows, cols)
    assert ei.value.code == capi.DVO_ERR_INVALID
    assert lib.dvo_raycast_params_default(None) == capi.DVO_ERR_INVALID
    p = capi.DvoRaycastParams.default()
    assert (p.z_near, p.z_far, p.step_trunc, p.min_weight) == (0.1, 8.0, 0.5, 1) == (rr.Z_NEAR, rr.Z_FAR, rr.STEP_TRUNC, rr.MIN_WEIGHT)
    assert lib.dvo_raycast_views(None, None, 1, None, 0, 1, 1, None, None, None, None, 0) == capi.DVO_ERR_INVALID


def test_symbols_constants_and_struct_text():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    names = ["dvo_raycast_params_default", "dvo_raycast_host", "dvo_raycast_views"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    assert sorted(n for n in capi.C_ABI_SYMBOLS if n.startswith("dvo_raycast_")) == sorted(names)
    launch = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_launch.h")).read()
    assert int(re.search(r"#define\s+DVO_RAYCAST_LAUNCHES\s+(\d+)", text).group(1)) == capi.DVO_RAYCAST_LAUNCHES == 1
    assert int(re.search(r"constexpr int kRaycastLaunches = (\d+);", launch).group(1)) == capi.DVO_RAYCAST_LAUNCHES
    assert int(re.search(r"#define\s+DVO_RAYCAST_MAX_STEPS\s+(\d+)", text).group(1)) == capi.DVO_RAYCAST_MAX_STEPS == rr.MAX_STEPS
    hip = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_raycast.hip")).read()
    body = hip.split("int launch_tsdf_raycast(")[1].split("\n}\n")[0]
    assert body.count("hipLaunchKernelGGL(") == capi.DVO_RAYCAST_LAUNCHES
    # the struct is declared twice under one guard (the public header and the definition's own): the two texts must be the same
    own = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_raycast.h")).read(), flags=re.S)
    pat = r"typedef struct dvo_raycast_params \{.*?\} dvo_raycast_params;"
    assert re.search(pat, text, re.S).group(0).split() == re.search(pat, own, re.S).group(0).split()
    assert "#ifndef DVO_RAYCAST_TYPES_DEFINED_" in text and "#ifndef DVO_RAYCAST_TYPES_DEFINED_" in own
    assert int(re.search(r"#define\s+DVO_RAYCAST_MAX_STEPS\s+(\d+)", own).group(1)) == capi.DVO_RAYCAST_MAX_STEPS


def test_struct_layout_matches_header(tmp_path):
    """the ctypes mirror must have the layout the C compiler gives dvo_raycast_params"""
    from rgbd_odometry_amd import capi
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu %zu", '
                   'sizeof(dvo_raycast_params), offsetof(dvo_raycast_params, z_far), offsetof(dvo_raycast_params, step_trunc), '
                   'offsetof(dvo_raycast_params, min_weight));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = tuple(int(x) for x in subprocess.check_output([exe]).split())
    P = capi.DvoRaycastParams
    assert (C.sizeof(P), P.z_far.offset, P.step_trunc.offset, P.min_weight.offset) == got


# ---- the definition's own code under sanitizers, and the C++ mirror ----

def write_case(d, vol, words, K, poses, params=None):
    from rgbd_odometry_amd import capi
    paths = {k: str(d / (k + ".bin")) for k in ("volume", "params", "words", "views")}
    open(paths["volume"], "wb").write(bytes(c_volume(vol)))
    open(paths["params"], "wb").write(bytes(params if params is not None else capi.DvoRaycastParams.default()))
    np.asarray(words, np.uint32).tofile(paths["words"])
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    np.concatenate([np.broadcast_to(np.array(K, np.float64), (len(poses), 4)).ravel(), poses.ravel()]).tofile(paths["views"])
    return paths


def parse_output(stdout, count, rows, cols, fmt):
    lines = stdout.splitlines()
    assert lines[0].split() == ["depth", str(count * rows * cols)] and lines[2].split() == ["normals", str(count * rows * cols)]
    if fmt == "u16":
        depth = np.frombuffer(bytes.fromhex(lines[1]), ">u2").astype(np.uint16).reshape(count, rows, cols)
    else:
        depth = np.frombuffer(bytes.fromhex(lines[1]), ">u4").astype(np.uint32).view(np.float32).reshape(count, rows, cols)
    nrm = np.frombuffer(bytes.fromhex(lines[3]), ">u4").astype(np.uint32).view(np.float32).reshape(count, rows, cols, 3)
    return depth, nrm, lines[4:]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_raycast")
    exe = str(d / "tsdf_raycast_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tsdf_raycast_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/tsdf_raycast_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def run_program(host_program, vol, words, K, poses, fmt, rows, cols, params=None, count=None):
    from rgbd_odometry_amd import capi
    d, exe = host_program
    p = write_case(d, vol, words, K, poses, params)
    n = len(poses) if count is None else count
    code = {"u16": capi.DVO_DEPTH_U16, "f32": capi.DVO_DEPTH_F32}.get(fmt, fmt)
    run = subprocess.run([exe, p["volume"], p["params"], p["words"], p["views"], str(code), str(rows), str(cols), str(n)],
                         capture_output=True, text=True, timeout=300)
    if run.returncode == 3:
        assert run.stdout.strip() == "refused"
        return None
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    depth, nrm, rest = parse_output(run.stdout, n, rows, cols, fmt)
    assert rest == ["clipped equal 1"], rest[:1]
    return depth, nrm


@pytest.mark.parametrize("fmt", FORMATS)
def test_definition_under_sanitizers(host_program, fmt):
    """the same code the library compiles, with every buffer allocated to its exact size: the library's bytes, clean under
    -fsanitize=address,undefined, and the march clipped to the volume's box (what the kernel runs) gives the same bytes as the whole one"""
    from rgbd_odometry_amd import capi
    for name, vol, words in volumes():
        poses = np.stack([p for _, p in rr.view_list(vol)])
        for (rows, cols), settings in ((rr.SIZES[0], rr.SETTINGS), (rr.SIZES[1], rr.SETTINGS[:1])):
            K = rr.k4_for(rows, cols)
            for setting in settings:
                got = run_program(host_program, vol, words, K, poses, fmt, rows, cols, capi.DvoRaycastParams.default(**setting))
                assert got is not None, name
                want = host(vol, words, K, poses, rows, cols, fmt, True, **setting)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, fmt, rows, cols, setting)


def test_program_refuses_what_the_definition_refuses(host_program):
    from rgbd_odometry_amd import capi
    name, vol, words = volumes()[0]
    pose, (rows, cols) = tr.POSES[0][None], rr.SIZES[0]
    assert run_program(host_program, vol, words, tr.K4, pose, "u16", rows, cols) is not None
    for bad in (dict(vol, trunc=0.0), dict(vol, voxel_size=float("nan")), dict(vol, origin=(0.0, float("inf"), 0.0))):
        assert run_program(host_program, bad, words, tr.K4, pose, "u16", rows, cols) is None
    P = capi.DvoRaycastParams.default
    for kw in (dict(fmt=2), dict(rows=0), dict(cols=-1), dict(count=-1), dict(count=0), dict(params=P(min_weight=0)), dict(params=P(z_near=9.0)),
               dict(params=P(step_trunc=1.5)), dict(params=P(step_trunc=1e-6))):
        args = dict(fmt="u16", rows=rows, cols=cols)
        args.update(kw)
        assert run_program(host_program, vol, words, tr.K4, pose, **args) is None, kw
    bad_pose = pose.copy()
    bad_pose[0, 10] = np.nan
    assert run_program(host_program, vol, words, tr.K4, bad_pose, "u16", rows, cols) is None


# ---- the domain of clip(): rr.domain_views ----

_domain = {}


def domain_results(host_program):
    """every case of rr.domain_views through the stand-alone program, which marches each view whole and clipped under the sanitizers and
    says whether the bytes are the same: (cases, [(depth, normals) of the whole march]); run once, eight programs at a time"""
    from concurrent.futures import ThreadPoolExecutor
    from rgbd_odometry_amd import capi
    if "out" not in _domain:
        d, exe = host_program
        cases = rr.domain_views(0)
        rows, cols = rr.DOMAIN_SIZE

        def run(i):
            c = cases[i]
            sub = d / ("domain%03d" % i)
            sub.mkdir(exist_ok=True)
            try:
                got = run_program((sub, exe), c["vol"], c["words"], c["K4"], c["pose"][None], c["fmt"], rows, cols, capi.DvoRaycastParams.default(**c["params"]))
            except AssertionError as e:
                raise AssertionError("case %d (%s): %s" % (i, c["category"], e))
            assert got is not None, "case %d (%s) was refused" % (i, c["category"])
            return got[0][0], got[1][0]

        with ThreadPoolExecutor(max_workers=8) as pool:
            _domain["out"] = (cases, list(pool.map(run, range(len(cases)))))
    return _domain["out"]


def test_clip_domain(host_program):
    """the clipped march equals the whole one ("clipped equal 1", asserted per case by run_program) on every case of rr.domain_views:
    rays exactly parallel to slabs, cameras on lattice planes, volumes far from the origin, z_near and z_far inside the volume, samples on a face of the box, marches
    of 63,334 samples; and the program's bytes are the library's"""
    from rgbd_odometry_amd import capi
    cases, results = domain_results(host_program)
    rows, cols = rr.DOMAIN_SIZE
    assert 400 <= len(cases) <= 460
    for i, (c, (depth, nrm)) in enumerate(zip(cases, results)):
        want = host(c["vol"], c["words"], c["K4"], c["pose"][None], rows, cols, c["fmt"], True, **c["params"])
        assert same_bits(depth, want[0][0]) and same_bits(nrm, want[1][0]), (i, c["category"])
    assert len(rr.domain_groups(cases)) <= 36, "a few dozen ray-cast calls take all cases"


def test_clip_domain_is_not_vacuous(host_program):
    """conditions on rr.domain_views, from the whole march alone: hits are common, in every category, and on the rays with xn == 0 or
    yn == 0"""
    cases, results = domain_results(host_program)
    rows, cols = rr.DOMAIN_SIZE
    hits = sum(int((depth != 0).sum()) for depth, _ in results)
    print("%d cases, %d of %d pixels hit" % (len(cases), hits, len(cases) * rows * cols))
    assert 100 * hits >= 15 * len(cases) * rows * cols
    categories = {"axis", "perturbed", "lattice", "inside", "back", "far_origin", "sizes", "z_range", "step", "on_sample", "long_march"}
    assert {c["category"] for c in cases} == categories
    for category in sorted(categories):
        mine = [depth != 0 for c, (depth, _) in zip(cases, results) if c["category"] == category]
        print("%-10s %3d views, %3d with a hit, %3d with a hole" % (category, len(mine), sum(h.any() for h in mine), sum((~h).any() for h in mine)))
        assert any(h.any() for h in mine) and any((~h).any() for h in mine), category
    on_axis = 0
    for c, (depth, _) in zip(cases, results):
        fx, fy, cx, cy = c["K4"]
        xn, yn = (np.arange(cols, dtype=np.float64) - cx) / fx, (np.arange(rows, dtype=np.float64) - cy) / fy
        on_axis += bool((depth != 0)[:, xn == 0.0].any() or (depth != 0)[yn == 0.0, :].any())
    print("%d views with a hit on a ray with xn == 0 or yn == 0" % on_axis)
    assert on_axis >= 20
    assert {c["fmt"] for c in cases} == {"u16", "f32"}
    # what the categories are for
    assert sum(np.all(np.isin(c["pose"][:9], (0.0, 1.0, -1.0))) for c in cases if c["category"] == "axis") == 48
    assert {max(abs(o) for o in c["vol"]["origin"]) > 400.0 for c in cases if c["category"] == "far_origin"} == {True, False}
    assert max(abs(o) for c in cases for o in c["vol"]["origin"]) > 9e4
    assert {c["vol"]["voxel_size"] for c in cases if c["category"] == "sizes"} == {0.003, 0.01, 0.05, 0.25}
    assert {d for c in cases if c["category"] == "sizes" for d in c["vol"]["dims"]} == set(range(1, 11))
    assert {c["params"]["step_trunc"] for c in cases} == {1.0, 0.5, 0.25, 0.07}
    long = [c for c in cases if c["category"] == "long_march"]
    assert sorted(c["fmt"] for c in long) == ["f32", "u16"] and all(60000 <= rr.march_samples(c["params"], c["vol"]["trunc"]) <= rr.MAX_STEPS for c in long)
    p = long[0]["params"]
    assert p["z_near"] + p["step_trunc"] * long[0]["vol"]["trunc"] * 63333.0 <= p["z_far"] < p["z_near"] + p["step_trunc"] * long[0]["vol"]["trunc"] * 63334.0


def test_clip_domain_restatement():
    """the numpy restatement equals the host definition on a seeded subset of 40 cases of rr.domain_views.  The restatement marches
    sample by sample in Python: cases whose march has more than 3000 samples -- the two long marches, and the 3 mm voxels at the finest
    step -- take more than a second each and are left out of the draw"""
    cases = rr.domain_views(0)
    rows, cols = rr.DOMAIN_SIZE
    short = [i for i, c in enumerate(cases) if rr.march_samples(c["params"], c["vol"]["trunc"]) <= 3000]
    assert len(short) >= len(cases) - 20
    picked = sorted(np.random.RandomState(40).choice(short, size=40, replace=False))
    assert len({cases[i]["category"] for i in picked}) >= 6
    hits = 0
    for i in picked:
        c = cases[i]
        ref = rr.raycast_view(c["vol"], c["words"], c["K4"], c["pose"], rows, cols, **c["params"])
        depth, nrm = host(c["vol"], c["words"], c["K4"], c["pose"][None], rows, cols, c["fmt"], True, **c["params"])
        assert same_bits(depth[0], ref[c["fmt"]]) and same_bits(nrm[0], ref["normals_" + c["fmt"]]), (i, c["category"])
        hits += int((ref["kind"] == rr.HIT).sum())
    assert hits >= 200


def test_cpp_mirror(tmp_path):
    """include/dvo_amd.hpp's tsdfRaycastHost and TsdfVolumes::raycast: tests/host/tsdf_raycast_hpp_main.cpp compiles with plain g++ and
    every warning on and links against the library; the host function gives the library's bytes on every volume, and on three cases
    TsdfVolumes is asked too: the same bytes where there is a device, a loud refusal where there is none"""
    import torch
    from rgbd_odometry_amd import capi
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "tsdf_raycast_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tsdf_raycast_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    DEVICE_CASES = {("volume1", "u16"), ("random1", "f32"), ("volume2", "u16")}
    rows, cols = rr.SIZES[1]
    K = rr.k4_for(rows, cols)
    for fmt in FORMATS:
        code = capi.DVO_DEPTH_U16 if fmt == "u16" else capi.DVO_DEPTH_F32
        for name, vol, words in volumes():
            poses = np.stack([p for _, p in rr.view_list(vol)])
            p = write_case(tmp_path, vol, words, K, poses)
            on_device = (name, fmt) in DEVICE_CASES                   # every process that asks for the device initialises it: a few are enough
            run = subprocess.run([exe, p["volume"], p["words"], p["views"], str(code), str(rows), str(cols), str(len(poses))] +
                                 (["device"] if on_device else []), capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            depth, nrm, rest = parse_output(run.stdout, len(poses), rows, cols, fmt)
            want = host(vol, words, K, poses, rows, cols, fmt, True)
            assert same_bits(depth, want[0]) and same_bits(nrm, want[1]), (name, fmt)
            if not on_device:
                assert rest == []
            elif torch.cuda.is_available():
                assert rest[0] == "device equal 1", (name, fmt, rest)
            else:
                assert rest[0].startswith("device none") and "no CPU fallback" in rest[0]
    bad = write_case(tmp_path, dict(tr.VOLUMES[2], trunc=-1.0), volumes()[2][2], K, tr.pose12()[None])
    run = subprocess.run([exe, bad["volume"], bad["words"], bad["views"], "1", str(rows), str(cols), "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 3 and run.stdout.strip() == "refused"
