"""The triangle mesh of fused volumes on the CPU (include/dvo_amd.h, "the surface as a triangle mesh"): dvo_mesh_host against the numpy
restatement of the definition (tests/tsdf_mesh_reference.py) on every case, the axis vertices against dvo_tsdf_extract_host, capacities
with guard values, the topology of every mesh from its indices alone, conditions that keep the cases from being vacuous, every refusal,
the symbols and the launch constant, the definition's own code (rgbd_odometry_amd/csrc/dvo_tsdf_mesh.h) as a stand-alone program under
the address and undefined-behaviour sanitizers (tests/host/tsdf_mesh_main.cpp), the C++ mirror (tests/host/tsdf_mesh_hpp_main.cpp) and
the PLY writer.  No GPU.  Comparisons are byte equality unless a bound is stated."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_map_reference as tr
import tsdf_mesh_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, mw) for name in mr.CASE_NAMES for mw in mr.MIN_WEIGHTS[name]]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_host = {}


def host(name, min_weight):
    """dvo_mesh_host on a case through the binding's two-call pattern; computed once"""
    from rgbd_odometry_amd import capi
    if (name, min_weight) not in _host:
        vol, words = mr.case(name)
        v, t = capi.tsdf_mesh_host(c_volume(vol), words, min_weight)
        v.setflags(write=False)
        t.setflags(write=False)
        _host[(name, min_weight)] = (v, t)
    return _host[(name, min_weight)]


def raw_call(lib, vol, words, min_weight, vcap, tcap, guard=3):
    """dvo_mesh_host into buffers of vcap and tcap entries followed by `guard` entries of guard values: (rc, xyz, tri, nv, nt)"""
    from rgbd_odometry_amd import capi
    xyz = np.full((vcap + guard, 3), -7.5, np.float32)
    tri = np.full((tcap + guard, 3), -77, np.int32)
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)
    rc = lib.dvo_mesh_host(C.byref(c_volume(vol)), capi._ptr(words), min_weight, capi._ptr(xyz) if vcap else None, vcap,
                           capi._ptr(tri) if tcap else None, tcap, C.byref(nv), C.byref(nt))
    return rc, xyz, tri, nv.value, nt.value


def test_the_fused_cases_are_the_host_definitions():
    """the reference fuses its volumes with the numpy restatement of the fusion: the same words as the host definition's"""
    from rgbd_odometry_amd import capi
    imgs, poses = tr.frame_list("u16")
    for vi, vol in enumerate(tr.VOLUMES):
        idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
        w = capi.tsdf_integrate_host(c_volume(vol), None, [imgs[i] for i in idx], tr.K4, poses[idx])
        assert same_bits(w, mr.case("volume%d" % vi)[1])


@pytest.mark.parametrize("name,min_weight", CASES)
def test_host_equals_the_restatement(name, min_weight):
    v, t = host(name, min_weight)
    rv, rt = mr.reference(name, min_weight)[:2]
    print("%s at min_weight %d: %d vertices, %d triangles" % (name, min_weight, len(v), len(t)))
    assert len(v) == len(rv) and len(t) == len(rt)
    assert same_bits(v, rv), int((v.view(np.uint32) != rv.view(np.uint32)).any(axis=1).sum())
    assert same_bits(t, rt), int((t != rt).any(axis=1).sum())


@pytest.mark.parametrize("name,min_weight", CASES)
def test_axis_vertices_are_the_surface_points(name, min_weight):
    from rgbd_odometry_amd import capi
    vol, words = mr.case(name)
    v, _ = host(name, min_weight)
    d = mr.reference(name, min_weight)[2]
    pts, n = capi.tsdf_extract_host(c_volume(vol), words, min_weight)
    assert n == int((d < 3).sum())
    assert same_bits(v[d < 3], pts)


@pytest.mark.parametrize("name,min_weight", [("volume0", 1), ("random1", 2), ("volume2", 1), ("SPHERE", 1)])
def test_capacities(name, min_weight):
    """zero, exact, one short and short on one side only: the written prefix is the full result's, nothing beyond it is touched, the
    counts are always the full counts"""
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol, words = mr.case(name)
    v, t = host(name, min_weight)
    nv, nt = len(v), len(t)
    caps = [(0, 0), (nv, nt), (max(nv - 1, 0), max(nt - 1, 0)), (max(nv - 1, 0), nt), (nv, max(nt - 1, 0)), (nv // 2, nt), (nv, nt // 3), (0, nt), (nv, 0),
            (nv + 2, nt + 2)]
    for vcap, tcap in caps:
        rc, xyz, tri, gv, gt = raw_call(lib, vol, words, min_weight, vcap, tcap)
        assert rc == capi.DVO_OK and (gv, gt) == (nv, nt), (vcap, tcap)
        kv, kt = min(vcap, nv), min(tcap, nt)
        assert same_bits(xyz[:kv], v[:kv]) and same_bits(tri[:kt], t[:kt]), (vcap, tcap)
        assert np.all(xyz[kv:] == -7.5) and np.all(tri[kt:] == -77), (vcap, tcap)


@pytest.mark.parametrize("name", ["SPHERE", "TORUS"])
def test_closed_surfaces(name):
    """a closed surface wholly inside valid cells: every directed edge exactly once and its reverse exactly once, V - E + T = 2 (sphere)
    or 0 (torus), no unreferenced vertex, no zero-area triangle, and every triangle normal on the analytic outward side"""
    vol, words = mr.case(name)
    assert not (tr.word_q(words) == 0).any(), "the centre is off the lattice: no voxel lies exactly on the surface"
    assert np.all(tr.word_w(words) == 1)
    v, t = host(name, 1)
    topo = mr.topology(len(v), t)
    print("%s: %d vertices, %d triangles, %s" % (name, len(v), len(t), topo))
    assert len(t) > 10000
    assert topo["max_multiplicity"] == 1 and topo["closed"]
    assert topo["euler"] == (2 if name == "SPHERE" else 0)
    assert topo["unreferenced"] == 0
    P = v.astype(np.float64)[t.astype(np.int64)]
    normal = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert mr.zero_area(v, t) == 0
    dots = np.einsum("ij,ij->i", normal, mr.outward(name, P.mean(axis=1)))
    assert np.all(dots > 0.0), int((dots <= 0.0).sum())


@pytest.mark.parametrize("name,min_weight", CASES)
def test_topology_of_every_case(name, min_weight):
    """no directed edge occurs twice and every index is below n_vertices; with every weight >= min_weight and every dimension >= 2 no
    vertex is unreferenced"""
    vol, words = mr.case(name)
    v, t = host(name, min_weight)
    assert t.dtype == np.int32 and (len(t) == 0 or (t.min() >= 0 and t.max() < len(v)))
    topo = mr.topology(len(v), t)
    assert topo["max_multiplicity"] <= 1
    assert len(t) == 0 or np.all((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2]))
    if np.all(tr.word_w(words) >= min_weight) and min(vol["dims"]) >= 2:
        assert topo["unreferenced"] == 0


def test_full_weights_leave_no_unreferenced_vertex():
    """volume 1's geometry and volume (5, 3, 2) with random q, 30 % of them 0, and every weight 2: every vertex is in some triangle"""
    from rgbd_odometry_amd import capi
    for vol in (tr.VOLUMES[1], tr.VOLUMES[2]):
        words = tr.make_words(tr.word_q(mr.random_words(vol, seed=9)), np.full(tr.voxels_of(vol), 2))
        for mw in (1, 2):
            v, t = capi.tsdf_mesh_host(c_volume(vol), words, mw)
            topo = mr.topology(len(v), t)
            assert len(v) > 0 and topo["unreferenced"] == 0 and topo["max_multiplicity"] == 1, (vol["dims"], mw, topo)
        v, t = capi.tsdf_mesh_host(c_volume(vol), words, 3)
        assert len(v) == 0 and len(t) == 0


def test_cases_are_not_vacuous():
    """the counts a numpy prototype of the definition gave when the feature was specified; the host definition reproduces them"""
    want = {("volume1", 1): dict(vertices=8688, axis=2356, triangles=15622, unreferenced=341, zero_area=2980),
            ("volume1", 2): dict(vertices=2753, triangles=4224, unreferenced=292),
            ("volume0", 1): dict(vertices=1333, triangles=2420, unreferenced=28),
            ("volume0", 2): dict(vertices=970, triangles=1504, unreferenced=90),
            ("volume2", 1): dict(vertices=29, triangles=0),
            ("volume3", 1): dict(vertices=0, triangles=0)}
    for (name, mw), w in want.items():
        v, t = host(name, mw)
        d = mr.reference(name, mw)[2]
        got = dict(vertices=len(v), axis=int((d < 3).sum()), triangles=len(t), unreferenced=mr.topology(len(v), t)["unreferenced"],
                   zero_area=mr.zero_area(v, t))
        print("%s at min_weight %d: %s" % (name, mw, got))
        for key, value in w.items():
            assert got[key] == value, (name, mw, key, got[key], value)
    v, t = host("volume1", 1)
    assert mr.topology(len(v), t)["unreferenced"] < 0.10 * len(v)
    # the random words: many vertices on every direction, many zero-area triangles, and min_weight matters
    v1, t1 = host("random1", 1)
    v2, t2 = host("random1", 2)
    d = mr.reference("random1", 1)[2]
    print("random words: %d / %d vertices, %d / %d triangles, per direction %s" % (len(v1), len(v2), len(t1), len(t2), np.bincount(d, minlength=7)))
    assert np.all(np.bincount(d, minlength=7) >= 1000) and len(t2) >= 1000 and len(t1) > len(t2) and mr.zero_area(v1, t1) >= 100


def test_refusals_of_the_host_definition():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol, words = mr.case("volume0")
    xyz = np.full((8, 3), 7.0, np.float32)
    tri = np.full((8, 3), -9, np.int32)
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)

    def call(null=(), min_weight=1, vcap=8, tcap=8, vol_edit=None):
        v = c_volume(vol)
        if vol_edit:
            vol_edit(v)
        return lib.dvo_mesh_host(None if "vol" in null else C.byref(v), None if "voxels" in null else capi._ptr(words), min_weight,
                                 None if "xyz" in null else capi._ptr(xyz), vcap, None if "tri" in null else capi._ptr(tri), tcap,
                                 None if "nv" in null else C.byref(nv), None if "nt" in null else C.byref(nt))

    def setter(field, value, index=None):
        def edit(o):
            if index is None:
                setattr(o, field, value)
            else:
                getattr(o, field)[index] = value
        return edit

    nan, inf = float("nan"), float("inf")
    bad = [dict(null=(k,)) for k in ("vol", "voxels", "xyz", "tri", "nv", "nt")]
    bad += [dict(min_weight=0), dict(min_weight=-3), dict(vcap=-1), dict(tcap=-1), dict(vcap=-1, tcap=0), dict(null=("xyz", "tri"), vcap=0)]
    for field in ("nx", "ny", "nz"):
        bad += [dict(vol_edit=setter(field, 0)), dict(vol_edit=setter(field, -1)), dict(vol_edit=setter(field, capi.DVO_TSDF_MAX_DIM + 1))]
    for field in ("voxel_size", "trunc"):
        bad += [dict(vol_edit=setter(field, value)) for value in (0.0, -0.1, nan, inf)]
    bad += [dict(vol_edit=setter("origin", value, k)) for k in range(3) for value in (nan, inf, -inf)]
    for kw in bad:
        assert call(**kw) == capi.DVO_ERR_INVALID, kw
        assert (nv.value, nt.value) == (-5, -6) and np.all(xyz == 7.0) and np.all(tri == -9), kw
    # either buffer may be NULL with capacity 0
    assert call(null=("xyz", "tri"), vcap=0, tcap=0) == capi.DVO_OK and (nv.value, nt.value) == (1333, 2420)
    assert call(null=("xyz",), vcap=0) == capi.DVO_OK and np.all(xyz == 7.0) and not np.all(tri == -9)
    tri[:] = -9
    assert call(null=("tri",), tcap=0) == capi.DVO_OK and not np.all(xyz == 7.0) and np.all(tri == -9)
    with pytest.raises(capi.DvoError) as ei:
        capi.tsdf_mesh_host(c_volume(dict(vol, trunc=0.0)), words)
    assert ei.value.code == capi.DVO_ERR_INVALID
    with pytest.raises(ValueError):
        capi.tsdf_mesh_host(c_volume(vol), words[:-1])


def test_handle_calls_without_a_handle():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    nv, nt = C.c_longlong(-5), C.c_longlong(-6)
    assert lib.dvo_mesh_extract(None, 0, 1, None, 0, None, 0, C.byref(nv), C.byref(nt), 0) == capi.DVO_ERR_INVALID
    assert lib.dvo_mesh_extract(None, 0, 1, None, 0, None, 0, None, None, capi.DVO_UPLOAD_DEVICE) == capi.DVO_ERR_INVALID
    assert (nv.value, nt.value) == (-5, -6)


def test_symbols_constants_and_launches():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    names = ["dvo_mesh_host", "dvo_mesh_extract"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    assert sorted(n for n in capi.C_ABI_SYMBOLS if n.startswith("dvo_mesh_")) == sorted(names)
    launch = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_launch.h")).read()
    assert int(re.search(r"#define\s+DVO_MESH_LAUNCHES\s+(\d+)", text).group(1)) == capi.DVO_MESH_LAUNCHES
    assert int(re.search(r"constexpr int kMeshLaunches = (\d+);", launch).group(1)) == capi.DVO_MESH_LAUNCHES
    hip = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_mesh.hip")).read()
    body = hip.split("int launch_tsdf_mesh(")[1].split("\n}\n")[0]
    assert body.count("hipLaunchKernelGGL(") == capi.DVO_MESH_LAUNCHES
    # no atomics and no environment switch in the kernels' file, the tile walk they share with the point extraction, or the definition
    own = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_mesh.h")).read()
    walk = open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "dvo_tsdf_walk.h")).read()
    assert '#include "dvo_tsdf_walk.h"' in hip and "__device__" in walk
    for src in (hip, own, walk):
        code = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        assert "atomic" not in code and "getenv" not in code
    # meshes are no longer out of the fusion section's scope
    full = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    fusion = full.split("---- depth fusion:")[1].split("#ifndef DVO_TSDF_TYPES_DEFINED_")[0]
    assert "OUT OF SCOPE" in fusion and "meshes" not in fusion.split("OUT OF SCOPE")[1]


# ---- the definition's own code under sanitizers, and the C++ mirror ----

def fnv1a(*blocks):
    """the 64-bit FNV-1a of the blocks' bytes, as the programs compute it"""
    h = 0xCBF29CE484222325
    data = np.frombuffer(b"".join(np.ascontiguousarray(b).tobytes() for b in blocks), np.uint8)
    for byte in data.tolist():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


_checksums = {}


def host_checksum(name, min_weight):
    """fnv1a of the library's mesh of a case; computed once (the loop walks every byte)"""
    if (name, min_weight) not in _checksums:
        _checksums[(name, min_weight)] = fnv1a(*host(name, min_weight))
    return _checksums[(name, min_weight)]


def write_case(d, vol, words):
    paths = {k: str(d / (k + ".bin")) for k in ("volume", "words")}
    open(paths["volume"], "wb").write(bytes(c_volume(vol)))
    np.asarray(words, np.uint32).tofile(paths["words"])
    return paths


def parse(stdout):
    lines = stdout.splitlines()
    out = dict(line.split(" ", 1) for line in lines if line.split(" ", 1)[0] in ("vertices", "triangles", "checksum", "device", "table"))
    return out


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_mesh")
    exe = str(d / "tsdf_mesh_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tsdf_mesh_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/tsdf_mesh_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


# the checksum in Python walks every byte: the small cases, and the sphere through its counts and the library's own checksum path below
SANITIZER_CASES = [("volume0", 1), ("volume0", 2), ("volume1", 1), ("volume1", 2), ("volume2", 1), ("volume3", 1), ("random1", 1), ("random1", 2)]


@pytest.mark.parametrize("name,min_weight", SANITIZER_CASES)
def test_definition_under_sanitizers(host_program, name, min_weight):
    """the same code the library compiles, with every buffer allocated to its exact size: clean under -fsanitize=address,undefined, the
    generated table agrees with the geometry, and the mesh has the library's bytes"""
    d, exe = host_program
    vol, words = mr.case(name)
    p = write_case(d, vol, words)
    run = subprocess.run([exe, p["volume"], p["words"], str(min_weight)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = parse(run.stdout)
    v, t = host(name, min_weight)
    assert got["table"] == "ok"
    assert (int(got["vertices"]), int(got["triangles"])) == (len(v), len(t))
    assert int(got["checksum"], 16) == host_checksum(name, min_weight)


def test_program_refuses_what_the_definition_refuses(host_program):
    d, exe = host_program
    vol, words = mr.case("volume0")
    for bad_vol, mw in ((dict(vol, trunc=0.0), 1), (dict(vol, voxel_size=float("nan")), 1), (dict(vol, origin=(0.0, float("inf"), 0.0)), 1), (vol, 0), (vol, -2)):
        p = write_case(d, bad_vol, words)
        run = subprocess.run([exe, p["volume"], p["words"], str(mw)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 3 and run.stdout.splitlines()[-1] == "refused", run.stdout + run.stderr


def test_cpp_mirror(tmp_path):
    """include/dvo_amd.hpp's tsdfMeshHost and TsdfVolumes::mesh: tests/host/tsdf_mesh_hpp_main.cpp compiles with plain g++ and every
    warning on and links against the library; the host function gives the library's bytes on every small case, and on three cases
    TsdfVolumes is asked too: the same bytes where there is a device, a loud refusal where there is none"""
    import torch
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "tsdf_mesh_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "tsdf_mesh_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    DEVICE_CASES = {("volume1", 1), ("random1", 2), ("volume2", 1)}
    for name, mw in SANITIZER_CASES:
        vol, words = mr.case(name)
        p = write_case(tmp_path, vol, words)
        on_device = (name, mw) in DEVICE_CASES                        # every process that asks for the device initialises it: a few are enough
        run = subprocess.run([exe, p["volume"], p["words"], str(mw)] + (["device"] if on_device else []), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        got = parse(run.stdout)
        v, t = host(name, mw)
        assert (int(got["vertices"]), int(got["triangles"])) == (len(v), len(t)) and int(got["checksum"], 16) == host_checksum(name, mw), (name, mw)
        if not on_device:
            assert "device" not in got
        elif torch.cuda.is_available():
            assert got["device"] == "equal 1", (name, mw, got)
        else:
            assert got["device"].startswith("none") and "no CPU fallback" in got["device"]
    bad = write_case(tmp_path, dict(tr.VOLUMES[2], trunc=-1.0), mr.case("volume2")[1])
    run = subprocess.run([exe, bad["volume"], bad["words"], "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 3 and run.stdout.strip() == "refused"


def test_save_ply(tmp_path):
    """the header text, and the two binary blocks read back"""
    from rgbd_odometry_amd import capi
    v, t = host("volume0", 1)
    path = str(tmp_path / "mesh.ply")
    capi.save_ply(path, v, t)
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0" and header[-1] == "end_header"
    rest = [line for line in header[2:-1] if not line.startswith("comment")]
    assert rest == ["element vertex %d" % len(v), "property float x", "property float y", "property float z", "element face %d" % len(t),
                    "property list uchar int vertex_indices"]
    assert len(raw) == end + 12 * len(v) + 13 * len(t)
    assert same_bits(np.frombuffer(raw, "<f4", 3 * len(v), end).reshape(-1, 3), v)
    faces = np.frombuffer(raw, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), len(t), end + 12 * len(v))
    assert np.all(faces["n"] == 3) and same_bits(np.ascontiguousarray(faces["i"]), t)
    # an empty mesh is a header with two zero counts
    capi.save_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    raw = open(path, "rb").read()
    assert raw.endswith(b"end_header\n") and b"element vertex 0\n" in raw and b"element face 0\n" in raw
