"""Distance fields on the CPU (include/dvo_amd.h, "distance fields"): the host definition (rgbd_odometry_amd/csrc/dvo_esdf.h) against
the two numpy forms of tests/esdf_reference.py on fused, random and constructed volumes, what the numbers mean on an analytic sphere, the
point query bit for bit, three deliberately wrong stand-ins and the assertion each one fails, every refusal, the symbols and struct
sizes, and the definition's own code as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/host/esdf_main.cpp) and the C++ mirror (tests/host/esdf_hpp_main.cpp).  No GPU.  Comparisons are byte equality unless a bound is
stated."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import esdf_reference as er
import tsdf_map_reference as tr
import tsdf_mesh_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_esdf_params_default", "dvo_esdf_host", "dvo_esdf_distances_host", "dvo_esdf_query_host", "dvo_esdf_enable", "dvo_esdf_update",
               "dvo_esdf_get_words", "dvo_esdf_get_distances", "dvo_esdf_query"]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def host(vol, tw, mw=1, sites=0):
    from rgbd_odometry_amd import capi
    return capi.esdf_host(c_volume(vol), tw, capi.DvoEsdfParams.default(min_weight=mw, sites=sites))


# ---- 1: the host definition, the full and the separable brute force ----

def test_fused_and_random_volumes_equal_both_brute_forces():
    cases = er.fused_cases()
    assert [n for n, _, _ in cases] == ["volume0", "volume1", "volume2", "volume3", "edge", "random0", "random23"]
    er.check_words(host, cases)
    # the cases are not vacuous: sites, inside voxels and unknown voxels in the fused volumes; both modes differ
    for name in ("volume0", "volume1"):
        vol, tw = mr.case(name)
        a, b = host(vol, tw, 1, 0), host(vol, tw, 1, 1)
        assert (a & er.NO_SITE).min() == 0 and (a & er.INSIDE).any() and (a & er.UNKNOWN).any() and not np.array_equal(a, b), name
        assert ((a & er.NO_SITE) >= (b & er.NO_SITE)).all() and ((a & er.NO_SITE) > 9).any()


# ---- 2: constructed volumes ----

def test_constructed_volumes():
    from rgbd_odometry_amd import capi
    cases = er.constructed_cases()
    er.check_words(host, cases)
    by = {n: (v, w) for n, v, w in cases}
    # no site at all: every d2 is NO_SITE, the distances +-infinity by the inside bit
    for name, inf in (("no_site_outside", np.inf), ("no_site_inside", -np.inf)):
        vol, tw = by[name]
        w = host(vol, tw)
        assert np.all((w & er.NO_SITE) == er.NO_SITE) and np.all((w & er.INSIDE != 0) == (inf < 0)) and not (w & er.UNKNOWN).any()
        m = capi.esdf_distances_host(c_volume(vol), w)
        assert np.all(m == np.float32(inf)) and np.array_equal(m, er.metres(vol, w))
    # every voxel a site
    vol, tw = by["all_sites"]
    assert np.all((host(vol, tw) & er.NO_SITE) == 0)
    # one site in the corner of 70 x 67 x 65: the far corner
    vol, tw = by["corner"]
    w = host(vol, tw, 1, 1).reshape(65, 67, 70)
    assert int(w[64, 66, 69]) == 69 ** 2 + 66 ** 2 + 64 ** 2 and int(w[0, 0, 0]) == er.UNKNOWN
    assert np.all((host(vol, tw, 1, 0) & er.NO_SITE) == er.NO_SITE)
    # two sites at equal distance: the middle voxel of the row between them
    vol, tw = by["two_equal"]
    w = host(vol, tw).reshape(3, 3, 21) & er.NO_SITE
    assert int(w[1, 1, 10]) == 9 * 9 and int(w[1, 1, 1]) == 0 == int(w[1, 1, 19]) and np.array_equal(w[1, 1], w[1, 1, ::-1])
    # 1 x 1 x 1
    vol, tw = by["one_voxel"]
    assert int(host(vol, tw)[0]) == er.NO_SITE and int(host(vol, tw, 2, 1)[0]) == er.UNKNOWN and int(host(vol, tw, 2, 0)[0]) == (er.UNKNOWN | er.NO_SITE)
    # lines along y and z: |i - the nearest of the three sites| squared
    for name, at in (("line_y", 5), ("line_z", 33)):
        vol, tw = by[name]
        n = max(vol["dims"])
        want = np.maximum(np.abs(np.arange(n) - at) - 1, 0) ** 2
        assert np.array_equal(host(vol, tw) & er.NO_SITE, want), name
    # the largest dimension on every axis
    for name, far in (("long_x", 1022), ("long_y", 1022), ("long_z", 522)):
        vol, tw = by[name]
        assert max(vol["dims"]) == 1024 and int((host(vol, tw) & er.NO_SITE).max()) >= far ** 2, name


# ---- 3: what the numbers mean ----

_sphere = {}


def sphere():
    """(volume, ESDF words by the separable brute force, |p - c| per voxel); computed once"""
    if not _sphere:
        vol, tw = mr.case("SPHERE")
        x, y, z = mr._analytic_grid()
        _sphere["all"] = (vol, tw, er.reference("SPHERE", vol, tw, 1, 0), np.sqrt(x * x + y * y + z * z).reshape(-1))
    return _sphere["all"]


def check_sphere_meaning(vol, words, rho):
    """T = | |p - c| - r | is the true distance to the sphere; every voxel's D must satisfy T - voxel_size <= |D| <= T + 2 sqrt(3)
    voxel_size.  Lower: |D| is the distance to a site's centre, and a site has a neighbour of the other sign one voxel_size away, so the
    surface crosses that edge and the site lies within one voxel_size of it.  Upper: within one cell diagonal (sqrt(3) voxel_size) of the
    nearest surface point of a sphere this large some lattice edge crosses the surface, and its two ends are sites; the second diagonal
    is slack for the quantised words.  The sign is negative exactly where |p - c| < r for voxels further than one voxel from the surface"""
    vs = vol["voxel_size"]
    D = er.signed(words, vs)
    T = np.abs(rho - mr.SPHERE_RADIUS)
    assert not ((words & er.NO_SITE) == er.NO_SITE).any()
    lower, upper = (np.abs(D) - (T - vs)).min(), (T + 2.0 * np.sqrt(3.0) * vs - np.abs(D)).min()
    print("sphere: min(|D| - (T - vs)) = %.6f, min(T + 2 sqrt(3) vs - |D|) = %.6f, max | |D| - T | = %.6f" % (lower, upper, np.abs(np.abs(D) - T).max()))
    assert lower >= 0.0, "a voxel's distance is more than one voxel_size below the true distance"
    assert upper >= 0.0, "a voxel's distance is more than two cell diagonals above the true distance"
    far = T > vs
    assert np.array_equal((D < 0)[far], (rho < mr.SPHERE_RADIUS)[far]), "the sign is wrong further than one voxel from the surface"
    assert far.sum() > 0.8 * far.size and (D < 0)[far].any() and (D > 0)[far].any()


def test_sphere_reference_alone_meets_the_bound():
    vol, tw, ref, rho = sphere()
    check_sphere_meaning(vol, ref, rho)


def test_sphere_host_definition():
    from rgbd_odometry_amd import capi
    vol, tw, ref, rho = sphere()
    w = host(vol, tw)
    assert np.array_equal(w, ref)
    check_sphere_meaning(vol, w, rho)
    m = capi.esdf_distances_host(c_volume(vol), w)
    assert m.dtype == np.float32 and m.tobytes() == er.metres(vol, w).tobytes()


# ---- 4: the point query ----

def query_cases():
    """[(name, volume, ESDF words)]: fused volumes with unknown corners, the sphere, a volume without a site"""
    out = []
    for name in ("volume0", "volume2"):
        vol, tw = mr.case(name)
        out.append((name, vol, er.reference(name, vol, tw, 1, 0)))
    vol, tw, ref, _ = sphere()
    out.append(("SPHERE", vol, ref))
    name, vol, tw = er.constructed_cases()[0]
    out.append((name, vol, er.reference(name, vol, tw, 1, 0)))
    return out


def test_query_equals_the_restatement_bit_for_bit():
    from rgbd_odometry_amd import capi
    seen, unknown_seen = set(), False
    for name, vol, words in query_cases():
        P = er.query_points(vol, words)
        got, want = capi.esdf_query_host(c_volume(vol), words, P), er.query(vol, words, P)
        assert got.dtype == er.SAMPLE_DTYPE and got.tobytes() == want.tobytes(), (name, int((got != want).sum()))
        seen |= set(int(s) for s in got["status"])
        unknown_seen |= bool(((got["status"] == er.FOUND) & (got["unknown"] > 0)).any())
        # the points by kind: outside by one ulp on either side, the last lattice point, the first
        nx, ny, nz = vol["dims"]
        o, vs = np.array(vol["origin"]), vol["voxel_size"]
        hi = o + vs * (np.array([nx, ny, nz], np.float64) - 1.0)
        mid = o + vs * (np.array([nx, ny, nz], np.float64) - 1.0) / 2.0
        for k, n in enumerate((nx, ny, nz)):
            # the first double whose g reaches n - 1 (g is monotone in P; o + vs (n - 1) itself may round to either side): it is outside,
            # the double below it is not; one ulp below the origin is outside too
            edge = hi[k]
            while (edge - o[k]) / vs < n - 1:
                edge = np.nextafter(edge, np.inf)
            while (np.nextafter(edge, -np.inf) - o[k]) / vs >= n - 1:
                edge = np.nextafter(edge, -np.inf)
            below, at_edge, inside = mid.copy(), mid.copy(), mid.copy()
            below[k], at_edge[k], inside[k] = np.nextafter(o[k], -np.inf), edge, np.nextafter(edge, -np.inf)
            rec = capi.esdf_query_host(c_volume(vol), words, np.stack([below, at_edge, inside]))
            assert list(rec["status"][:2]) == [er.OUTSIDE, er.OUTSIDE] and rec["status"][2] != er.OUTSIDE, (name, k, rec["status"])
            assert not rec["distance"][:2].any() and not rec["gradient"][:2].any() and not rec["unknown"][:2].any(), (name, k)
    assert seen == {er.FOUND, er.OUTSIDE, er.NO_DISTANCE} and unknown_seen
    # a point on the lattice reads its voxel's value exactly
    vol, tw, ref, _ = sphere()
    nx, ny, nz = vol["dims"]
    o, vs = np.array(vol["origin"]), vol["voxel_size"]
    idx = np.array([[3, 4, 5], [40, 40, 40], [0, 0, 0], [nx - 2, ny - 2, nz - 2]])
    rec = capi.esdf_query_host(c_volume(vol), ref, o + vs * idx)
    on = np.flatnonzero((np.floor((vs * idx) / vs) == idx).all(axis=1))          # where (o + vs i - o) / vs is i again
    assert len(on) >= 1
    assert np.array_equal(rec["distance"][on], er.signed(ref, vs).reshape(nz, ny, nx)[idx[on, 2], idx[on, 1], idx[on, 0]])


def test_query_gradient_points_away_from_the_sphere():
    """points 5 to 10 voxels outside: the cosine between the gradient and the outward direction, measured on the restatement; the host
    records are asserted against the restatement's bytes, not against a threshold"""
    from rgbd_odometry_amd import capi
    vol, tw, ref, _ = sphere()
    rng = np.random.RandomState(77)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P = np.array(mr.ANALYTIC_CENTRE) + d * (mr.SPHERE_RADIUS + vol["voxel_size"] * rng.uniform(5.0, 10.0, size=(400, 1)))
    want = er.query(vol, ref, P)
    inside = want["status"] == er.FOUND                               # ten voxels out reaches the rim of the lattice: those points are OUTSIDE
    assert inside.sum() >= 300 and set(want["status"]) <= {er.FOUND, er.OUTSIDE}
    g, d = want["gradient"][inside], d[inside]
    cos = (g * d).sum(axis=1) / np.linalg.norm(g, axis=1)
    print("gradient of the restatement 5 to 10 voxels outside the sphere: cosine min %.4f mean %.4f; |gradient| %.3f .. %.3f"
          % (cos.min(), cos.mean(), np.linalg.norm(g, axis=1).min(), np.linalg.norm(g, axis=1).max()))
    assert np.all(cos > 0.0), "the restatement's gradient points towards the sphere"
    assert capi.esdf_query_host(c_volume(vol), ref, P).tobytes() == want.tobytes()


# ---- 5: three wrong stand-ins, and the assertion each one fails ----

def stand_in(fault):
    def run(vol, tw, mw, sites):
        if fault == "city_block":
            return er.words(vol, tw, mw, sites, form="full", metric="city")
        if fault == "radius_8":
            return er.words(vol, tw, mw, sites, radius=8)
        if fault == "forward_neighbours":
            return er.words(vol, tw, mw, sites, neighbours=((0, 1), (1, 1), (2, 1)))
        return er.words(vol, tw, mw, sites)
    return run


def small_cases():
    return [c for c in er.fused_cases() if c[0] in ("volume0", "random23")] + [c for c in er.constructed_cases() if c[0] in ("two_equal", "line_z")]


def test_the_check_passes_a_correct_stand_in():
    er.check_words(stand_in(None), small_cases())


@pytest.mark.parametrize("fault,assertion", [("city_block", r"d2 of volume0 differs from the separable brute force"),
                                             ("radius_8", r"d2 of (volume0|two_equal|line_z) differs from the separable brute force"),
                                             ("forward_neighbours", r"d2 of volume0 differs from the separable brute force")])
def test_the_check_sees_a_wrong_stand_in(fault, assertion):
    """a city-block distance in place of the Euclidean one, a scan that stops at a fixed radius of 8, a site test that looks only at the
    +x, +y, +z neighbours"""
    with pytest.raises(AssertionError, match="^" + assertion):
        er.check_words(stand_in(fault), small_cases())


# ---- 6: refusals, symbols, sizes ----

def test_refusals_write_nothing():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    vol, tw = mr.case("volume2")
    n = tr.voxels_of(vol)
    cv = c_volume(vol)
    tw = np.ascontiguousarray(tw)
    ew = host(vol, tw)
    p = capi.DvoEsdfParams.default()
    assert (p.min_weight, p.sites) == (1, 0) and lib.dvo_esdf_params_default(None) == capi.DVO_ERR_INVALID
    out = np.full(n, 0xA5A5A5A5, np.uint32)
    fout = np.full(n, -7.5, np.float32)
    P = er.query_points(vol, ew)[:8].copy()
    rec = np.full(8, 9, er.SAMPLE_DTYPE)
    keep = rec.tobytes()
    ptr = lambda a: a.ctypes.data
    bad_volumes = [dict(vol, dims=(0, 3, 2)), dict(vol, dims=(5, 1025, 2)), dict(vol, voxel_size=0.0), dict(vol, voxel_size=float("nan")),
                   dict(vol, trunc=-1.0), dict(vol, origin=(0.0, float("inf"), 0.0))]
    for bv in bad_volumes:
        bc = c_volume(bv)
        assert lib.dvo_esdf_host(C.byref(bc), ptr(tw), C.byref(p), ptr(out)) == capi.DVO_ERR_INVALID
        assert lib.dvo_esdf_distances_host(C.byref(bc), ptr(ew), ptr(fout)) == capi.DVO_ERR_INVALID
        assert lib.dvo_esdf_query_host(C.byref(bc), ptr(ew), 8, ptr(P), ptr(rec)) == capi.DVO_ERR_INVALID
    for mw, sites in ((0, 0), (-1, 1), (1, 2), (1, -1)):
        q = capi.DvoEsdfParams.default(min_weight=mw, sites=sites)
        assert lib.dvo_esdf_host(C.byref(cv), ptr(tw), C.byref(q), ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_host(None, ptr(tw), C.byref(p), ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_host(C.byref(cv), None, C.byref(p), ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_host(C.byref(cv), ptr(tw), None, ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_host(C.byref(cv), ptr(tw), C.byref(p), None) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_distances_host(None, ptr(ew), ptr(fout)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_distances_host(C.byref(cv), None, ptr(fout)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_distances_host(C.byref(cv), ptr(ew), None) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_query_host(None, ptr(ew), 8, ptr(P), ptr(rec)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_query_host(C.byref(cv), None, 8, ptr(P), ptr(rec)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_query_host(C.byref(cv), ptr(ew), 0, ptr(P), ptr(rec)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_query_host(C.byref(cv), ptr(ew), 8, None, ptr(rec)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_query_host(C.byref(cv), ptr(ew), 8, ptr(P), None) == capi.DVO_ERR_INVALID
    for value in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[7, 2] = value                                                # the last point: nothing of the first seven is written either
        assert lib.dvo_esdf_query_host(C.byref(cv), ptr(ew), 8, ptr(Q), ptr(rec)) == capi.DVO_ERR_INVALID
    assert np.all(out == 0xA5A5A5A5) and np.all(fout == -7.5) and rec.tobytes() == keep
    with pytest.raises(ValueError):
        capi.esdf_host(cv, tw[:-1])
    # the handle's calls without a handle
    assert lib.dvo_esdf_enable(None) == capi.DVO_ERR_INVALID and lib.dvo_esdf_update(None, C.byref(p), 1, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_get_words(None, 0, ptr(out)) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_get_distances(None, 0, 0, 1, ptr(fout), 0) == capi.DVO_ERR_INVALID
    assert lib.dvo_esdf_query(None, 0, 8, ptr(P), ptr(rec), 0) == capi.DVO_ERR_INVALID
    assert np.all(out == 0xA5A5A5A5) and np.all(fout == -7.5) and rec.tobytes() == keep


def test_symbols_headers_and_launches():
    from rgbd_odometry_amd import capi
    full = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", full, flags=re.S)
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    assert sorted(n for n in capi.C_ABI_SYMBOLS if n.startswith("dvo_esdf_")) == sorted(NEW_SYMBOLS)
    assert sorted(set(re.findall(r"\b(dvo_esdf_[a-z0-9_]+)\s*\(", text))) == sorted(NEW_SYMBOLS)
    csrc = lambda f: open(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", f)).read()
    own, launch, hip = csrc("dvo_esdf.h"), csrc("dvo_esdf_launch.h"), csrc("dvo_esdf.hip")
    assert '#include "dvo_tsdf_map.h"' in own and '#include "dvo_esdf.h"' in launch
    block = lambda src: re.search(r"#ifndef DVO_ESDF_TYPES_DEFINED_(.*?)#endif", src, flags=re.S).group(1).split()
    assert block(full) == block(own)
    assert int(re.search(r"#define\s+DVO_ESDF_UPDATE_LAUNCHES\s+(\d+)", text).group(1)) == capi.DVO_ESDF_UPDATE_LAUNCHES
    assert int(re.search(r"constexpr int kEsdfUpdateLaunches = (\d+);", launch).group(1)) == capi.DVO_ESDF_UPDATE_LAUNCHES
    for fn, want in (("launch_esdf_update", capi.DVO_ESDF_UPDATE_LAUNCHES), ("launch_esdf_distances", 1), ("launch_esdf_query", 1)):
        body = hip.split("int %s(" % fn)[1].split("\n}\n")[0]
        assert body.count("hipLaunchKernelGGL(") == want, fn
    # no atomics, no environment switch, no LDS and no barrier in the definition and its kernels
    for src in (own, hip):
        code = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        assert "atomic" not in code and "getenv" not in code and "__shared__" not in code and "__syncthreads" not in code
    for macro, value in (("DVO_ESDF_SITES_SURFACE", 0), ("DVO_ESDF_SITES_SURFACE_AND_UNKNOWN", 1), ("DVO_ESDF_NO_SITE", er.NO_SITE),
                         ("DVO_ESDF_INSIDE", er.INSIDE), ("DVO_ESDF_UNKNOWN", er.UNKNOWN), ("DVO_ESDF_FOUND", 0), ("DVO_ESDF_OUTSIDE", 1),
                         ("DVO_ESDF_NO_DISTANCE", 2)):
        assert int(re.search(r"#define\s+%s\s+(\w+)" % macro, text).group(1).rstrip("u"), 0) == value == getattr(capi, macro), macro
    section = full.split("---- distance fields:")[1].split("#ifndef DVO_ESDF_TYPES_DEFINED_")[0]
    for word in ("CONTRACT", "OUT OF SCOPE", "incremental", "clamp", "sub-voxel", "cost-map", "hashed"):
        assert word in section, word
    assert full.index("---- colour in the map:") < full.index("---- distance fields:") < full.index("---- frame-to-model alignment:")


def test_struct_sizes_agree_with_a_compiled_program(tmp_path):
    from rgbd_odometry_amd import capi
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu", '
                   'sizeof(dvo_esdf_params), offsetof(dvo_esdf_params, sites), sizeof(dvo_esdf_sample), offsetof(dvo_esdf_sample, unknown), '
                   'offsetof(dvo_esdf_sample, distance), offsetof(dvo_esdf_sample, gradient));return 0;}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = capi.DvoEsdfSample
    assert got == [C.sizeof(capi.DvoEsdfParams), capi.DvoEsdfParams.sites.offset, C.sizeof(S), S.unknown.offset, S.distance.offset, S.gradient.offset]
    assert C.sizeof(S) == capi.ESDF_SAMPLE_DTYPE.itemsize == er.SAMPLE_DTYPE.itemsize == 40
    assert [capi.ESDF_SAMPLE_DTYPE.fields[k][1] for k in ("status", "unknown", "distance", "gradient")] == [0, S.unknown.offset, S.distance.offset, S.gradient.offset]


# ---- 7: the definition's own code under sanitizers, and the C++ mirror ----

def fnv1a(*blocks):
    """the 64-bit FNV-1a of the blocks' bytes, as the programs compute it"""
    h = 0xCBF29CE484222325
    data = np.frombuffer(b"".join(np.ascontiguousarray(b).tobytes() for b in blocks), np.uint8)
    for byte in data.tolist():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


#: (case, min_weight, sites): small volumes, whose bytes the checksum in Python can walk
PROGRAM_CASES = [("volume0", 1, 0), ("volume0", 2, 1), ("volume2", 1, 1), ("volume3", 1, 0), ("random23", 1, 0)]


def program_case(name):
    return next((v, w) for n, v, w in er.fused_cases() if n == name)


def program_args(d, name, mw, sites, vol=None):
    v, tw = program_case(name)
    ew = host(v, tw, mw, sites)
    P = er.query_points(v, ew, n=40)
    paths = {k: str(d / ("%s_%s_%d_%d.bin" % (k, name, mw, sites))) for k in ("volume", "words", "points")}
    open(paths["volume"], "wb").write(bytes(c_volume(vol or v)))
    np.ascontiguousarray(tw).tofile(paths["words"])
    P.tofile(paths["points"])
    return [paths["volume"], paths["words"], str(mw), str(sites), paths["points"], str(len(P))]


def expected(name, mw, sites):
    from rgbd_odometry_amd import capi
    v, tw = program_case(name)
    ew = host(v, tw, mw, sites)
    P = er.query_points(v, ew, n=40)
    return dict(words="%016x" % fnv1a(ew), metres="%016x" % fnv1a(capi.esdf_distances_host(c_volume(v), ew)),
                records="%016x" % fnv1a(capi.esdf_query_host(c_volume(v), ew, P)))


def parse(stdout):
    return dict(line.split(" ", 1) for line in stdout.splitlines() if " " in line)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("esdf")
    exe = str(d / "esdf_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "esdf_main.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/esdf_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


@pytest.mark.parametrize("name,mw,sites", PROGRAM_CASES)
def test_definition_under_sanitizers(host_program, name, mw, sites):
    """the same code the library compiles, with every buffer allocated to its exact size: clean under -fsanitize=address,undefined, and
    words, metres and query records have the library's bytes"""
    d, exe = host_program
    run = subprocess.run([exe] + program_args(d, name, mw, sites), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert parse(run.stdout) == expected(name, mw, sites)


def test_program_refuses_what_the_definition_refuses(host_program):
    d, exe = host_program
    v, _ = program_case("volume2")
    for vol, mw, sites in ((dict(v, trunc=0.0), 1, 0), (dict(v, voxel_size=float("nan")), 1, 0), (None, 0, 0), (None, 1, 2)):
        args = program_args(d, "volume2", 1, 0, vol=vol)
        args[2], args[3] = str(mw), str(sites)
        run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert run.returncode == 3 and run.stdout.splitlines()[-1] == "refused", run.stdout + run.stderr
    # a point that is not finite
    args = program_args(d, "volume2", 1, 0)
    P = np.fromfile(args[4], np.float64)
    P[4] = np.nan
    P.tofile(args[4])
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 3 and run.stdout.splitlines()[-1] == "refused", run.stdout + run.stderr


def test_cpp_mirror(tmp_path):
    """include/dvo_amd.hpp's distance-field functions and the members of TsdfVolumes: tests/host/esdf_hpp_main.cpp compiles with plain
    g++ and every warning on and links against the library; the host functions give the library's bytes on every case, and on two cases
    TsdfVolumes is asked too: the same bytes where there is a device, a loud refusal where there is none"""
    import torch
    lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
    exe = str(tmp_path / "esdf_hpp_main")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "esdf_hpp_main.cpp"), "-L" + lib, "-ldvo_amd", "-Wl,-rpath," + lib,
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    DEVICE_CASES = {("volume0", 2, 1), ("random23", 1, 0)}
    for name, mw, sites in PROGRAM_CASES:
        on_device = (name, mw, sites) in DEVICE_CASES                  # every process that asks for the device initialises it: a few are enough
        run = subprocess.run([exe] + program_args(tmp_path, name, mw, sites) + (["device"] if on_device else []), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        got = parse(run.stdout)
        device = got.pop("device", None)
        assert got == expected(name, mw, sites), (name, mw, sites)
        if on_device and torch.cuda.is_available():
            assert device == "equal 1", (name, mw, sites, device)
        elif on_device:
            assert device.startswith("none") and "no CPU fallback" in device
    v, _ = program_case("volume2")
    bad = program_args(tmp_path, "volume2", 1, 0, vol=dict(v, trunc=-1.0))
    run = subprocess.run([exe] + bad, capture_output=True, text=True, timeout=120)
    assert run.returncode == 3 and run.stdout.splitlines()[-1] == "refused"
