"""Euclidean signed distance fields (include/dvo_amd.h, "distance fields") restated in numpy from the text of
rgbd_odometry_amd/csrc/dvo_esdf.h, in two independent forms -- the full brute force, every voxel against every site, and the separable
brute force, per axis the n x n min-plus table -- plus metres, the point query, and the cases and checks the CPU and GPU tests share.
A volume is a dict(dims=(nx, ny, nz), voxel_size, origin, trunc) as in tsdf_map_reference; its TSDF and ESDF words are nx * ny * nz
uint32 each, voxel (ix, iy, iz) at index ix + nx * (iy + ny * iz)."""
import numpy as np

import tsdf_map_reference as tr
import tsdf_mesh_reference as mr

NO_SITE = 0xFFFFFF
INSIDE, UNKNOWN = 0x40000000, 0x80000000
SURFACE, SURFACE_AND_UNKNOWN = 0, 1
FOUND, OUTSIDE, NO_DISTANCE = 0, 1, 2
SAMPLE_DTYPE = np.dtype([("status", np.int32), ("unknown", np.int32), ("distance", np.float64), ("gradient", np.float64, (3,))])
_BIG = np.int64(1) << np.int64(40)


def classify(vol, tsdf_words, min_weight=1, sites=SURFACE, neighbours=((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))):
    """(flag bits (nz, ny, nx) uint32, site mask (nz, ny, nx) bool).  observed = w >= min_weight; inside = observed and q < 0; a surface
    site is observed with an observed axis neighbour of the other sign; with sites == 1 every voxel that is not observed is a site.
    neighbours: (axis, step) pairs -- all six in the definition"""
    nx, ny, nz = vol["dims"]
    q = tr.word_q(tsdf_words).reshape(nz, ny, nx)
    w = tr.word_w(tsdf_words).reshape(nz, ny, nx)
    observed = w >= min_weight
    neg = q < 0
    site = np.zeros((nz, ny, nx), bool)
    for axis, step in neighbours:
        ax = 2 - axis                                                  # arrays are [z, y, x]
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = (slice(0, -1), slice(1, None)) if step > 0 else (slice(1, None), slice(0, -1))
        a, b = tuple(a), tuple(b)
        site[a] |= observed[a] & observed[b] & (neg[a] != neg[b])
    if sites == SURFACE_AND_UNKNOWN:
        site |= ~observed
    flags = np.where(observed, np.where(neg, np.uint32(INSIDE), np.uint32(0)), np.uint32(UNKNOWN)).astype(np.uint32)
    return flags, site


def d2_full(site, chunk=1 << 22, metric="euclid"):
    """the full brute force: every voxel against every site, in chunks of voxels.  (nz, ny, nx) int64; NO_SITE without a site"""
    nz, ny, nx = site.shape
    s = np.argwhere(site).astype(np.int64)                             # (S, 3) z, y, x
    if len(s) == 0:
        return np.full(site.shape, NO_SITE, np.int64)
    a = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    out = np.empty(len(a), np.int64)
    step = max(1, chunk // len(s))
    if metric == "euclid":
        # |a - s|^2 = |a|^2 + (|s|^2 - 2 a.s): the bracket for every pair is one matrix product of (x, y, z, 1) with (-2 sx, -2 sy, -2 sz,
        # |s|^2).  Every entry and partial sum is an integer below 2^24 in magnitude (a dimension is at most 1024), so float32 is exact
        assert max(nx, ny, nz) <= 1024
        s_aug = np.concatenate([-2.0 * s, (s * s).sum(axis=1, keepdims=True)], axis=1).astype(np.float32).T.copy()
        a_aug = np.concatenate([a, np.ones((len(a), 1), np.int64)], axis=1).astype(np.float32)
        a2 = (a * a).sum(axis=1)
        for i in range(0, len(a), step):
            out[i:i + step] = a2[i:i + step] + (a_aug[i:i + step] @ s_aug).min(axis=1).astype(np.int64)
        return out.reshape(site.shape)
    s32 = s.astype(np.int32)
    for i in range(0, len(a), step):                                   # a wrong stand-in: the city-block distance, squared
        d = a[i:i + step, None, :].astype(np.int32) - s32[None, :, :]
        m = np.abs(d).sum(axis=-1, dtype=np.int32).min(axis=1).astype(np.int64)
        out[i:i + step] = m * m
    return out.reshape(site.shape)


def _min_plus(f, axis, radius=None):
    """out[i] = min_j f[j] + (i - j)^2 along `axis`, by the n x n table; radius: a wrong stand-in that only looks |i - j| <= radius"""
    n = f.shape[axis]
    i = np.arange(n, dtype=np.int64)
    table = (i[:, None] - i[None, :]) ** 2                             # [i, j]
    if radius is not None:
        table = np.where(np.abs(i[:, None] - i[None, :]) <= radius, table, _BIG)
    g = np.ascontiguousarray(np.moveaxis(f, axis, -1))
    out = np.empty(g.shape, np.int64)
    flat, oflat = g.reshape(-1, n), out.reshape(-1, n)
    step = max(1, (1 << 22) // (n * n))
    for k in range(0, len(flat), step):
        oflat[k:k + step] = (flat[k:k + step, None, :] + table[None, :, :]).min(axis=-1)
    return np.moveaxis(out, -1, axis)


def d2_separable(site, radius=None):
    """the separable brute force: along x from the site flags, then y, then z.  (nz, ny, nx) int64; NO_SITE without a site"""
    f = np.where(site, np.int64(0), _BIG)
    for axis in (2, 1, 0):
        f = _min_plus(f, axis, radius)
    return np.where(f >= _BIG, np.int64(NO_SITE), f)


def words(vol, tsdf_words, min_weight=1, sites=SURFACE, form="separable", **wrong):
    """the ESDF words of a volume: form "full" or "separable".  wrong: metric="city" (full), radius=8 (separable), or
    neighbours=... -- deliberately wrong stand-ins"""
    flags, site = classify(vol, tsdf_words, min_weight, sites, **({"neighbours": wrong["neighbours"]} if "neighbours" in wrong else {}))
    if form == "full":
        d2 = d2_full(site, metric=wrong.get("metric", "euclid"))
    else:
        d2 = d2_separable(site, wrong.get("radius"))
    return (flags | d2.astype(np.uint32)).reshape(-1)


def signed(esdf_words, voxel_size):
    """+-voxel_size * sqrt(d2) as float64 (the value of NO_SITE words is not meaningful)"""
    w = np.asarray(esdf_words, np.uint32)
    d = np.float64(voxel_size) * np.sqrt((w & np.uint32(NO_SITE)).astype(np.float64))
    return np.where((w & np.uint32(INSIDE)) != 0, -d, d)


def metres(vol, esdf_words):
    w = np.asarray(esdf_words, np.uint32)
    d = signed(w, vol["voxel_size"]).astype(np.float32)
    inf = np.where((w & np.uint32(INSIDE)) != 0, np.float32(-np.inf), np.float32(np.inf))
    return np.where((w & np.uint32(NO_SITE)) == NO_SITE, inf, d).astype(np.float32)


def query(vol, esdf_words, points):
    """the point query, one record of SAMPLE_DTYPE per point; every step in the header's order"""
    nx, ny, nz = vol["dims"]
    vs = np.float64(vol["voxel_size"])
    w = np.asarray(esdf_words, np.uint32)
    P = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(P), SAMPLE_DTYPE)
    out["status"] = OUTSIDE
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(P[:, k] - np.float64(vol["origin"][k])) / vs for k in range(3)]
        i = [np.floor(gk) for gk in g]
        ok = np.ones(len(P), bool)
        for k, n in enumerate((nx, ny, nz)):
            ok &= (i[k] >= 0.0) & (i[k] + 1.0 <= np.float64(n - 1))
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return out
    ix, iy, iz = (i[k][idx].astype(np.int64) for k in range(3))
    fx, fy, fz = (g[k][idx] - i[k][idx] for k in range(3))
    a = ix + nx * (iy + ny * iz)
    corner = [w[a + (c & 1) + nx * ((c >> 1) & 1) + nx * ny * (c >> 2)] for c in range(8)]
    unknown = sum(((c & np.uint32(UNKNOWN)) != 0).astype(np.int32) for c in corner)
    none = np.zeros(len(idx), bool)
    for c in corner:
        none |= (c & np.uint32(NO_SITE)) == NO_SITE
    v = [signed(c, vs) for c in corner]
    c00 = v[0] + fx * (v[1] - v[0]); c10 = v[2] + fx * (v[3] - v[2]); c01 = v[4] + fx * (v[5] - v[4]); c11 = v[6] + fx * (v[7] - v[6])
    c0 = c00 + fy * (c10 - c00); c1 = c01 + fy * (c11 - c01)
    x00 = v[1] - v[0]; x10 = v[3] - v[2]; x01 = v[5] - v[4]; x11 = v[7] - v[6]
    x0 = x00 + fy * (x10 - x00); x1 = x01 + fy * (x11 - x01)
    y0 = c10 - c00; y1 = c11 - c01
    dist = c0 + fz * (c1 - c0)
    grad = np.stack([(x0 + fz * (x1 - x0)) / vs, (y0 + fz * (y1 - y0)) / vs, (c1 - c0) / vs], axis=1)
    rec = np.zeros(len(idx), SAMPLE_DTYPE)
    rec["status"] = np.where(none, NO_DISTANCE, FOUND)
    rec["unknown"] = unknown
    rec["distance"] = np.where(none, 0.0, dist)
    rec["gradient"] = np.where(none[:, None], 0.0, grad)
    out[idx] = rec
    return out


# ---- the shared cases ----

RANDOM_VOLUME = tr.volume((23, 9, 17), 0.03, (-0.3, -0.1, 0.5), 0.09)
COMBOS = [(1, SURFACE), (2, SURFACE), (1, SURFACE_AND_UNKNOWN), (2, SURFACE_AND_UNKNOWN)]
_fused = {}


def fused_cases():
    """[(name, volume, TSDF words)]: VOLUMES[0..3] after the frame list is fused, EDGE_VOLUME after its frame, and random words on two
    geometries; computed once, read-only"""
    if not _fused:
        out = [(n, v, w) for n, v, w in mr.cases() if n.startswith("volume")]
        out.append(("edge", tr.EDGE_VOLUME, tr.edge_run(tr.integrate, np.zeros(tr.voxels_of(tr.EDGE_VOLUME), np.uint32))))
        out.append(("random0", tr.VOLUMES[0], mr.random_words(tr.VOLUMES[0])))
        out.append(("random23", RANDOM_VOLUME, mr.random_words(RANDOM_VOLUME, seed=6)))
        for _, _, w in out:
            w.setflags(write=False)
        _fused["all"] = out
    return _fused["all"]


def words_with_sites(dims, site_list, q_out=100, q_in=-100):
    """TSDF words of a volume of `dims`, every voxel observed (w = 1) and outside (q > 0), except that each (x, y, z) of site_list is
    inside: it and its axis neighbours become the sites.  A single inside voxel in a corner makes that corner and its neighbours sites"""
    nx, ny, nz = dims
    q = np.full((nz, ny, nx), q_out, np.int64)
    for x, y, z in site_list:
        q[z, y, x] = q_in
    return tr.make_words(q.reshape(-1), np.ones(q.size, np.int64))


def constructed_cases():
    """[(name, volume, TSDF words, check(esdf words (nz, ny, nx) d2, flags) or None)]: the constructed volumes of the tests"""
    vol = lambda dims: tr.volume(dims, 0.05, (0.0, 0.0, 0.5), 0.15)
    out = []
    # no site at all: all observed and outside; all observed and inside
    for name, q in (("no_site_outside", 50), ("no_site_inside", -50)):
        dims = (7, 5, 3)
        out.append((name, vol(dims), tr.make_words(np.full(105, q), np.ones(105, np.int64))))
    # every voxel a site: a checkerboard of signs
    dims = (6, 5, 4)
    z, y, x = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
    out.append(("all_sites", vol(dims), tr.make_words(np.where((x + y + z) % 2 == 0, 200, -200).reshape(-1), np.ones(120, np.int64))))
    # 70 x 67 x 65, all observed and outside except the corner voxel (0, 0, 0), which was never seen: no site with DVO_ESDF_SITES_SURFACE,
    # exactly one with DVO_ESDF_SITES_SURFACE_AND_UNKNOWN and min_weight 1
    w = np.ones(70 * 67 * 65, np.int64)
    w[0] = 0
    out.append(("corner", vol((70, 67, 65)), tr.make_words(np.full(w.size, 100), w)))
    # two sites at equal distance from the voxels between them
    out.append(("two_equal", vol((21, 3, 3)), words_with_sites((21, 3, 3), [(0, 1, 1), (20, 1, 1)])))
    out.append(("one_voxel", vol((1, 1, 1)), tr.make_words([77], [1])))
    out.append(("line_y", vol((1, 37, 1)), words_with_sites((1, 37, 1), [(0, 5, 0)])))
    out.append(("line_z", vol((1, 1, 41)), words_with_sites((1, 1, 41), [(0, 0, 33)])))
    out.append(("long_x", vol((1024, 3, 2)), words_with_sites((1024, 3, 2), [(0, 0, 0)])))
    out.append(("long_y", vol((3, 1024, 2)), words_with_sites((3, 1024, 2), [(2, 1023, 1)])))
    out.append(("long_z", vol((2, 3, 1024)), words_with_sites((2, 3, 1024), [(1, 1, 500)])))
    for _, _, w in out:
        w.setflags(write=False)
    return out


def tiling_cases(B, C):
    """[(name, volume, TSDF words)] around the tiling of the kernels: x of B - 1, B, B + 1, 2 B + 1 and y, z of C - 1, C, C + 1, the other
    dimensions 3 and 5, each with one inside voxel at the far end so that the nearest site of the voxels at the near end lies in another
    row chunk or column tile"""
    vol = lambda dims: tr.volume(dims, 0.04, (-0.1, 0.0, 0.4), 0.12)
    out = []
    for nx in (B - 1, B, B + 1, 2 * B + 1):
        out.append(("x%d" % nx, vol((nx, 3, 5)), words_with_sites((nx, 3, 5), [(nx - 1, 2, 4)])))
    for n in (C - 1, C, C + 1):
        out.append(("y%d" % n, vol((3, n, 5)), words_with_sites((3, n, 5), [(0, n - 1, 0)])))
        out.append(("z%d" % n, vol((5, 3, n)), words_with_sites((5, 3, n), [(4, 0, n - 1)])))
    return out


_reference = {}


def reference(name, vol, tsdf_words, min_weight, sites):
    """words(..., form="separable") of a named case, computed once and shared, read-only"""
    key = (name, min_weight, sites)
    if key not in _reference:
        w = words(vol, tsdf_words, min_weight, sites)
        w.setflags(write=False)
        _reference[key] = w
    return _reference[key]


def check_words(esdf_under_test, case_list, combos=COMBOS, full_limit=2.0e10):
    """shared by the CPU tests (the host definition, and deliberately wrong stand-ins) and the GPU tests:
    `esdf_under_test(vol, tsdf_words, min_weight, sites)` returns the ESDF words.  They must equal the separable brute force word for
    word and, where voxels x sites <= full_limit, the full brute force too (which must equal the separable one)"""
    for name, vol, tw in case_list:
        for mw, sites in combos:
            want = reference(name, vol, tw, mw, sites)
            got = np.asarray(esdf_under_test(vol, tw, mw, sites))
            assert got.dtype == np.uint32 and got.shape == want.shape, "the words of %s have the wrong shape or type" % name
            flags_differ = int(((got ^ want) & np.uint32(~NO_SITE & 0xFFFFFFFF)).astype(bool).sum())
            assert flags_differ == 0, "flag bits of %s differ from the restatement (min_weight %d, sites %d): %d words" % (name, mw, sites, flags_differ)
            differ = int((got != want).sum())
            assert differ == 0, "d2 of %s differs from the separable brute force (min_weight %d, sites %d): %d words" % (name, mw, sites, differ)
            _, site = classify(vol, tw, mw, sites)
            if float(site.size) * float(site.sum()) <= full_limit:
                full = words(vol, tw, mw, sites, form="full")
                assert np.array_equal(full, want), "the two numpy forms differ on %s (min_weight %d, sites %d)" % (name, mw, sites)


# ---- the query points ----

def query_points(vol, esdf_words, seed=3, n=300):
    """seeded points of a volume: inside cells, on lattice planes, in the last cell, outside by one ulp on either side of every axis, and
    the centres of cells that have an unknown corner or a no-distance corner where the words have such cells.  (m, 3) float64, all
    finite"""
    nx, ny, nz = vol["dims"]
    vs, o = vol["voxel_size"], np.array(vol["origin"], np.float64)
    dims = np.array([nx, ny, nz], np.float64)
    rng = np.random.RandomState(9000 + seed)
    pts = [o + vs * rng.uniform(-0.5, 1.0, size=(n, 3)) * (dims - 1.0) * np.array([1.0, 1.0, 1.0])]
    lattice = o + vs * np.floor(rng.uniform(0, 1, size=(n // 4, 3)) * dims)                      # on lattice planes, every axis
    mixed = lattice.copy()
    mixed[:, 1] += vs * rng.uniform(0, 1, size=len(mixed))                                       # on the x and z planes only
    last = o + vs * (dims - 2.0 + rng.uniform(0, 1, size=(n // 4, 3)))                           # the last cell
    hi = o + vs * (dims - 1.0)                                                                   # the last lattice point: its cell is outside
    edge = []
    mid = o + vs * (dims - 1.0) / 2.0
    for k in range(3):
        for value in (np.nextafter(o[k], -np.inf), o[k], np.nextafter(hi[k], -np.inf), hi[k], np.nextafter(hi[k], np.inf)):
            p = mid.copy()
            p[k] = value
            edge.append(p)
    pts += [lattice, mixed, last, np.array(edge), hi[None], o[None]]
    w = np.asarray(esdf_words, np.uint32).reshape(nz, ny, nx)
    for mask in ((w & np.uint32(UNKNOWN)) != 0, (w & np.uint32(NO_SITE)) == NO_SITE):
        zs, ys, xs = np.nonzero(mask[:max(nz - 1, 0), :max(ny - 1, 0), :max(nx - 1, 0)])
        if len(zs):
            pick = rng.choice(len(zs), size=min(len(zs), 16), replace=False)
            pts.append(o + vs * (np.stack([xs[pick], ys[pick], zs[pick]], axis=1) + 0.5))
    return np.ascontiguousarray(np.concatenate(pts, axis=0))
