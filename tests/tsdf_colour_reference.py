"""Colour in the map (include/dvo_amd.h, "colour in the map") restated in numpy from the text of the definition, independently of
rgbd_odometry_amd/csrc/dvo_tsdf_colour.h: int64 for the running means, float64 in the stated order for the interpolations; numpy never
fuses.  The uncoloured parts -- the words of a fusion, the march of a ray, the vertices of a mesh -- come from the restatements of their
own sections (tsdf_map_reference, tsdf_raycast_reference, tsdf_mesh_reference).  Also the cases the CPU and GPU tests share.  A volume's
colour state is nx * ny * nz uint64 words: r, g, b in 1/256 levels and the count wc, 16 bits each from the low end."""
import numpy as np

import tsdf_map_reference as tr
import tsdf_mesh_reference as mr
import tsdf_raycast_reference as rr

BGR8, RGB8, MONO8 = 0, 1, 2
FORMATS = {"bgr8": BGR8, "rgb8": RGB8, "mono8": MONO8}


# ---- the colour word ----

def colour_channel(colours, ch):
    return ((np.asarray(colours, np.uint64) >> np.uint64(16 * ch)) & np.uint64(0xFFFF)).astype(np.int64)


def colour_wc(colours):
    return (np.asarray(colours, np.uint64) >> np.uint64(48)).astype(np.int64)


def make_colours(r, g, b, wc):
    u = lambda a: np.asarray(a, np.int64).astype(np.uint64)
    return u(r) | (u(g) << np.uint64(16)) | (u(b) << np.uint64(32)) | (u(wc) << np.uint64(48))


# ---- pixels ----

def image_rgb(image, fmt):
    """(rows, cols, 3) int64 R, G, B of an image in format fmt"""
    m = np.asarray(image)
    assert m.dtype == np.uint8
    if fmt == MONO8:
        return np.repeat(m.astype(np.int64)[:, :, None], 3, axis=2)
    return m.astype(np.int64) if fmt == RGB8 else m[:, :, ::-1].astype(np.int64)


def image_of_levels(levels, fmt):
    """levels (..., 3) int64 R, G, B -> the bytes of an image in format fmt"""
    R, G, B = levels[..., 0], levels[..., 1], levels[..., 2]
    if fmt == MONO8:
        return ((1868 * B + 9617 * G + 4899 * R + 8192) >> 14).astype(np.uint8)
    return np.stack([R, G, B] if fmt == RGB8 else [B, G, R], axis=-1).astype(np.uint8)


def level(c):
    """the 8-bit level of channel values in 1/256 levels (float64)"""
    return np.clip(np.floor(c / 256.0 + 0.5), 0.0, 255.0).astype(np.int64)


# ---- fusing ----

def band(vol, depth, K, pose, z_near=tr.Z_NEAR, z_far=tr.Z_FAR):
    """(in_band (nz, ny, nx) bool: the voxel is not skipped and sdf <= trunc; vv, uu: the pixel its depth was read from)"""
    nx, ny, nz = vol["dims"]
    vs, o, trunc = vol["voxel_size"], vol["origin"], vol["trunc"]
    rows, cols = depth.shape
    R, t = np.asarray(pose, np.float64)[:9], np.asarray(pose, np.float64)[9:]
    fx, fy, cx, cy = (float(k) for k in K)
    wx = (o[0] + vs * np.arange(nx, dtype=np.float64))[None, None, :]
    wy = (o[1] + vs * np.arange(ny, dtype=np.float64))[None, :, None]
    wz = (o[2] + vs * np.arange(nz, dtype=np.float64))[:, None, None]
    dx, dy, dz = wx - t[0], wy - t[1], wz - t[2]
    with np.errstate(all="ignore"):
        X = R[0] * dx + R[1] * dy + R[2] * dz
        Y = R[3] * dx + R[4] * dy + R[5] * dz
        Z = R[6] * dx + R[7] * dy + R[8] * dz
        ok = Z > z_near
        iz = 1.0 / Z
        u = fx * (X * iz) + cx
        v = fy * (Y * iz) + cy
        ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
        ok &= (ui >= 0.0) & (ui < float(cols)) & (vi >= 0.0) & (vi < float(rows))
        uu, vv = np.where(ok, ui, 0.0).astype(np.int64), np.where(ok, vi, 0.0).astype(np.int64)
        D_img, hole_img = tr.metres(depth)
        D, hole = D_img[vv, uu], hole_img[vv, uu]
        ok &= ~hole
        ok &= ~(D > z_far)
        sdf = D - Z
        ok &= ~(sdf < -trunc)
        ok &= sdf <= trunc
    return ok, vv, uu


def integrate_frame(vol, words, colours, depth, image, fmt, K, pose, z_near=tr.Z_NEAR, z_far=tr.Z_FAR, max_weight=tr.MAX_WEIGHT):
    """one frame into the words and the colour words (new arrays)"""
    nx, ny, nz = vol["dims"]
    new_words = tr.integrate_frame(vol, words, depth, K, pose, z_near=z_near, z_far=z_far, max_weight=max_weight)
    ok, vv, uu = band(vol, depth, K, pose, z_near, z_far)
    C = image_rgb(image, fmt)[vv, uu]                                  # (nz, ny, nx, 3)
    c0 = np.asarray(colours, np.uint64).reshape(nz, ny, nx)
    wc = colour_wc(c0)
    new = [(colour_channel(c0, ch) * wc + 256 * C[..., ch] + ((wc + 1) >> 1)) // (wc + 1) for ch in range(3)]
    assert all(int(n.max()) < 2 ** 32 for n in new)
    out = make_colours(new[0], new[1], new[2], np.minimum(wc + 1, max_weight))
    return new_words, np.where(ok, out, c0).reshape(-1).astype(np.uint64)


def integrate(vol, words, colours, depths, images, fmt, Ks, poses, **params):
    """a frame list, in list order (words, colours None: a cleared volume); returns (words, colours)"""
    words = np.zeros(tr.voxels_of(vol), np.uint32) if words is None else np.array(words, np.uint32).reshape(-1)
    colours = np.zeros(tr.voxels_of(vol), np.uint64) if colours is None else np.array(colours, np.uint64).reshape(-1)
    Ks = np.asarray(Ks, np.float64)
    for i, d in enumerate(depths):
        words, colours = integrate_frame(vol, words, colours, d, images[i], fmt, Ks if Ks.ndim == 1 else Ks[i], poses[i], **params)
    return words, colours


# ---- a ray-cast view ----

def colour_sample(vol, colours, gx, gy, gz):
    """(valid, levels (..., 3) int64) at the voxel coordinates g"""
    nx, ny, nz = vol["dims"]
    with np.errstate(all="ignore"):
        ix, iy, iz = np.floor(gx), np.floor(gy), np.floor(gz)
        ok = ((ix >= 0.0) & (ix + 1.0 <= float(nx - 1)) & (iy >= 0.0) & (iy + 1.0 <= float(ny - 1)) & (iz >= 0.0) & (iz + 1.0 <= float(nz - 1)))
        fx, fy, fz = gx - ix, gy - iy, gz - iz
        base = (np.where(ok, ix, 0.0).astype(np.int64) +
                nx * (np.where(ok, iy, 0.0).astype(np.int64) + ny * np.where(ok, iz, 0.0).astype(np.int64)))
        if nx < 2 or ny < 2 or nz < 2:
            return np.zeros(ok.shape, bool), np.zeros(ok.shape + (3,), np.int64)
        W = np.asarray(colours, np.uint64).reshape(-1)
        corner = {(dx, dy, dz): W[base + dx + nx * dy + nx * ny * dz] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
        for c in corner.values():
            ok = ok & (colour_wc(c) >= 1)
        out = []
        for ch in range(3):
            q = {k: colour_channel(c, ch).astype(np.float64) for k, c in corner.items()}
            c00 = q[0, 0, 0] + fx * (q[1, 0, 0] - q[0, 0, 0])
            c10 = q[0, 1, 0] + fx * (q[1, 1, 0] - q[0, 1, 0])
            c01 = q[0, 0, 1] + fx * (q[1, 0, 1] - q[0, 0, 1])
            c11 = q[0, 1, 1] + fx * (q[1, 1, 1] - q[0, 1, 1])
            c0 = c00 + fy * (c10 - c00)
            c1 = c01 + fy * (c11 - c01)
            out.append(level(np.where(ok, c0 + fz * (c1 - c0), 0.0)))
    return ok, np.stack(out, axis=-1)


def raycast_view(vol, words, colours, K, pose, rows, cols, **settings):
    """rr.raycast_view's dict plus levels_u16 and levels_f32: (rows, cols, 3) int64 R, G, B under either depth format (a pixel whose
    16-bit depth is out of range is a hole there)"""
    out = rr.raycast_view(vol, words, K, pose, rows, cols, **settings)
    fx, fy, cx, cy = (float(k) for k in K)
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    g = rr.ray_point(vol, pose, (u - cx) / fx, (v - cy) / fy, out["Zs"])
    ok, levels = colour_sample(vol, colours, *g)
    for name in ("u16", "f32"):
        hit = out[name] != 0 if name == "u16" else out["kind"] == rr.HIT
        out["levels_" + name] = np.where((ok & hit)[..., None], levels, 0)
    return out


# ---- a mesh ----

def mesh_colours(vol, words, colours, min_weight=1):
    """(colours (n, 3) uint8 R, G, B of the vertices of mr.mesh in their order, how many coloured ends (0, 1, 2) each vertex has)"""
    nx, ny, nz = vol["dims"]
    W = np.asarray(words, np.uint32).reshape(nz, ny, nx)
    Cw = np.asarray(colours, np.uint64).reshape(nz, ny, nx)
    q, w = tr.word_q(W), tr.word_w(W)
    ok, neg = w >= min_weight, q < 0
    has = np.zeros((nz, ny, nx, 7), bool)
    rgb = np.zeros((nz, ny, nx, 7, 3), np.int64)
    ends = np.zeros((nz, ny, nx, 7), np.int64)
    has_a = colour_wc(Cw) >= 1
    for d, off in enumerate(mr.DIRS):
        shifted = lambda a, fill: mr._shifted(a, off, fill)
        hit = shifted(np.ones((nz, ny, nx), bool), False) & ok & shifted(ok, False) & (neg != shifted(neg, False))
        has[..., d] = hit
        with np.errstate(all="ignore"):
            lam = q.astype(np.float64) / (q - shifted(q, 0)).astype(np.float64)
        Cb = shifted(Cw, np.uint64(0))
        has_b = colour_wc(Cb) >= 1
        ends[..., d] = has_a.astype(np.int64) + has_b.astype(np.int64)
        for ch in range(3):
            ca, cb = colour_channel(Cw, ch).astype(np.float64), colour_channel(Cb, ch).astype(np.float64)
            with np.errstate(all="ignore"):
                both = ca + lam * (cb - ca)
            value = np.where(has_a & has_b, both, np.where(has_a, ca, np.where(has_b, cb, 0.0)))
            rgb[..., d, ch] = level(np.where(hit, value, 0.0))
    flat = has.reshape(-1)
    return rgb.reshape(-1, 3)[flat].astype(np.uint8), ends.reshape(-1)[flat]


# ---- the shared cases ----

def images(kind, fmt, size=(tr.ROWS, tr.COLS)):
    """the seven frames' images, 24 x 32 unless another size is given, seeded: kind "random" (every pixel and channel on its own) or
    "gradient" (smooth ramps with a different slope per channel and frame); fmt "bgr8", "rgb8" (the same colours, channels exchanged) or
    "mono8" (their engine grey)"""
    rows, cols = size
    out = []
    for i in range(7):
        if kind == "random":
            rgb = np.random.RandomState(7000 + i).randint(0, 256, size=(rows, cols, 3)).astype(np.int64)
        else:
            v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
            rgb = np.stack([(u * (5 + i) + v) % 256, (v * (7 + i) + 2 * u + 40 * i) % 256, 255 - (u * 3 + v * 4 + 9 * i) % 256], axis=-1).astype(np.int64)
        out.append(image_of_levels(rgb, FORMATS[fmt]))
    return out


def random_colours(vol, seed=5):
    """channels over 0 .. 65280, wc in 0 .. 2: vertices with no, one and two coloured ends all occur"""
    n = tr.voxels_of(vol)
    rng = np.random.RandomState(6000 + seed)
    r, g, b = (rng.randint(0, 65281, size=n) for _ in range(3))
    return make_colours(r, g, b, rng.randint(0, 3, size=n))


def analytic_colours():
    """SPHERE and TORUS: colour as a function of position, wc = 1 everywhere"""
    nx, ny, nz = mr.ANALYTIC_VOLUME["dims"]
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r, g, b = 256 * (ix * 3 % 256) + iy, 256 * (iy * 3 % 256) + iz, 256 * (255 - iz * 3 % 256)
    return make_colours(r.reshape(-1), g.reshape(-1), b.reshape(-1), np.ones(nx * ny * nz, np.int64))


_fused = {}


def fused(kind="random", fmt="bgr8", depth="u16"):
    """[(vol, words, colours)] of the four volumes after their frames of the seven, by the restatement; computed once, read-only"""
    key = (kind, fmt, depth)
    if key not in _fused:
        imgs, poses = tr.frame_list(depth)
        cols = images(kind, fmt)
        out = []
        for vi, vol in enumerate(tr.VOLUMES):
            idx = [i for i, v in enumerate(tr.FRAME_VOLUMES) if v == vi]
            w, c = integrate(vol, None, None, [imgs[i] for i in idx], [cols[i] for i in idx], FORMATS[fmt], tr.K4, poses[idx])
            w.setflags(write=False)
            c.setflags(write=False)
            out.append((vol, w, c))
        _fused[key] = out
    return _fused[key]


_mesh_cases = {}


def mesh_case(name):
    """(vol, words, colours) of a mesh case: volume0 .. volume3 fused with the random bgr8 images, random1 with random colour words,
    SPHERE and TORUS with the analytic colours; computed once, read-only"""
    if name not in _mesh_cases:
        if name.startswith("volume"):
            _mesh_cases[name] = fused()[int(name[6:])]
        else:
            vol, words = mr.case(name)
            c = random_colours(vol) if name == "random1" else analytic_colours()
            c.setflags(write=False)
            _mesh_cases[name] = (vol, words, c)
    return _mesh_cases[name]


MESH_CASES = [(name, mw) for name in mr.CASE_NAMES for mw in mr.MIN_WEIGHTS[name]]

_mesh_reference = {}


def mesh_reference(name, min_weight):
    """(vertices, triangles, colours (n, 3) uint8, coloured ends per vertex) of a mesh case; computed once"""
    key = (name, min_weight)
    if key not in _mesh_reference:
        vol, words, colours = mesh_case(name)
        v, t = mr.reference(name, min_weight)[:2]
        rgb, ends = mesh_colours(vol, words, colours, min_weight)
        assert len(rgb) == len(v)
        _mesh_reference[key] = (v, t, rgb, ends)
    return _mesh_reference[key]


def edge_image(levels=(10, 200, 77)):
    """an image for tr.EDGE_DEPTH: one colour everywhere, as rgb8"""
    return np.tile(np.array(levels, np.uint8), (tr.ROWS, tr.COLS, 1))


# ---- rounding and limits on tr.EDGE_VOLUME, with states crafted through the words ----

EDGE_LEVELS = (10, 200, 77)


def edge_run(integrate_under_test, words, colours, vol=tr.EDGE_VOLUME, frames=1, levels=EDGE_LEVELS, **params):
    return integrate_under_test(vol, words, colours, [tr.EDGE_DEPTH] * frames, [edge_image(levels)] * frames, RGB8, tr.EDGE_K,
                                np.stack([tr.pose12()] * frames), **params)


def check_rounding_and_limits(integrate_under_test):
    """shared with the GPU tests: `integrate_under_test(vol, words, colours, depths, images, fmt, K, poses, **params)` -> (words,
    colours) is the implementation under test; every result is also the restatement's"""
    n = tr.voxels_of(tr.EDGE_VOLUME)
    zeros, czeros = np.zeros(n, np.uint32), np.zeros(n, np.uint64)

    def both(words, colours, **kw):
        got_w, got_c = edge_run(integrate_under_test, words, colours, **kw)
        ref_w, ref_c = edge_run(integrate, words, colours, **kw)
        assert np.array_equal(got_w, ref_w) and np.array_equal(got_c, ref_c), kw
        return got_w, got_c

    # a fresh volume: sdf = +trunc exactly, 0 and -trunc exactly are all inside the band: every voxel coloured once, channel = 256 C
    w, c = both(zeros, czeros)
    assert np.all(colour_wc(c) == 1) and np.all(tr.word_w(w) == 1)
    for ch in range(3):
        assert np.all(colour_channel(c, ch) == 256 * EDGE_LEVELS[ch])
    # trunc the next double below 0.25: sdf = 0.25 > trunc takes depth but no colour, sdf = -0.25 < -trunc takes nothing
    tight = dict(tr.EDGE_VOLUME, trunc=float(np.nextafter(0.25, 0.0)))
    w, c = both(zeros, czeros, vol=tight)
    assert np.all(tr.word_w(w[tr.PLANE[0.5]]) == 1) and np.all(c[tr.PLANE[0.5]] == 0)
    assert np.all(tr.word_w(w[tr.PLANE[0.75]]) == 1) and np.all(colour_wc(c[tr.PLANE[0.75]]) == 1)
    assert np.all(w[tr.PLANE[1.0]] == 0) and np.all(c[tr.PLANE[1.0]] == 0)
    # half-up ties: (1 * 1 + 0 + 1) / 2 = 1, (3 * 1 + 0 + 1) / 2 = 2
    for start, want in ((1, 1), (3, 2)):
        w, c = both(zeros, make_colours(np.full(n, start), np.full(n, start), np.full(n, start), np.ones(n, np.int64)), levels=(0, 0, 0))
        assert np.all(colour_wc(c) == 2) and all(np.all(colour_channel(c, ch) == want) for ch in range(3)), start
    # the largest values stay where they are: (65280 * 65535 + 65280 + 32768) / 65536 = 65280, wc = max_weight = 65535
    top = make_colours(np.full(n, 65280), np.full(n, 65280), np.full(n, 65280), np.full(n, 65535))
    w, c = both(zeros, top, levels=(255, 255, 255), max_weight=65535)
    assert np.array_equal(c, top)
    # max_weight 3 over five frames ends at 3
    w, c = both(zeros, czeros, frames=5, max_weight=3)
    assert np.all(colour_wc(c) == 3) and np.all(tr.word_w(w) == 3)
