"""Depth fusion (include/dvo_amd.h, "depth fusion") restated in numpy: the definition of rgbd_odometry_amd/csrc/dvo_tsdf_map.h, written
from its text -- IEEE double in the order written, numpy never fuses -- plus the volumes, scenes and frame lists the CPU and GPU tests
share.  A volume is a dict(dims=(nx, ny, nz), voxel_size, origin, trunc); its state is nx * ny * nz uint32 words."""
import numpy as np

ROWS, COLS = 24, 32
K4 = (30.0, 30.0, 15.5, 11.5)
QMAX = 32767.0
Z_NEAR, Z_FAR, MAX_WEIGHT = 0.1, 8.0, 128


def volume(dims, voxel_size, origin, trunc):
    return dict(dims=tuple(int(d) for d in dims), voxel_size=float(voxel_size), origin=tuple(float(o) for o in origin), trunc=float(trunc))


#: the four volumes of the tests, in the order the GPU tests set them: odd sizes, one larger than a workgroup's share, two tiny ones
VOLUMES = [volume((20, 14, 11), 0.05, (-0.5, -0.35, 0.6), 0.15),
           volume((64, 48, 40), 0.02, (-0.64, -0.48, 0.45), 0.06),
           volume((5, 3, 2), 0.1, (-0.2, -0.1, 0.8), 0.15),
           volume((1, 1, 1), 0.1, (0.0, 0.0, 0.8), 0.2)]


def voxels_of(vol):
    nx, ny, nz = vol["dims"]
    return nx * ny * nz


def word_q(words):
    return (np.asarray(words, np.uint32) & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int64)


def word_w(words):
    return (np.asarray(words, np.uint32) >> np.uint32(16)).astype(np.int64)


def make_words(q, w):
    return ((np.asarray(w, np.int64).astype(np.uint32) << np.uint32(16)) |
            (np.asarray(q, np.int64).astype(np.int16).view(np.uint16).astype(np.uint32))).astype(np.uint32)


def pose12(R=None, t=None):
    """{R column-major, t}, camera to world"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64).reshape(3)
    return np.concatenate([R.T.ravel(), t])


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def metres(depth):
    """(D float64, hole mask) of a raw image"""
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        return d.astype(np.float64) / 1000.0, d == 0
    if d.dtype != np.float32:
        raise ValueError("uint16 millimetres or float32 metres")
    D = d.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return D, ~(np.isfinite(D) & (D > 0.0))


def integrate_frame(vol, words, depth, K, pose, z_near=Z_NEAR, z_far=Z_FAR, max_weight=MAX_WEIGHT):
    """one frame into the words (a new array)"""
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
        D_img, hole_img = metres(depth)
        D, hole = D_img[vv, uu], hole_img[vv, uu]
        ok &= ~hole
        ok &= ~(D > z_far)
        sdf = D - Z
        ok &= ~(sdf < -trunc)
        f = sdf * (1.0 / trunc)
        f = np.where(f > 1.0, 1.0, f)
        F = f * QMAX
        w0 = np.asarray(words, np.uint32).reshape(nz, ny, nx)
        q, w = word_q(w0).astype(np.float64), word_w(w0)
        qn = np.rint((q * w.astype(np.float64) + F) / (w.astype(np.float64) + 1.0))
        wn = np.minimum(w + 1, max_weight)
        new = make_words(np.where(ok, qn, 0.0).astype(np.int64), wn)
    return np.where(ok, new, w0).reshape(-1).astype(np.uint32)


def integrate(vol, words, depths, Ks, poses, **params):
    """a frame list, in list order (words None: a cleared volume)"""
    words = np.zeros(voxels_of(vol), np.uint32) if words is None else np.array(words, np.uint32).reshape(-1)
    Ks = np.asarray(Ks, np.float64)
    for i, d in enumerate(depths):
        words = integrate_frame(vol, words, d, Ks if Ks.ndim == 1 else Ks[i], poses[i], **params)
    return words


def extract(vol, words, min_weight=1):
    """(points (n, 3) float32 in the definition's order, the axis of each point)"""
    nx, ny, nz = vol["dims"]
    vs, o = vol["voxel_size"], vol["origin"]
    W = np.asarray(words, np.uint32).reshape(nz, ny, nx)
    q, w = word_q(W), word_w(W)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    centre = [o[0] + vs * ix.astype(np.float64), o[1] + vs * iy.astype(np.float64), o[2] + vs * iz.astype(np.float64)]
    index = ix + nx * (iy + ny * iz)
    keys, pts, axes = [], [], []
    for axis, (sa, sb) in enumerate([((slice(None), slice(None), slice(0, -1)), (slice(None), slice(None), slice(1, None))),
                                     ((slice(None), slice(0, -1), slice(None)), (slice(None), slice(1, None), slice(None))),
                                     ((slice(0, -1), slice(None), slice(None)), (slice(1, None), slice(None), slice(None)))]):
        qa, qb, wa, wb = q[sa], q[sb], w[sa], w[sb]
        hit = (wa >= min_weight) & (wb >= min_weight) & ((qa < 0) != (qb < 0))
        if not hit.any():
            continue
        lam = qa[hit].astype(np.float64) / (qa[hit] - qb[hit]).astype(np.float64)
        p = [c[sa][hit] for c in centre]
        p[axis] = p[axis] + lam * vs
        pts.append(np.stack(p, axis=1).astype(np.float32))
        keys.append(index[sa][hit] * 3 + axis)
        axes.append(np.full(int(hit.sum()), axis))
    if not keys:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int64)
    keys, pts, axes = np.concatenate(keys), np.concatenate(pts), np.concatenate(axes)
    order = np.argsort(keys, kind="stable")
    return pts[order], axes[order]


# ---- scenes and frame lists ----

#: the image sizes beside 24 x 32.  37 x 53: a 16-bit image is 3922 bytes, a float one 7844, an rgb8 one 5883 and a mono8 one 1961 --
#: none a multiple of 16, so every staged image after the first starts at a padded offset.  480 x 640: pixel indices beyond 65,535 and
#: a row pitch that is no power of two
ODD_SIZE, VGA_SIZE = (37, 53), (480, 640)


def k4_for(rows, cols):
    """K4 for the 24 x 32 image; for another size the same field of view"""
    if (rows, cols) == (ROWS, COLS):
        return K4
    s = cols / float(COLS)
    return (K4[0] * s, K4[1] * s, (cols - 1) / 2.0, (rows - 1) / 2.0)


def scene_u16(seed=0, holes=0.05, size=(ROWS, COLS)):
    """a plane at 850 mm with a nearer box at 700 mm over the middle third of the image (at 24 x 32 rows 8-15, columns 10-19), and
    5 % holes"""
    rows, cols = size
    d = np.full((rows, cols), 850, np.uint16)
    d[rows // 3:2 * rows // 3, cols // 3:5 * cols // 8] = 700
    rng = np.random.RandomState(1000 + seed)
    d[rng.rand(rows, cols) < holes] = 0
    return d


def as_f32(d16):
    return (d16.astype(np.float64) / 1000.0).astype(np.float32)


#: seven poses: identity, rotated and translated cameras that all still see the volumes
POSES = [pose12(),
         pose12(rot(1, 0.10), (0.08, 0.0, 0.0)),
         pose12(rot(0, 0.08) @ rot(1, -0.12), (0.0, 0.02, 0.0)),
         pose12(t=(0.06, -0.04, 0.03)),
         pose12(t=(-0.05, 0.05, -0.02)),
         pose12(rot(2, 0.2), (0.05, -0.03, -0.05)),
         pose12(rot(1, -0.07), (-0.03, 0.0, 0.02))]
#: the volume each of the seven frames goes into (indices into VOLUMES)
FRAME_VOLUMES = [0, 1, 0, 2, 1, 0, 3]


def frame_list(fmt, size=(ROWS, COLS)):
    """the seven frames: (depth images, poses (7, 12)); fmt "u16" or "f32"; their camera is k4_for(*size)"""
    imgs = [scene_u16(i, size=size) for i in range(7)]
    if fmt == "f32":
        imgs = [as_f32(d) for d in imgs]
    return imgs, np.stack(POSES)


#: the case at 480 x 640: the first three frames of the list, all three into each of the volumes 0, 2 and 3 (volume 1 left out keeps
#: the restatement to a fraction of a second)
VGA_VOLUMES, VGA_FRAMES = [0, 0, 0, 2, 2, 2, 3, 3, 3], [0, 1, 2, 0, 1, 2, 0, 1, 2]


def seen_and_negative(words):
    """(voxels with a weight, voxels with a weight and a negative distance)"""
    return int((word_w(words) > 0).sum()), int(((word_w(words) > 0) & (word_q(words) < 0)).sum())


def f32_specials(seed=7):
    """metres with NaN, both infinities, zeros, negative values and values beyond z_far mixed in"""
    d = as_f32(scene_u16(seed, holes=0.0))
    rng = np.random.RandomState(2000 + seed)
    pick = rng.randint(0, 12, size=d.shape)
    d[pick == 0] = np.nan
    d[pick == 1] = np.inf
    d[pick == 2] = -np.inf
    d[pick == 3] = -0.85
    d[pick == 4] = 0.0
    d[pick == 5] = 8.5
    return d


def degenerate_frames():
    """[(name, depth image, pose)]: ordinary inputs of the definition that exercise its skips"""
    v0 = VOLUMES[0]
    mid = [v0["origin"][k] + v0["voxel_size"] * (v0["dims"][k] - 1) / 2.0 for k in range(3)]
    return [("looking_away", scene_u16(11), pose12(np.diag([-1.0, 1.0, -1.0]))),
            ("camera_inside", scene_u16(12), pose12(t=mid)),
            ("all_holes", np.zeros((ROWS, COLS), np.uint16), pose12()),
            ("f32_specials", f32_specials(), pose12()),
            ("beyond_2_30", scene_u16(13), pose12(t=(-1.0e9, 2.0e9, 0.0)))]


# ---- rounding and limits, with states crafted through the words ----
# a 3 x 3 x 3 volume whose z planes lie at exactly 0.5, 0.75 and 1.0 m in front of an identity camera that sees 0.75 m everywhere (its
# focal length is short enough for every voxel to project into the image): sdf = +0.25 (f clipped to 1, F = 32767), 0 and
# -0.25 = -trunc exactly (F = -32767)
EDGE_VOLUME = volume((3, 3, 3), 0.25, (-0.25, -0.25, 0.5), 0.25)
EDGE_DEPTH = np.full((ROWS, COLS), 0.75, np.float32)
EDGE_K = (10.0, 10.0, 15.5, 11.5)
PLANE = {z: slice(9 * k, 9 * k + 9) for k, z in enumerate((0.5, 0.75, 1.0))}


def edge_run(integrate, words, vol=EDGE_VOLUME, frames=1, **params):
    return integrate(vol, words, [EDGE_DEPTH] * frames, EDGE_K, np.stack([pose12()] * frames), **params)


def check_rounding_and_limits(integrate_under_test):
    """shared with the GPU tests: `integrate_under_test(vol, words, imgs, K, poses, **params)` is the implementation under test"""
    n = voxels_of(EDGE_VOLUME)
    # a fresh volume: +32767 in front, 0 on the surface, -32767 at exactly -trunc, every weight 1
    got = edge_run(integrate_under_test, np.zeros(n, np.uint32))
    assert np.array_equal(got, edge_run(integrate, np.zeros(n, np.uint32)))
    assert np.all(word_w(got) == 1)
    assert np.all(word_q(got[PLANE[0.5]]) == 32767) and np.all(word_q(got[PLANE[0.75]]) == 0) and np.all(word_q(got[PLANE[1.0]]) == -32767)
    # q even, w = 1, F = 32767: (q + 32767) / 2 lands exactly on a half and rounds to the even neighbour
    for q, want in ((100, 16434), (102, 16434), (-100, 16334), (-102, 16332), (0, 16384), (2, 16384)):
        start = make_words(np.full(n, q), np.full(n, 1))
        got = edge_run(integrate_under_test, start)
        assert np.array_equal(got, edge_run(integrate, start)), q
        assert np.all(word_q(got[PLANE[0.5]]) == want) and np.all(word_w(got) == 2), (q, word_q(got[PLANE[0.5]]))
    # sdf == -trunc exactly is integrated (above); with trunc the next double below 0.25, sdf = -0.25 is the next double below -trunc
    # and the plane is skipped
    tight = dict(EDGE_VOLUME, trunc=float(np.nextafter(0.25, 0.0)))
    got = edge_run(integrate_under_test, np.zeros(n, np.uint32), vol=tight)
    assert np.array_equal(got, edge_run(integrate, np.zeros(n, np.uint32), vol=tight))
    assert np.all(got[PLANE[1.0]] == 0) and np.all(word_w(got[PLANE[0.75]]) == 1) and np.all(word_w(got[PLANE[0.5]]) == 1)
    # w = 65535 stays at max_weight 65535, and q = +-32767 stays where the frame agrees with it
    for q in (32767, -32767):
        start = make_words(np.full(n, q), np.full(n, 65535))
        got = edge_run(integrate_under_test, start, max_weight=65535)
        assert np.array_equal(got, edge_run(integrate, start, max_weight=65535)), q
        assert np.all(word_w(got) == 65535) and np.all(np.abs(word_q(got)) <= 32767)
        assert np.all(word_q(got[PLANE[0.5 if q > 0 else 1.0]]) == q)
    # max_weight 3 over five frames ends at 3
    got = edge_run(integrate_under_test, np.zeros(n, np.uint32), frames=5, max_weight=3)
    assert np.array_equal(got, edge_run(integrate, np.zeros(n, np.uint32), frames=5, max_weight=3))
    assert np.all(word_w(got) == 3)


# ---- a packed pool: volumes at every alignment of the pool's 16-byte groups ----

def packed_volume(dims, voxel_size, centre):
    """a volume by the centre of its lattice, trunc three voxels"""
    origin = [float(c) - voxel_size * (d - 1) / 2.0 for c, d in zip(centre, dims)]
    return volume(dims, voxel_size, origin, 3 * voxel_size)


#: 23 volumes whose pool is exactly their sum, set in this order.  The integrate kernel's thread owns an aligned group of four pool
#: words: volumes 0, 1, 2 and the first word of 3 share one group, 3 straddles two, 17 takes five workgroups from an offset of 2 mod 4,
#: 18 sits alone in the first word of the group behind it, 21 and 22 share the last group; nx of 1, 2 and 3 wrap inside every group
PACKED_VOLUMES = [packed_volume(*a) for a in (
    ((1, 1, 1), .05, (0, 0, .84)), ((1, 1, 1), .05, (.10, .05, .86)), ((1, 1, 1), .05, (-.1, 0, .80)), ((2, 1, 1), .04, (0, 0, .85)),
    ((1, 3, 1), .04, (.05, 0, .84)), ((1, 1, 3), .04, (0, .1, .85)), ((7, 1, 1), .03, (0, -.1, .85)), ((1, 1, 9), .02, (.12, .1, .85)),
    ((1, 9, 7), .03, (-.15, 0, .85)), ((9, 1, 7), .03, (0, .15, .85)), ((9, 7, 1), .03, (.1, -.1, .85)), ((2, 9, 7), .03, (.2, 0, .85)),
    ((3, 5, 4), .04, (-.2, .1, .82)), ((5, 4, 3), .04, (0, 0, .72)), ((1, 1, 1), .05, (0, 0, .70)), ((6, 5, 3), .04, (.15, .12, .84)),
    ((7, 3, 5), .03, (-.1, -.12, .84)), ((33, 17, 9), .02, (0, 0, .80)), ((1, 1, 1), .05, (.05, .05, .69)), ((4, 4, 4), .05, (0, 0, .85)),
    ((8, 3, 2), .04, (-.05, .05, .85)), ((1, 2, 1), .05, (0, 0, .68)), ((1, 1, 2), .05, (0, 0, .84)))]
#: the frames of the list that go into every volume of a cleared packed pool
PACKED_FRAMES = (0, 1, 3)
GROUP = 4                                        # words of one thread of the integrate kernel (kRun of dvo_tsdf_launch.h)
INTEGRATE_BLOCK = 256                            # threads of its workgroup (kBlock)


def pool_offsets(volumes):
    """the pool offset of every volume set back to back in order, and the pool's size"""
    off = np.concatenate([[0], np.cumsum([voxels_of(v) for v in volumes])]).astype(np.int64)
    return [int(o) for o in off[:-1]], int(off[-1])


def integrate_workgroups(off, n):
    """the workgroups the integrate launch gives a volume of n voxels at pool offset off (integrate_blocks of dvo_tsdf_launch.h)"""
    groups = (off + n + GROUP - 1) // GROUP - off // GROUP
    return (groups + INTEGRATE_BLOCK - 1) // INTEGRATE_BLOCK


def random_pool_words(rng, n):
    """any 32-bit pattern"""
    return rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def random_pool_colours(rng, n, max_weight=MAX_WEIGHT):
    """colour words as dvo_tsdf_colour.h leaves them: channels in 0 .. 65280, a count in 0 .. max_weight, 0 where the count is 0"""
    ch = [rng.randint(0, 65281, size=n).astype(np.uint64) for _ in range(3)]
    wc = rng.randint(0, max_weight + 1, size=n).astype(np.uint64)
    c = ch[0] | (ch[1] << np.uint64(16)) | (ch[2] << np.uint64(32)) | (wc << np.uint64(48))
    return np.where(wc == 0, np.uint64(0), c).astype(np.uint64)


def round_robin(order, queues):
    """one frame list from per-volume frame queues: (volumes, frames).  The volumes first appear in `order`, every volume's frames are
    interleaved with the others' and keep their own order"""
    volumes, frames = [], []
    for r in range(max(len(q) for q in queues.values())):
        for v in order:
            if r < len(queues[v]):
                volumes.append(int(v))
                frames.append(int(queues[v][r]))
    return volumes, frames


def check_packed_pool(make_handle, image_format=None, formats=("u16", "f32"), seed=11):
    """shared by the CPU tests (Python stand-ins of a handle, a correct one and deliberately wrong ones) and the GPU tests:
    `make_handle(volumes)` returns a handle over one cleared pool of exactly the volumes' sum, set in order, with set_voxels, voxels and
    integrate(list, imgs, K, poses) and, where image_format is given, set_colours, get_colours and integrate_colour(list, imgs, images,
    K, poses, image_format=...).  Random start words, frame lists whose order is not the pool order, and after every call: a listed
    volume holds what the host definition makes of its start words, an unlisted one keeps its words byte for byte."""
    from rgbd_odometry_amd import capi
    vols = PACKED_VOLUMES
    nv = len(vols)
    cvols = [capi.DvoTsdfVolume.make(v["dims"], v["voxel_size"], v["origin"], v["trunc"]) for v in vols]
    colour = image_format is not None

    def host(v, words, colours, imgs, pics, poses, frames):
        if colour:
            return capi.tsdf_integrate_colour_host(cvols[v], words, colours, [imgs[f] for f in frames], [pics[f] for f in frames], K4, poses[frames],
                                                   image_format=image_format)
        return capi.tsdf_integrate_host(cvols[v], words, [imgs[f] for f in frames], K4, poses[frames]), None

    def call(h, imgs, pics, poses, volumes, frames):
        if colour:
            h.integrate_colour(volumes, [imgs[f] for f in frames], [pics[f] for f in frames], K4, poses[frames], image_format=image_format)
        else:
            h.integrate(volumes, [imgs[f] for f in frames], K4, poses[frames])
        if hasattr(h, "stats"):
            assert h.stats() == (capi.DVO_TSDF_INTEGRATE_LAUNCHES, 1), "one launch and one synchronisation per call"

    def compare(h, state, cstate, listed, where):
        for v in range(nv):
            got = h.voxels(v)
            if v in listed:
                assert np.array_equal(got, state[v]), "listed volume %d differs from the host definition (%s): %d words" % (v, where, (got != state[v]).sum())
            else:
                assert np.array_equal(got, state[v]), "unlisted volume %d changed (%s): %d words" % (v, where, (got != state[v]).sum())
            if colour:
                got = h.get_colours(v)
                if v in listed:
                    assert np.array_equal(got, cstate[v]), "listed volume %d: colour words differ from the host definition (%s)" % (v, where)
                else:
                    assert np.array_equal(got, cstate[v]), "unlisted volume %d: colour words changed (%s)" % (v, where)

    for fmt in formats:
        imgs, poses = frame_list(fmt)
        pics = None
        if colour:
            import tsdf_colour_reference as cr
            pics = cr.images("random", image_format)
        rng = np.random.RandomState(seed)
        # 1. a pool of random words
        h = make_handle(vols)
        state = [random_pool_words(rng, voxels_of(v)) for v in vols]
        cstate = [random_pool_colours(rng, voxels_of(v)) for v in vols] if colour else [None] * nv
        for v in range(nv):
            h.set_voxels(v, state[v])
            if colour:
                h.set_colours(v, cstate[v])
        compare(h, state, cstate, (), "after the fill, " + fmt)
        # 2. - 5. the calls: twelve volumes in a shuffled order, the other eleven, volume 1 alone (the middle word of a group of three
        # volumes), volume 18 alone (one word in a group of its own), all of them
        order = [int(v) for v in rng.permutation(nv)]
        every = [int(v) for v in rng.permutation(nv)]
        assert order[:12] != sorted(order[:12]) and order[12:] != sorted(order[12:]) and every != sorted(every)
        for k, (name, listed) in enumerate((("shuffled", order[:12]), ("swapped", order[12:]), ("volume 1 alone", [1]), ("volume 18 alone", [18]),
                                            ("all", every))):
            queues = {v: [int(f) for f in rng.randint(0, len(imgs), size=rng.randint(1, 5))] for v in listed}
            queues[listed[0]] = [int(f) for f in rng.randint(0, len(imgs), size=4)]
            volumes, frames = round_robin(listed, queues)
            if k == 0:
                assert 24 <= len(volumes) <= 40 and set(volumes) == set(listed) and len(set(volumes)) < nv
                assert volumes[:len(listed)] == listed and volumes[len(listed)] in listed, "the frames of a volume are interleaved with the others'"
            call(h, imgs, pics, poses, volumes, frames)
            for v in listed:
                state[v], cstate[v] = host(v, state[v], cstate[v], imgs, pics, poses, queues[v])
            compare(h, state, cstate, set(listed), "%s, %s" % (name, fmt))
        if hasattr(h, "close"):
            h.close()
        # 6. from a cleared pool: PACKED_FRAMES into every volume
        h = make_handle(vols)
        assert all(not h.voxels(v).any() for v in range(nv)) and (not colour or all(not h.get_colours(v).any() for v in range(nv)))
        queues = {v: list(PACKED_FRAMES) for v in range(nv)}
        volumes, frames = round_robin(every, queues)
        call(h, imgs, pics, poses, volumes, frames)
        state, cstate = [list(s) for s in zip(*[host(v, None, None, imgs, pics, poses, queues[v]) for v in range(nv)])]
        compare(h, state, cstate, set(range(nv)), "from a cleared pool, " + fmt)
        assert all(seen_and_negative(w)[0] >= 1 for w in state), "every volume has a seen voxel"
        assert sum(seen_and_negative(w)[1] for w in state) >= 500, "the pool holds 500 seen voxels with a negative distance"
        assert not colour or all((np.asarray(c) >> np.uint64(48)).any() for c in cstate), "every volume has a coloured voxel"
        if hasattr(h, "close"):
            h.close()


class FakePool:
    """A handle restated in Python for check_packed_pool: one pool, the host definition applied per listed volume.  fault None: correct.
    "whole_groups": every touched group of four pool words is stored whole, with zeros in the words that are not the volume's own (seen
    where those are an unlisted neighbour's); "whole_colour_groups": the same with the colour words alone.  "no_wrap": a group's words all keep y and z of the group's first voxel, x stepping past
    the row's end.  "reversed": a volume's frames are applied in the reverse of their list order"""

    def __init__(self, volumes, colour=False, fault=None):
        from rgbd_odometry_amd import capi
        self.capi, self.vols, self.fault = capi, list(volumes), fault
        self.off, total = pool_offsets(self.vols)
        self.pool = np.zeros(total, np.uint32)
        self.cpool = np.zeros(total, np.uint64) if colour else None

    def _span(self, v):
        return slice(self.off[v], self.off[v] + voxels_of(self.vols[v]))

    def set_voxels(self, v, words):
        self.pool[self._span(v)] = np.asarray(words, np.uint32).reshape(-1)

    def voxels(self, v):
        return self.pool[self._span(v)].copy()

    def set_colours(self, v, colours):
        self.cpool[self._span(v)] = np.asarray(colours, np.uint64).reshape(-1)

    def get_colours(self, v):
        return self.cpool[self._span(v)].copy()

    def integrate(self, volumes, imgs, K, poses):
        self._run(volumes, imgs, None, None, K, poses)

    def integrate_colour(self, volumes, imgs, images, K, poses, image_format="bgr8"):
        self._run(volumes, imgs, images, image_format, K, poses)

    def _host(self, vol, words, colours, imgs, images, image_format, K, poses):
        cv = self.capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])
        if images is None:
            return self.capi.tsdf_integrate_host(cv, words, imgs, K, poses), None
        return self.capi.tsdf_integrate_colour_host(cv, words, colours, imgs, images, K, poses, image_format=image_format)

    def _run(self, volumes, imgs, images, image_format, K, poses):
        poses = np.asarray(poses, np.float64).reshape(-1, 12)
        listed = []
        for v in volumes:
            if v not in listed:
                listed.append(v)
        for v in listed:
            idx = [i for i, q in enumerate(volumes) if q == v]
            if self.fault == "reversed":
                idx = idx[::-1]
            vol, span = self.vols[v], self._span(v)
            args = ([imgs[i] for i in idx], None if images is None else [images[i] for i in idx], image_format, K, poses[idx])
            if self.fault == "no_wrap":
                nx, ny, nz = vol["dims"]
                i = np.arange(voxels_of(vol))
                first = np.maximum((self.off[v] + i) // GROUP * GROUP - self.off[v], 0)       # the group's first voxel of this volume
                cell = (first % nx + (i - first)) + (nx + GROUP - 1) * (first // nx)          # in a volume with rows long enough
                wide = dict(vol, dims=(nx + GROUP - 1, ny, nz))
                words = np.zeros(voxels_of(wide), np.uint32)
                words[cell] = self.pool[span]
                colours = None
                if images is not None:
                    colours = np.zeros(voxels_of(wide), np.uint64)
                    colours[cell] = self.cpool[span]
                words, colours = self._host(wide, words, colours, *args)
                words, colours = words[cell], None if colours is None else colours[cell]
            else:
                words, colours = self._host(vol, self.pool[span], None if images is None else self.cpool[span], *args)
            self.pool[span] = words
            if images is not None:
                self.cpool[span] = colours
        if self.fault in ("whole_groups", "whole_colour_groups"):
            theirs = np.ones(self.pool.size, bool)
            for v in listed:
                theirs[self._span(v)] = False
            for v in listed:
                lo, hi = self.off[v] // GROUP * GROUP, min(-(-self._span(v).stop // GROUP) * GROUP, self.pool.size)
                hit = np.zeros(self.pool.size, bool)
                hit[lo:hi] = True
                if self.fault == "whole_groups":
                    self.pool[hit & theirs] = 0
                if images is not None:
                    self.cpool[hit & theirs] = 0
