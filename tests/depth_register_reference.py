"""The definition of depth registration (include/dvo_amd.h, "depth registration"), restated in numpy from the text of the definition --
whole-image arrays, one np.minimum.at per footprint offset; nothing of the C++ builder's loops.

Per depth pixel (v, u) with raw value r, in IEEE double, in the order written:
  1. Z: uint16: r == 0 is no measurement, else Z = r / 1000.0; float32 metres: r finite and > 0, Z = r.
  2. project(a, b): X = ((a - cxd) Z) / fxd, Y = ((b - cyd) Z) / fyd; Xc = R00 X + R01 Y + R02 Z + tx (left to right); invalid unless
     Zc > 0; x = Xc / Zc, y = Yc / Zc; with Dc5 the forward distortion; uc = fxc x + cxc, vc = fyc y + cyc.
  3. centre (u, v) and corners (u - 0.5, v - 0.5), (u + 0.5, v + 0.5) at the pixel's own Z; dropped if one is invalid or a corner
     coordinate is not finite or >= 2^30 in magnitude.
  4. q = rint(Zc_centre * 1000.0); dropped unless 1 <= q <= 65535.
  5. x0 = ceil(min corner uc), x1 = min(ceil(max corner uc), x0 + SPLAT_MAX); rows likewise; clipped; half-open.
  6. out = min(out, q) over the footprint; untouched pixels are 0.

TEST INFRASTRUCTURE ONLY.  A rig is a dict: depth_shape (rows, cols), Kd4, Kc4, R (3, 3), t (3,), Dc5 (5 numbers or None), has_Dc5
(whether Dc5 is applied: by default whenever there is one; False with a Dc5 in place is the rig whose numbers are there and ignored)."""
import numpy as np

SPLAT_MAX = 8
EMPTY = np.uint32(0xFFFFFFFF)
TINY = (0.0004, 0.0005, 0.00049, 1e-40)          # metres, the case tiny; 1e-40 is a subnormal float
SHAPES = ((1, 1), (1, 300), (17, 15), (257, 1))   # depth geometries of the cases shape_*
MANY_SHAPE = (6, 8)                              # colour geometry of many_to_one
PILE_COLS, PILE_PX_M = 160, 32.0                 # the case pile_up: columns of its depth image, fx * tx in pixel metres


def rig(depth_shape, Kd4, Kc4, R=None, t=None, Dc5=None, has_Dc5=None):
    return dict(has_Dc5=(Dc5 is not None) if has_Dc5 is None else bool(has_Dc5 and Dc5 is not None),
                depth_shape=(int(depth_shape[0]), int(depth_shape[1])), Kd4=[float(v) for v in Kd4], Kc4=[float(v) for v in Kc4],
                R=np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3),
                t=np.zeros(3) if t is None else np.asarray(t, np.float64).reshape(3), Dc5=None if Dc5 is None else [float(v) for v in Dc5])


def rot(axis, angle):
    """rotation matrix about a coordinate axis ('x', 'y', 'z'), exact for angle = pi up to the rounding of cos and sin"""
    c, s = np.cos(angle), np.sin(angle)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


def project(g, a, b, Z):
    fxd, fyd, cxd, cyd = g["Kd4"]
    fxc, fyc, cxc, cyc = g["Kc4"]
    R, t = g["R"], g["t"]
    with np.errstate(all="ignore"):
        X = ((a - cxd) * Z) / fxd
        Y = ((b - cyd) * Z) / fyd
        Xc = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + t[0]
        Yc = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + t[1]
        Zc = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
        ok = Zc > 0
        x, y = Xc / Zc, Yc / Zc
        if g["has_Dc5"]:
            k1, k2, p1, p2, k3 = g["Dc5"]
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
            yd = y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
            x, y = xd, yd
        return fxc * x + cxc, fyc * y + cyc, Zc, ok


def steps(g, depth):
    """the definition's intermediate results, one entry per measurement (rule 1) in raster order of the depth image: what register()
    is made of, and what the conditions of tests/test_depth_register_cpu.py::test_cases_mean_something are computed from.
    index: flat index into the depth image; front / front_a / front_b: Zc > 0 at the centre and the two corners; ua, va, ub, vb: the
    corners' colour coordinates (whatever they came to); Zc: the centre's; q = rint(Zc * 1000) as a double; ok: the pixel writes
    (rules 2 to 4); x0, x1, y0, y1: the footprint before clipping, for the entries with ok only (0 elsewhere)"""
    d = np.asarray(depth)
    assert d.shape == g["depth_shape"]
    if d.dtype == np.uint16:
        valid = d != 0
        Z = d.astype(np.float64) / 1000.0
    else:
        Z = d.astype(np.float32).astype(np.float64)
        valid = np.isfinite(Z) & (Z > 0)
    v, u = np.mgrid[0:d.shape[0], 0:d.shape[1]]
    index = np.flatnonzero(valid.reshape(-1))
    v, u, Z = v[valid].astype(np.float64), u[valid].astype(np.float64), Z[valid]
    _, _, Zc, front = project(g, u, v, Z)
    ua, va, _, front_a = project(g, u - 0.5, v - 0.5, Z)
    ub, vb, _, front_b = project(g, u + 0.5, v + 0.5, Z)
    with np.errstate(all="ignore"):
        ok = front & front_a & front_b
        for c in (ua, va, ub, vb):
            ok &= np.isfinite(c) & (np.abs(c) < 2.0 ** 30)
        q = np.rint(Zc * 1000.0)
        ok &= (q >= 1) & (q <= 65535)
    box = {k: np.zeros(len(index), np.int64) for k in ("x0", "x1", "y0", "y1")}
    box["x0"][ok] = np.ceil(np.minimum(ua[ok], ub[ok])).astype(np.int64)
    box["x1"][ok] = np.minimum(np.ceil(np.maximum(ua[ok], ub[ok])).astype(np.int64), box["x0"][ok] + SPLAT_MAX)
    box["y0"][ok] = np.ceil(np.minimum(va[ok], vb[ok])).astype(np.int64)
    box["y1"][ok] = np.minimum(np.ceil(np.maximum(va[ok], vb[ok])).astype(np.int64), box["y0"][ok] + SPLAT_MAX)
    return dict(index=index, front=front, front_a=front_a, front_b=front_b, ua=ua, va=va, ub=ub, vb=vb, Zc=Zc, q=q, ok=ok, **box)


def writers(g, depth, rows, cols):
    """per colour pixel, the q of every depth pixel whose clipped footprint holds it, in raster order of the depth image:
    dict (y, x) -> list.  A plain loop over the footprints of steps(): for the small images the contention conditions look at"""
    s = steps(g, depth)
    out = {}
    for k in np.flatnonzero(s["ok"]):
        for y in range(max(int(s["y0"][k]), 0), min(int(s["y1"][k]), rows)):
            for x in range(max(int(s["x0"][k]), 0), min(int(s["x1"][k]), cols)):
                out.setdefault((y, x), []).append(int(s["q"][k]))
    return out


def register(g, depth, rows, cols):
    """(rows, cols) uint16 millimetres, 0 = hole"""
    s = steps(g, depth)
    ok = s["ok"]
    q = s["q"][ok].astype(np.uint32)
    x0, x1, y0, y1 = s["x0"][ok], s["x1"][ok], s["y0"][ok], s["y1"][ok]
    z = np.full(rows * cols, EMPTY, np.uint32)
    for dy in range(SPLAT_MAX):
        for dx in range(SPLAT_MAX):
            y, x = y0 + dy, x0 + dx
            m = (y < y1) & (x < x1) & (y >= 0) & (y < rows) & (x >= 0) & (x < cols)
            if m.any():
                np.minimum.at(z, y[m] * cols + x[m], q[m])
    return np.where(z == EMPTY, 0, z).astype(np.uint16).reshape(rows, cols)


def resample_nn(img, shape):
    """nearest-neighbour resampling of an image to another geometry (what makes a raw depth image of a rig out of a colour-sized one)"""
    r = (np.arange(shape[0]) * img.shape[0]) // shape[0]
    c = (np.arange(shape[1]) * img.shape[1]) // shape[1]
    return np.ascontiguousarray(img[r][:, c])


def colour_K(rows, cols):
    """a colour camera for a rows x cols image: focal length = cols pixels, principal point at the image centre"""
    return [float(cols), float(cols), (cols - 1) / 2.0, (rows - 1) / 2.0]


def scaled_K(K4, from_shape, to_shape):
    """the intrinsics of the same field of view sampled at another geometry (pixel centres at integers)"""
    sy, sx = to_shape[0] / from_shape[0], to_shape[1] / from_shape[1]
    return [K4[0] * sx, K4[1] * sy, (K4[2] + 0.5) * sx - 0.5, (K4[3] + 0.5) * sy - 0.5]


def box_scene(shape, back_mm=3000, box_mm=1000):
    """background plane with a foreground box in the middle third; (image, box mask)"""
    d = np.full(shape, back_mm, np.uint16)
    box = np.zeros(shape, bool)
    box[shape[0] // 3:2 * shape[0] // 3, shape[1] // 3:2 * shape[1] // 3] = True
    d[box] = box_mm
    return d, box


def ramp(shape, lo_mm=800, hi_mm=4000):
    v, u = np.mgrid[0:shape[0], 0:shape[1]]
    return (lo_mm + (hi_mm - lo_mm) * (u + 2 * v) / (shape[1] + 2 * shape[0])).astype(np.uint16)


def cases(rows, cols):
    """the cases of tests/test_depth_register_cpu.py for one colour geometry: list of (name, rig, raw depth image); uint16 images stand
    for their float32-metres twin as well (float32(d) / float32(1000)), float32 images are F32 only"""
    Kc = colour_K(rows, cols)
    rng = np.random.default_rng(rows * 1000 + cols)
    out = []
    ident = rng.integers(300, 6000, (rows, cols)).astype(np.uint16)
    ident[rng.random((rows, cols)) < 0.10] = 0
    out.append(("identity", rig((rows, cols), Kc, Kc), ident))
    for shape in ((60, 80), (96, 128)):
        out.append(("plane_%dx%d" % shape, rig(shape, scaled_K(Kc, (rows, cols), shape), Kc), np.full(shape, 1500, np.uint16)))
    out.append(("baseline_box", rig((rows, cols), Kc, Kc, t=[0.05, 0.0, 0.0]), box_scene((rows, cols))[0]))
    R = rot("z", 0.03) @ rot("y", 0.03) @ rot("x", -0.03)
    out.append(("rot_dist_ramp", rig((60, 80), scaled_K(Kc, (rows, cols), (60, 80)), Kc, R=R, t=[0.025, -0.01, 0.005],
                                    Dc5=[0.1, -0.05, 0.001, -0.002, 0.01]), ramp((60, 80))))
    four = np.zeros((7, 7), np.uint16)
    for v, u in ((2, 2), (2, 4), (4, 2), (4, 4)):
        four[v, u] = 2000
    out.append(("clamp_12x", rig((7, 7), [10.0, 10.0, 3.0, 3.0], [120.0, 120.0, cols / 2.0, rows / 2.0]), four))
    out.append(("behind", rig((rows, cols), Kc, Kc, R=np.diag([-1.0, 1.0, -1.0])), ramp((rows, cols))))
    special = (ramp((rows, cols)).astype(np.float32) / np.float32(1000.0))
    flat = special.reshape(-1)
    flat[0::7] = np.nan
    flat[1::11] = np.inf
    flat[2::13] = 0.0
    flat[3::17] = -1.5
    flat[4::19] = -np.inf
    out.append(("f32_specials", rig((rows, cols), Kc, Kc, t=[0.01, 0.0, 0.0]), special))
    far = np.full((rows, cols), 65535, np.uint16)
    far[::2] = 64000
    out.append(("q_beyond", rig((rows, cols), Kc, Kc, t=[0.0, 0.0, 1.0]), far))              # 65.535 m + 1 m is beyond 16 bits, 65 m is not
    out.append(("f32_far", rig((rows, cols), Kc, Kc), np.full((rows, cols), 70.0, np.float32)))
    out.append(("outside", rig((rows, cols), Kc, Kc, t=[5.0, 0.0, 0.0]), np.full((rows, cols), 1000, np.uint16)))
    out.append(("partly_outside", rig((rows, cols), Kc, Kc, t=[0.3, -0.2, 0.0]), ramp((rows, cols))))
    out.append(("all_zero", rig((60, 80), scaled_K(Kc, (rows, cols), (60, 80)), Kc, t=[0.05, 0.0, 0.0]), np.zeros((60, 80), np.uint16)))
    # rule 3, the limit: the principal point at a half-integer puts the corner of one pixel per row exactly on the optical axis (uc = cxc,
    # inside the image) while its other corner is fx / fxd = 2^38 / cols >= 2^31 pixels away -- beyond the range of int, where
    # (int)ceil(x) is no longer the same on every machine; the pixels further out have both corners there
    Kh = [float(cols), float(cols), (cols - 1) // 2 + 0.5, (rows - 1) // 2 + 0.5]
    out.append(("limit_corner_inside", rig((rows, cols), Kh, [2.0 ** 38] + Kh[1:]), ramp((rows, cols))))
    # rule 3, not finite: r2 * k3 overflows to an infinity (and 0 * inf to a NaN) for all but the rays next to the optical axis
    out.append(("not_finite", rig((rows, cols), Kc, Kc, t=[0.01, 0.0, 0.0], Dc5=[1.7e308, 1.7e308, 0.0, 0.0, 1.7e308]), ramp((rows, cols))))
    # rule 3, behind: the colour camera sits inside the scene and looks across the depth camera's view, so that its plane Zc = 0 cuts
    # through the surface: pixels behind it, pixels in front of it, and pixels with the centre in front and a corner behind.  Those
    # project far outside the image, all but a pixel that all but contains the camera's centre: the centre lies 0.5 m along the ray
    # through (us - 0.3, vs + 0.5) -- (-0.05, 0, 0.5) for 96 x 128 -- and pixel (vs, us) measures 2 mm more: its centre is 2 mm in
    # front of the camera's plane, its corner a behind it, and the two corners' coordinates, were both taken, span 8 x 8 pixels of
    # the image, at a depth of 2 mm that would win every minimum
    R = rot("y", -1.2)
    us, vs = int(round(Kc[2] - 0.1 * Kc[0] + 0.3)), int(round(Kc[3] - 0.5))
    centre = 0.5 * np.array([(us - 0.3 - Kc[2]) / Kc[0], (vs + 0.5 - Kc[3]) / Kc[1], 1.0])
    across = ramp((rows, cols), 450, 750)
    across[min(max(vs, 0), rows - 1), min(max(us, 0), cols - 1)] = 502
    out.append(("straddle", rig((rows, cols), Kc, Kc, R=R, t=-R @ centre), across))
    # rule 4: Zc * 1000 = (2 k + 1) * 62.5 exactly, every value a tie
    out.append(("ties", rig((rows, cols), Kc, Kc), np.resize((2 * np.arange(40) + 1) / 16.0, rows * cols).reshape(rows, cols).astype(np.float32)))
    # rule 4: q < 1.  0.0005f is a little above 0.0005 and rounds to 1, the others round to 0
    out.append(("tiny", rig((rows, cols), Kc, Kc), np.resize(np.repeat(np.array(TINY, np.float32), cols), rows * cols).reshape(rows, cols)))
    # rule 6 under contention: neighbours at unrelated depths, moved by a baseline of 1 to 16 pixels in both axes, land on one another
    out.append(("contended", rig((rows, cols), Kc, Kc, t=[0.05, 0.03, 0.0]), rng.integers(400, 6000, (rows, cols)).astype(np.uint16)))
    # rule 6 on one word: a depth camera with the colour camera's focal length and PILE_COLS columns, its principal point moved so that
    # its last column looks where the colour image's last column does, a baseline to the side, and in every row the hyperbola
    # Z(u) = fx tx / (x0 + PILE_COLS - cols - u) left of x0 = cols - 1 - (v mod 8): a surface that runs towards the colour camera's
    # centre, every pixel of a row one colour pixel wide and moved by its parallax onto the one colour pixel (v, x0).  Depth grows
    # with u, so the nearest writer of a word is the first in raster order
    piled = np.zeros((rows, PILE_COLS), np.uint16)
    for v in range(rows):
        steps_left = (cols - 1 - v % 8) + (PILE_COLS - cols) - np.arange(PILE_COLS)
        piled[v, steps_left >= 1] = np.rint(1000.0 * PILE_PX_M / steps_left[steps_left >= 1])
    out.append(("pile_up", rig((rows, PILE_COLS), [Kc[0], Kc[1], Kc[2] + PILE_COLS - cols, Kc[3]], Kc, t=[PILE_PX_M / Kc[0], 0.0, 0.0]), piled))
    # depth geometries of one pixel, one row, one column, less than a block: a plane, dense where the depth image is no coarser
    for shape in SHAPES:
        plane = np.full(shape, 1500, np.uint16)
        plane[rng.random(shape) < 0.05] = 0
        out.append(("shape_%dx%d" % shape, rig(shape, scaled_K(Kc, (rows, cols), shape), Kc), plane))
    # has_Dc5 = 0 with the numbers left in place: they are not applied
    name, g, d = next(c for c in out if c[0] == "rot_dist_ramp")
    out.append(("dc5_ignored", dict(g, has_Dc5=False), d))
    return out


def many_to_one(rows, cols, seed=0):
    """(rig, raw depth image) of a rows x cols depth camera registered into a colour image of MANY_SHAPE with the same field of view:
    the one case whose colour geometry is not (rows, cols).  A depth pixel is a small fraction of a colour pixel wide, and writes only
    where a colour pixel's corner lies between its own two corners"""
    Ks = colour_K(*MANY_SHAPE)
    rng = np.random.default_rng([rows, cols, seed])
    return rig((rows, cols), scaled_K(Ks, MANY_SHAPE, (rows, cols)), Ks, t=[0.01, 0.0, 0.0]), rng.integers(400, 6000, (rows, cols)).astype(np.uint16)


def all_cases(rows, cols):
    """cases(rows, cols) and many_to_one, each with its colour geometry: list of (name, rig, raw depth image, (rows, cols))"""
    g, d = many_to_one(rows, cols)
    return [(name, g_, d_, (rows, cols)) for name, g_, d_ in cases(rows, cols)] + [("many_to_one", g, d, MANY_SHAPE)]


def as_f32(depth):
    """the float32-metres twin of a uint16 image (holes stay 0)"""
    d = np.asarray(depth)
    return d if d.dtype == np.float32 else (d.astype(np.float32) / np.float32(1000.0))
