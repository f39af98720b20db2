"""Inputs of the tracker's form tests (tests/test_gpu_tracker_forms.py, pinned without a GPU by tests/test_tracker_forms_cpu.py):

the wide world -- 50 x 1282 frames with texture in the left quarter and a flat wall to the right, whose level 0 has a pixel farther
from every edge than the 512 px the compact now form ranks (a partial form with real texels) and whose level 1 (25 x 641) does not (a
complete form), both with rows that are no multiple of 6 and columns that are no multiple of 4;

the square -- a bright square on constant grey at constant depth, whose reference lists are shorter than one wave on the coarse levels;

the pose sweep -- poses from the identity to one where nothing is visible, with reprojections on all four borders of the level.

numpy and the CPU oracle only."""
import numpy as np

import frame_gen
import frame_reference as fr

WIDE = dict(rows=50, cols=1282, nl=2, shift=0)
WIDE_K = (262.5, 262.5, 640.75, 24.75)
WIDE_SHIFTS = [(0, 0), (1, -1), (1, -2)]
WIDE_SEED, WIDE_TEXTURE_COLS = 5, 322
SQUARE = dict(rows=240, cols=320, nl=3, shift=0)             # the geometry of tests/test_gpu_tracker_information.py
SQUARE_K = (262.5, 262.5, 159.75, 119.75)
SQUARE_N = (92, 44, 20)                                       # reference points per level of square_frame((0, 0))
P4_RANK_REACH = 512                                           # px: distances the presence bitmap of the compact form ranks
P4_PARTIAL_RANKS = 4094                                       # distinct distances a partial compact form keeps: the lowest ones


def wide_frame(shift):
    bgr, depth = frame_gen.camera_frame(WIDE_SEED, WIDE["rows"], WIDE["cols"], shift=shift, holes=True)
    bgr[:, WIDE_TEXTURE_COLS:] = 128
    return bgr, depth


def wide_sequences():
    """two streams: the same three frames, stream 1 one shift ahead"""
    frames = [wide_frame(s) for s in WIDE_SHIFTS]
    return [frames, frames[1:] + frames[:1]]


def square_frame(shift=(0, 0)):
    g = SQUARE
    bgr = np.full((g["rows"], g["cols"], 3), 100, np.uint8)
    bgr[100 + shift[0]:124 + shift[0], 150 + shift[1]:174 + shift[1]] = 230
    return bgr, np.full((g["rows"], g["cols"]), 2.0, np.float32)


def square_sequence():
    return [square_frame((i, i)) for i in range(3)]


def level_dims(geom, level):
    return fr.level_size(geom["rows"], geom["shift"] + level), fr.level_size(geom["cols"], geom["shift"] + level)


def oracle_levels(oracle, frame, geom, K):
    """per level dict(xyz, dt, gx, gy, edge, rows, cols) of a camera frame as reference AND as now frame, from the CPU oracle"""
    Kf = tuple(np.float32(k) for k in K)
    out = []
    for l, (g, d) in enumerate(oracle.build_pyramid(frame[0], frame[1], n_levels=geom["nl"], first_shift=geom["shift"])):
        xyz = oracle.ref_level_from_grey(l, g, d, Kf)[0]
        dt, gx, gy, edge = oracle.now_level_from_grey(g)
        out.append(dict(xyz=xyz, dt=dt, gx=gx, gy=gy, edge=edge, rows=g.shape[0], cols=g.shape[1]))
    return out


def farthest_from_edges(edge_cm, rows, cols):
    """the largest distance (px) of a pixel from its nearest edge pixel: exact, squared distances in integers"""
    E = np.asarray(edge_cm).reshape(cols, rows).T != 0
    assert E.any()
    big = 4 * (rows + cols) ** 2
    yy = np.arange(rows)
    dy2 = np.where(E[None, :, :], (yy[:, None, None] - yy[None, :, None]) ** 2, big).min(1)       # (rows, cols): within the column
    xx = np.arange(cols)
    dx2 = (xx[:, None] - xx[None, :]) ** 2
    return float(np.sqrt(max(int((dx2 + dy2[y][None, :]).min(1).max()) for y in range(rows))))


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) if axis == "y" else np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


ALL_INVISIBLE = ("t = (100, 0, 0)", np.eye(3), np.array([100.0, 0.0, 0.0]))


def fixed_sweep():
    out = [("identity", np.eye(3), np.zeros(3))]
    for axis in "yx":
        for a in (0.05, 0.2, 0.4):
            for sgn in (1, -1):
                out.append(("%s %+.2f" % (axis, sgn * a), rot(axis, sgn * a), np.zeros(3)))
    return out + [ALL_INVISIBLE]


def sides_hit(ev, rows, cols):
    """which borders of the level the visible reprojections of one oracle.eval_points touch: {side: count}"""
    vis = ev["visible"] != 0
    u, v = np.floor(ev["reproj"][vis, 0]), np.floor(ev["reproj"][vis, 1])
    return dict(first_row=int((v == 0).sum()), last_row=int((v == rows - 1).sum()), first_col=int((u == 0).sum()),
                last_col=int((u == cols - 1).sum()))


def far_guesses():
    """match guesses that turn the wide world's points from the textured quarter onto the flat wall, more than two hundred pixels
    from the nearest edge: distances a partial compact form does not rank"""
    return np.stack([rot("y", -0.8), rot("y", -1.0)]), np.zeros((2, 3))


def unranked_hits(oracle, level, xyz, now, rows, cols, K, R, t, margin=64):
    """how many visible reprojections at (R, t) land on pixels whose distance is beyond the P4_PARTIAL_RANKS lowest distinct values of
    the level (by `margin` ranks at least): the pixels a partial compact form leaves to the 16-byte texels"""
    ev = oracle.eval_points(level, xyz, now[0], now[1], now[2], rows, cols, K, R, t)
    vis = ev["visible"] != 0
    px, py = ev["reproj"][vis, 0].astype(np.int64), ev["reproj"][vis, 1].astype(np.int64)
    dt = np.asarray(now[0], np.float32)
    rank = np.searchsorted(np.unique(dt), dt[py + px * rows])
    return int((rank >= P4_PARTIAL_RANKS + margin).sum())


def sweep(oracle, level, xyz, now, rows, cols, K):
    """the fixed sweep, then for every border no pose of it reaches, a rotation aimed at it: the point nearest the image centre in the
    other coordinate is turned onto the middle of a border pixel (about y for a column, about x for a row), the next point is tried
    if the oracle does not see it there.  Returns (poses, report): report[name] = dict(visible, sides), with the last pose the
    all-invisible one; conditions() judges it"""
    s = np.float32(2.0) ** -level
    fx, fy, cx, cy = (float(np.float32(k) * s) for k in K)
    look = lambda R, t: oracle.eval_points(level, xyz, now[0], now[1], now[2], rows, cols, K, R, t)
    poses, report = fixed_sweep(), {}
    for name, R, t in poses:
        ev = look(R, t)
        report[name] = dict(visible=int((ev["visible"] != 0).sum()), sides=sides_hit(ev, rows, cols))
    at = look(np.eye(3), np.zeros(3))["reproj"]
    P = np.asarray(xyz, np.float64).reshape(-1, 3)
    aimed = []
    for side in ("first_row", "last_row", "first_col", "last_col"):
        if any(r["sides"][side] for r in report.values()):
            continue
        col = side.endswith("col")
        order = np.argsort(np.abs(at[:, 1] - rows / 2.0) if col else np.abs(at[:, 0] - cols / 2.0), kind="stable")
        for i in order[:32]:
            x, y, z = P[i]
            if col:
                a = np.arctan2(x, z) - np.arctan(((0.5 if side == "first_col" else cols - 0.5) - cx) / fx)
                R = rot("y", a)
            else:
                a = np.arctan(((0.5 if side == "first_row" else rows - 0.5) - cy) / fy) - np.arctan2(y, z)
                R = rot("x", a)
            ev = look(R, np.zeros(3))
            if sides_hit(ev, rows, cols)[side]:
                name = "%s aimed at %s" % ("y" if col else "x", side)
                aimed.append((name, R, np.zeros(3)))
                report[name] = dict(visible=int((ev["visible"] != 0).sum()), sides=sides_hit(ev, rows, cols))
                break
    poses = poses[:-1] + aimed + poses[-1:]
    return poses, report


def conditions(poses, report, n_points):
    """(a) the last pose sees nothing, (b) some pose sees between 10 % and 90 % of the points, (c) every border is reached"""
    a = report[poses[-1][0]]["visible"] == 0
    b = any(0.1 * n_points <= r["visible"] <= 0.9 * n_points for r in report.values())
    c = all(any(r["sides"][side] for r in report.values()) for side in ("first_row", "last_row", "first_col", "last_col"))
    return a, b, c
