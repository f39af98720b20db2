"""Frame-to-model alignment (include/dvo_amd.h, "frame-to-model alignment") restated in numpy: the definition of
rgbd_odometry_amd/csrc/dvo_icp.h, written from its text -- float64 elementwise in the order written (numpy never fuses), the tree sum by
reshapes, the L D L^T factorisation and the Cayley update written out in Python floats -- plus the analytic scenes, views and sizes the
CPU and GPU tests share.  A view is a dict(now_u16, now_f32, model_u16, model_f32, normals, K, model_pose, start_pose, true_pose)."""
import numpy as np

import tsdf_map_reference as tr

OK, FEW, DEGENERATE = 0, 1, 2
#: 24 x 32; 37 x 53: partial 64-runs, odd sub-grids at levels 1 and 2; 72 x 88: 6336 pixels, more than 4096, so the tree has a third
#: round with two groups at level 0
SIZES = [(24, 32), (37, 53), (72, 88)]
#: the list lengths at which the sum tree and its kernels change: 64 entries (one run exactly, a single round), 65 (a second round with a
#: run of one), 4096 (one full sweep workgroup, no third round), 4100 (a second workgroup of four entries), 2^18 (64 workgroups: a full
#: third round, no fourth) and 2^18 + 1 (65 workgroups: the smallest fourth round, its last group one partial of one entry; level 1 is
#: 241 x 273 = 65,793 entries = 17 workgroups inside a pitch of 65).  Kept apart from SIZES: these run with TREE_SETTING only
TREE_SIZES = [(8, 8), (5, 13), (64, 64), (50, 82), (512, 512), (481, 545)]
TREE_SETTING = dict(levels=2, iterations=(2, 2))
#: the largest of them: beyond a VGA frame's 307,200 entries in what it exercises
TREE_TOP = TREE_SIZES[-1]
#: 524,900 entries = 129 sweep workgroups = three values in the fourth round (64, 64 and 1 workgroups): the smallest number at which the
#: ORDER of the fourth round shows -- at TREE_TOP it adds two values, and a + b has one order.  For the sum-order case alone
TREE_DEEP = (724, 725)
#: level 3 -- the last of DVO_ICP_MAX_LEVELS, lists of ceil(rows / 8) x ceil(cols / 8): (size, setting)
LEVEL3_CASES = [((37, 53), dict(levels=4, iterations=(3, 2, 2, 2))), ((72, 88), dict(levels=4, iterations=(3, 2, 2, 2))),
                (TREE_TOP, dict(levels=4, iterations=(1, 1, 1, 1)))]
DEFAULTS = dict(levels=3, iterations=(10, 5, 4, 0), z_near=0.1, z_far=8.0, dist_max=0.1, huber=0.0, stop_norm=0.0, min_pivot_ratio=1e-9,
                min_count=6)


def params(**changes):
    p = dict(DEFAULTS)
    for k, v in changes.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    p["iterations"] = tuple(p["iterations"]) + (0,) * (4 - len(p["iterations"]))
    return p


def k4_for(rows, cols):
    return (0.9 * cols, 0.9 * cols, (cols - 1) / 2.0, (rows - 1) / 2.0)


# ---- scenes: planes (a point, a unit normal towards the viewer's side), ray-cast exactly ----

def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


#: three mutually non-parallel planes around the camera's view: a back wall, a side wall and a floor, none of them axis-aligned
CORNER = [((0.0, 0.0, 1.2), _unit((0.05, 0.10, -1.0))),
          ((0.35, 0.0, 0.0), _unit((-1.0, 0.05, -0.10))),
          ((0.0, 0.25, 0.0), _unit((0.08, -1.0, -0.05)))]
#: one plane: the first three columns of every J are one vector
PLANE = [((0.0, 0.0, 1.0), _unit((0.10, -0.05, -1.0)))]
SCENES = dict(corner=CORNER, plane=PLANE)


def raycast(scene, K, pose, rows, cols):
    """(Z (rows, cols) float64 camera depth, 0 = no hit; normals (rows, cols, 3) float64 in world axes) of the scene seen from `pose`:
    per pixel the nearest plane the ray meets from its front"""
    fx, fy, cx, cy = K
    R = np.asarray(pose[:9], np.float64).reshape(3, 3).T
    t = np.asarray(pose[9:], np.float64)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ R.T
    Z = np.full((rows, cols), np.inf)
    N = np.zeros((rows, cols, 3))
    for p0, n in scene:
        denom = dirs @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            s = ((np.asarray(p0) - t) @ n) / denom
        hit = (denom < 0.0) & (s > 0.0) & (s < Z)
        Z = np.where(hit, s, Z)
        N[hit] = n
    none = ~np.isfinite(Z)
    Z[none] = 0.0
    N[none] = 0.0
    return Z, N


def depth_images(Z):
    """(u16 millimetres, f32 metres) of exact depths; 0 = a hole"""
    mm = np.rint(Z * 1000.0)
    mm[(mm < 1.0) | (mm > 65535.0)] = 0.0
    return mm.astype(np.uint16), Z.astype(np.float32)


#: the named small motions of the now camera against the model view: (rotation, translation) applied in the model camera's frame
MOTIONS = dict(shift=(np.eye(3), (0.020, -0.010, 0.015)),
               turn=(tr.rot(1, 0.020) @ tr.rot(0, -0.015), (0.0, 0.0, 0.0)),
               both=(tr.rot(2, 0.015) @ tr.rot(1, -0.012) @ tr.rot(0, 0.010), (-0.012, 0.010, -0.008)),
               inward=(np.eye(3), (-0.015, -0.012, 0.020)))
#: where the model views look from
MODEL_POSES = dict(front=tr.pose12(),
                   aside=tr.pose12(tr.rot(1, 0.08) @ tr.rot(0, -0.05), (-0.05, 0.03, 0.04)))


def compose(pose, R2, t2):
    """pose o (R2, t2): the motion applied in the pose's camera frame"""
    R = np.asarray(pose[:9]).reshape(3, 3).T
    return tr.pose12(R @ np.asarray(R2), R @ np.asarray(t2, np.float64) + np.asarray(pose[9:]))


def make_view(scene, size, model="front", motion="shift", holes=0.0, seed=0, zero_normals=None, all_holes=False):
    """one view: the scene ray-cast from the model pose (depth and normals) and from the now pose (depth), in both formats; the start
    pose is the model's.  holes: the share of pixels zeroed in the now and in the model depth; zero_normals: (row slice, column slice)
    of the model normals set to (0, 0, 0); all_holes: the now depth is all holes"""
    rows, cols = size
    K = k4_for(rows, cols)
    pm = MODEL_POSES[model]
    true = compose(pm, *MOTIONS[motion])
    Zm, Nm = raycast(SCENES[scene], K, pm, rows, cols)
    Zn, _ = raycast(SCENES[scene], K, true, rows, cols)
    rng = np.random.RandomState(7000 + seed)
    if holes > 0.0:
        Zm = np.where(rng.rand(rows, cols) < holes, 0.0, Zm)
        Zn = np.where(rng.rand(rows, cols) < holes, 0.0, Zn)
    if all_holes:
        Zn = np.zeros_like(Zn)
    Nm = np.where((Zm > 0.0)[..., None], Nm, 0.0).astype(np.float32)
    if zero_normals is not None:
        Nm[zero_normals[0], zero_normals[1]] = 0.0
    mu, mf = depth_images(Zm)
    nu, nf = depth_images(Zn)
    view = dict(scene=scene, rows=rows, cols=cols, K=K, model_pose=pm, start_pose=pm.copy(), true_pose=true, model_u16=mu, model_f32=mf,
                now_u16=nu, now_f32=nf, normals=np.ascontiguousarray(Nm))
    for a in view.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return view


_views = {}


def good_views(size):
    """the corner views of a size: clean, with holes punched into both depth images, and with holes and a block of zero normals"""
    key = ("good", size)
    if key not in _views:
        rows, cols = size
        block = (slice(rows // 3, rows // 3 + rows // 4), slice(cols // 4, cols // 4 + cols // 3))
        _views[key] = [make_view("corner", size, "front", "shift"),
                       make_view("corner", size, "aside", "turn", holes=0.08, seed=1),
                       make_view("corner", size, "front", "both", holes=0.04, seed=2, zero_normals=block)]
    return _views[key]


def stopping_views(size):
    """(the single plane: DEGENERATE, a now frame of nothing but holes: FEW)"""
    key = ("stopping", size)
    if key not in _views:
        _views[key] = [make_view("plane", size, "front", "shift"), make_view("corner", size, "front", "shift", all_holes=True)]
    return _views[key]


def tail_view(size):
    """the clean corner after the motion "inward": the now camera has moved left, up and forward, so what the bottom-right pixels of
    the now image see lies inside the model image.  The last entries of the list -- at TREE_SIZES the last run, the last sweep workgroup
    and the last group of the fourth round -- stay paired once the pose is near the true one; in good_views they leave the model image
    with the first updates and add zeros from then on"""
    key = ("tail", size)
    if key not in _views:
        _views[key] = make_view("corner", size, "front", "inward")
    return _views[key]


def wide_range_view(size=(24, 32), seed=5):
    """the sum-order case: the clean corner view with every model normal scaled by its own power of ten between 1e-6 and 1e6 (the
    definition never asks for unit normals), so the terms of a sweep span 24 decimal orders of magnitude"""
    key = ("wide", size, seed)
    if key not in _views:
        v = dict(make_view("corner", size, "front", "shift"))
        rng = np.random.RandomState(seed)
        scale = (10.0 ** rng.randint(-6, 7, size=size)).astype(np.float64)
        v["normals"] = np.ascontiguousarray((v["normals"].astype(np.float64) * scale[..., None]).astype(np.float32))
        v["normals"].setflags(write=False)
        _views[key] = v
    return _views[key]


def convergence_view():
    """the clean corner at 72 x 88 with the motion "both": its start pose is off in rotation and in translation"""
    if "convergence" not in _views:
        _views["convergence"] = make_view("corner", SIZES[2], "front", "both")
    return _views["convergence"]


def pose_errors(pose, true):
    """(rotation angle in radians, translation distance in metres) between two poses"""
    Ra, Rb = np.asarray(pose[:9]).reshape(3, 3).T, np.asarray(true[:9]).reshape(3, 3).T
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.arccos(min(1.0, max(-1.0, c)))), float(np.linalg.norm(np.asarray(pose[9:]) - np.asarray(true[9:])))


# ---- the restatement ----

def tree_sum(x):
    """the definition's sum of a list over axis 0: x (n, ...) float64"""
    x = np.asarray(x, np.float64)
    while True:
        pad = (-x.shape[0]) % 64
        if pad:
            x = np.concatenate([x, np.zeros((pad,) + x.shape[1:])])
        x = x.reshape((-1, 64) + x.shape[1:])
        for s in (32, 16, 8, 4, 2, 1):
            x = x[:, :s] + x[:, s:2 * s]
        x = x[:, 0]
        if x.shape[0] == 1:
            return x[0]


def raster_sum(x):
    """NOT the definition: the entries added one after the other in raster order"""
    return np.add.accumulate(np.asarray(x, np.float64), axis=0)[-1]


def grouped_sum(x):
    """NOT the definition: the tree inside each run of 4096 entries -- the first two rounds, one sweep workgroup -- and the results of
    the runs added one after the other: what a wrong association in the third or fourth round gives"""
    x = np.asarray(x, np.float64)
    parts = np.array([tree_sum(x[i:i + 4096]) for i in range(0, x.shape[0], 4096)])
    return np.add.accumulate(parts, axis=0)[-1]


def fourth_round_raster_sum(x):
    """NOT the definition: the tree inside each run of 2^18 entries -- three rounds -- and the results added one after the other: a
    fourth round in the wrong order.  It has the tree's bits up to 2^19 entries, where the fourth round adds at most two values"""
    x = np.asarray(x, np.float64)
    parts = np.array([tree_sum(x[i:i + (1 << 18)]) for i in range(0, x.shape[0], 1 << 18)])
    return np.add.accumulate(parts, axis=0)[-1]


def terms(view, now_fmt, model_fmt, R, t, level, p):
    """(the (n, 28) entries of the sums, the (n,) validity) of the level's list at the estimate (R column-major 9, t 3)"""
    rows, cols = view["rows"], view["cols"]
    fx, fy, cx, cy = (float(k) for k in view["K"])
    Rm, tm = [float(x) for x in view["model_pose"][:9]], [float(x) for x in view["model_pose"][9:]]
    R, t = [float(x) for x in R], [float(x) for x in t]
    step = 1 << level
    vv, uu = np.meshgrid(np.arange(0, rows, step), np.arange(0, cols, step), indexing="ij")
    vv, uu = vv.ravel(), uu.ravel()
    Dn, hole_n = tr.metres(view["now_" + now_fmt])
    Dmod, hole_m = tr.metres(view["model_" + model_fmt])
    nrm = view["normals"].astype(np.float64)
    with np.errstate(all="ignore"):
        D = Dn[vv, uu]
        ok = ~hole_n[vv, uu]
        ok &= ~(D <= p["z_near"]) & ~(D > p["z_far"])
        pc = [(uu.astype(np.float64) - cx) / fx * D, (vv.astype(np.float64) - cy) / fy * D, D]
        P = [((R[k] * pc[0] + R[3 + k] * pc[1]) + R[6 + k] * pc[2]) + t[k] for k in range(3)]
        e = [P[k] - tm[k] for k in range(3)]
        q = [(Rm[3 * k] * e[0] + Rm[3 * k + 1] * e[1]) + Rm[3 * k + 2] * e[2] for k in range(3)]
        ok &= q[2] > p["z_near"]
        um = np.floor((fx * (q[0] / q[2]) + cx) + 0.5)
        vm = np.floor((fy * (q[1] / q[2]) + cy) + 0.5)
        ok &= (um >= 0.0) & (um < float(cols)) & (vm >= 0.0) & (vm < float(rows))
        ui, vi = np.where(ok, um, 0.0).astype(np.int64), np.where(ok, vm, 0.0).astype(np.int64)
        Dm = Dmod[vi, ui]
        ok &= ~hole_m[vi, ui]
        n = [nrm[vi, ui, k] for k in range(3)]
        ok &= ~((n[0] == 0.0) & (n[1] == 0.0) & (n[2] == 0.0))
        mc = [(um - cx) / fx * Dm, (vm - cy) / fy * Dm, Dm]
        M = [((Rm[k] * mc[0] + Rm[3 + k] * mc[1]) + Rm[6 + k] * mc[2]) + tm[k] for k in range(3)]
        d = [P[k] - M[k] for k in range(3)]
        ok &= ~((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > p["dist_max"] * p["dist_max"])
        r = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
        ar = np.abs(r)
        wgt = np.ones_like(r) if p["huber"] <= 0.0 else np.where(ar <= p["huber"], 1.0, p["huber"] / ar)
        J = [n[0], n[1], n[2], P[1] * n[2] - P[2] * n[1], P[2] * n[0] - P[0] * n[2], P[0] * n[1] - P[1] * n[0]]
        out = np.zeros((len(uu), 28))
        at = 0
        for i in range(6):
            wJ = wgt * J[i]
            for j in range(i, 6):
                out[:, at] = wJ * J[j]
                at += 1
            out[:, 21 + i] = wJ * r
        out[:, 27] = r * r
    out[~ok] = 0.0
    return out, ok


def upper(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


def ldlt6(sums, min_pivot_ratio):
    """x of A x = -b by A = L D L^T in the header's order, in Python floats; None: a pivot failed"""
    s = [float(v) for v in sums]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        ajj = s[upper(j, j)]
        dj = ajj
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        if not dj > min_pivot_ratio * ajj:
            return None
        D[j] = dj
        for i in range(j + 1, 6):
            a = s[upper(j, i)]
            for k in range(j):
                a = a - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = a / dj
    y = [0.0] * 6
    for i in range(6):
        a = -s[21 + i]
        for k in range(i):
            a = a - L[i][k] * y[k]
        y[i] = a
    x = [0.0] * 6
    for i in range(5, -1, -1):
        a = y[i] / D[i]
        for k in range(i + 1, 6):
            a = a - L[k][i] * x[k]
        x[i] = a
    return x


def cayley_update(R, t, x):
    a0, a1, a2 = x[3] * 0.5, x[4] * 0.5, x[5] * 0.5
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    s = 2.0 / (1.0 + aa)
    Cm = [1.0 + s * (a0 * a0 - aa), s * (a0 * a1 - a2), s * (a0 * a2 + a1),
          s * (a1 * a0 + a2), 1.0 + s * (a1 * a1 - aa), s * (a1 * a2 - a0),
          s * (a2 * a0 - a1), s * (a2 * a1 + a0), 1.0 + s * (a2 * a2 - aa)]
    Rn = [0.0] * 9
    for j in range(3):
        for i in range(3):
            Rn[i + 3 * j] = (Cm[3 * i] * R[3 * j] + Cm[3 * i + 1] * R[3 * j + 1]) + Cm[3 * i + 2] * R[3 * j + 2]
    tn = [((Cm[3 * i] * t[0] + Cm[3 * i + 1] * t[1]) + Cm[3 * i + 2] * t[2]) + x[i] for i in range(3)]
    return Rn, tn


def record_of(status, iterations, sums, count):
    info = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            info[i, j] = sums[upper(min(i, j), max(i, j))]
    s2 = float(sums[27])
    return dict(status=status, iterations=iterations, count=int(count), sum_r2=s2, rms=float(np.sqrt(s2 / float(count))) if count > 0 else 0.0,
                info=info)


def align_view(view, now_fmt, model_fmt, p, total=tree_sum):
    """(pose (12,), record dict) of one view; `total`: how a list is summed (the definition: tree_sum)"""
    R, t = [float(x) for x in view["start_pose"][:9]], [float(x) for x in view["start_pose"][9:]]
    iterations = 0

    def sweep(level):
        out, ok = terms(view, now_fmt, model_fmt, R, t, level, p)
        return total(out), int(ok.sum())

    for level in range(p["levels"] - 1, -1, -1):
        for _ in range(p["iterations"][level]):
            sums, count = sweep(level)
            if count < p["min_count"]:
                return np.array(R + t), record_of(FEW, iterations, sums, count)
            x = ldlt6(sums, p["min_pivot_ratio"])
            if x is None:
                return np.array(R + t), record_of(DEGENERATE, iterations, sums, count)
            R, t = cayley_update(R, t, x)
            iterations += 1
            xx = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]
            if xx < p["stop_norm"] * p["stop_norm"]:
                break
    sums, count = sweep(0)
    return np.array(R + t), record_of(OK, iterations, sums, count)


# ---- the floor of the convergence test: measured, not assumed ----
# The final errors (rotation in radians, translation in metres) of the HOST DEFINITION (dvo_icp_align_host, default parameters) on
# convergence_view() started at the model's pose, as printed by
#     python tests/icp_reference.py
# run from the repository root with the library built.  The test's bound is twice the recorded value.  The floor is set by the
# projective association itself -- a now point is paired with the model point of the nearest of 72 x 88 pixels, not with its foot on the
# plane, so near the scene's edges pairs straddle two planes -- and, with U16 depth, by the millimetre quantisation of both images.
#     start errors: rotation 2.169779e-02 rad, translation 1.754993e-02 m
MEASURED_FINAL_ERRORS = dict(f32=(2.254446e-04, 1.725792e-04), u16=(2.345331e-04, 1.927872e-04))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rgbd_odometry_amd import capi
    v = convergence_view()
    print("start errors: rotation %.6e rad, translation %.6e m" % pose_errors(v["start_pose"], v["true_pose"]))
    for fmt in ("f32", "u16"):
        poses, rec = capi.icp_align_host([v["now_" + fmt]], [v["model_" + fmt]], [v["normals"]], v["K"], v["model_pose"][None], v["start_pose"][None])
        print("%s: rotation %.6e rad, translation %.6e m (status %d, %d updates, count %d, rms %.3e m)" %
              ((fmt,) + pose_errors(poses[0], v["true_pose"]) + (rec[0]["status"], rec[0]["iterations"], rec[0]["count"], rec[0]["rms"])))
