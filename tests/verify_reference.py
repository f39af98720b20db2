"""Depth verification of loop-closure candidates (include/dvo_amd.h: dvo_tracker_verify; kernel in dvo_tracker_verify.hip), restated in
numpy.  Every operation is an np.float32 array operation in the order the header gives: numpy has no fused multiply-add, so the
floats are IEEE's and the seven integer fields of a record have one value -- the tests compare for equality.

u, v and the visibility come from the CPU oracle's eval_points (as views_reference.compose takes them); the depth p2 of the warped
point is recomputed here from xyz, R.astype(float32) and t.astype(float32):  d = X - t;  p2 = (r[6] d0 + r[7] d1) + r[8] d2  with r the
column-major float pose, i.e. the third column of R.

Also here, because the CPU test (which checks the inputs) and the GPU test (which uses them) must agree on them: the fixed twist of the
perturbed pose and the 480 x 640 frames of the long list."""
import numpy as np

FIELDS = ("n_points", "n_visible", "n_depth", "n_agree", "n_front", "n_behind", "sum_abs_q4")
DEFAULTS = dict(tol_mm=25.0, tol_rel=0.02, min_depth_mm=1.0, max_depth_mm=65535.0)      # dvo_tracker_verify_params_default

# the perturbed pose of the parity test: (R, t) -> (R exp(W), t + DT).  A rotation of 0.08 rad about y moves a point 1.2 m off the axis
# by 96 mm in depth -- beyond the default tolerance (25 mm + 2 % of 2 m = 65 mm) on both sides of the image, inside it in the middle
TWIST_W = (0.01, -0.08, 0.02)
TWIST_T = (0.02, -0.01, 0.0)

# a list longer than one trip of the kernel's walk (4 points per lane x 512 lanes): full-resolution 480 x 640 frames, one level
LONG_ROWS, LONG_COLS, LONG_K = 480, 640, (525.0, 525.0, 319.5, 239.5)


def long_list_frames():
    from rgbd_odometry_amd.frame_gen import camera_frame
    return [camera_frame(41, LONG_ROWS, LONG_COLS, shift=(0, 0)), camera_frame(41, LONG_ROWS, LONG_COLS, shift=(1, -2))]


def rodrigues(w):
    th = np.linalg.norm(w)
    k = np.asarray(w, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def perturbed(R, t):
    return np.asarray(R, np.float64) @ rodrigues(TWIST_W), np.asarray(t, np.float64) + np.asarray(TWIST_T)


def residuals(oracle, level, xyz, depth_rm, K, R, t, min_depth_mm=DEFAULTS["min_depth_mm"], max_depth_mm=DEFAULTS["max_depth_mm"]):
    """per point of the list: (vis, has, r, d), float32 where they are floats.  depth_rm: (rows, cols) float32 millimetres"""
    f32 = np.float32
    depth_rm = np.asarray(depth_rm, f32)
    rows, cols = depth_rm.shape
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, bool), np.zeros(0, f32), np.zeros(0, f32)
    nothing = np.zeros(rows * cols, f32)                     # the projection does not look at the now level
    ev = oracle.eval_points(level, xyz, nothing, nothing, nothing, rows, cols, K, R, t)
    u, v = ev["reproj"][:, 0], ev["reproj"][:, 1]
    with np.errstate(invalid="ignore"):
        vis = (u >= 0) & (u < f32(cols)) & (v >= 0) & (v < f32(rows))                       # half-open, False for NaN
    assert np.array_equal(vis, ev["visible"] != 0)
    Rf, tf = np.asarray(R, np.float64).astype(f32), np.asarray(t, np.float64).astype(f32)
    d0, d1, d2 = xyz[:, 0] - tf[0], xyz[:, 1] - tf[1], xyz[:, 2] - tf[2]
    with np.errstate(invalid="ignore", over="ignore"):
        p2 = (Rf[0, 2] * d0 + Rf[1, 2] * d1) + Rf[2, 2] * d2
        px = np.where(vis, u, f32(0)).astype(np.int32)
        py = np.where(vis, v, f32(0)).astype(np.int32)
        d = depth_rm[py, px]                                  # an invisible point reads pixel (0, 0) and ignores it
        has = vis & (d > f32(min_depth_mm)) & (d <= f32(max_depth_mm))                      # False for NaN
        z_mm = p2 * f32(1000.0)
        r = z_mm - d
    assert p2.dtype == f32 and r.dtype == f32 and d.dtype == f32
    return vis, has, r, d


def verify(oracle, level, xyz, depth_rm, K, R, t, tol_mm=DEFAULTS["tol_mm"], tol_rel=DEFAULTS["tol_rel"],
           min_depth_mm=DEFAULTS["min_depth_mm"], max_depth_mm=DEFAULTS["max_depth_mm"]):
    """the record of dvo_tracker_verify for one candidate: dict of the seven integer FIELDS"""
    f32 = np.float32
    vis, has, r, d = residuals(oracle, level, xyz, depth_rm, K, R, t, min_depth_mm, max_depth_mm)
    with np.errstate(invalid="ignore", over="ignore"):
        tol = f32(tol_mm) + f32(tol_rel) * d                  # multiply, then add
        agree = has & (np.abs(r) <= tol)
        front = has & (r < -tol)
        behind = has & (r > tol)
    assert tol.dtype == f32
    q = (np.minimum(np.abs(r[agree]), f32(65535.0)) * f32(16.0)).astype(np.uint32)          # truncated
    return dict(n_points=len(vis), n_visible=int(vis.sum()), n_depth=int(has.sum()), n_agree=int(agree.sum()), n_front=int(front.sum()),
                n_behind=int(behind.sum()), sum_abs_q4=int(q.astype(np.uint64).sum()))


def depth_verdict(record, min_agree_ratio, max_front_ratio, min_depth_points):
    """dvo_amd::depthVerdict, spelled out"""
    return (record["n_depth"] >= min_depth_points and record["n_agree"] >= min_agree_ratio * record["n_depth"] and
            record["n_front"] <= max_front_ratio * record["n_depth"])
