"""The front end of the frame-to-model alignment (include/dvo_amd.h, "preparing a depth frame") restated in numpy: the bilateral filter
and the now-frame normals of rgbd_odometry_amd/csrc/dvo_icp_prepare.h and the gated alignment of dvo_icp.h, written from their text --
float64 elementwise in the order written (numpy never fuses), one pass over the image per tap.  The gated alignment computes its own
association; the tree sum, the factorisation, the Cayley update, the record and the views are icp_reference's, by import.

Parameters are a dict(radius, range_scale, edge_max, range (256,) uint16, spatial (side, side) uint8): the weight tables are data."""
import math

import numpy as np

import icp_reference as ir
import tsdf_map_reference as tr

MAX_RADIUS, RANGE_BINS = 6, 256
#: the sizes of the filter cases: 5 x 13 (the window of radius 6 is larger than the image), then icp_reference.SIZES
FILTER_SIZES = [(5, 13)] + ir.SIZES
RADII = [0, 1, 3, 6]
DEFAULT = (3, 2.0, 0.03, 0.05)                    # radius, sigma_s in pixels, sigma_r in metres, edge_max in metres
#: the gate's settings in the tests: the cosine bound, and edge_max per size -- chosen so that the restatement shows pairs rejected by
#: the cosine test proper at the start pose of good_views at every size (asserted where they are used)
COS_MIN = 0.9
GATE_EDGE_MAX = {(24, 32): 0.05, (37, 53): 0.05, (72, 88): 0.05, (50, 82): 0.05}


def gaussian(radius, sigma_s, sigma_r, edge_max):
    """dvo_icp_prepare_params_gaussian by Python's math.exp (the library's tables are within one count of these)"""
    scale = 256.0 / (3.0 * sigma_r)
    rng = [int(np.rint(65535.0 * math.exp(-(((k + 0.5) / scale) ** 2) / (2.0 * sigma_r * sigma_r)))) for k in range(RANGE_BINS)]
    side = 2 * radius + 1
    sp = [[int(np.rint(255.0 * math.exp(-float(dx * dx + dy * dy) / (2.0 * sigma_s * sigma_s)))) for dx in range(-radius, radius + 1)]
          for dy in range(-radius, radius + 1)]
    return dict(radius=radius, range_scale=scale, edge_max=float(edge_max), range=np.array(rng, np.uint16), spatial=np.array(sp, np.uint8).reshape(side, side))


def from_c(p):
    """a DvoIcpPrepareParams as the restatement's dict"""
    side = 2 * p.radius + 1
    return dict(radius=int(p.radius), range_scale=float(p.range_scale), edge_max=float(p.edge_max), range=np.array(p.range[:], np.uint16),
                spatial=np.array(p.spatial[:side * side], np.uint8).reshape(side, side))


def shifted(a, dy, dx, fill):
    """b[v, u] = a[v + dy, u + dx], `fill` outside the image"""
    rows, cols = a.shape
    out = np.full_like(a, fill)
    v0, v1, u0, u1 = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(cols, cols - dx)
    if v0 < v1 and u0 < u1:
        out[v0:v1, u0:u1] = a[v0 + dy:v1 + dy, u0 + dx:u1 + dx]
    return out


def filter_image(depth, fp):
    """the filtered image: (rows, cols) float32 metres, 0 = a hole"""
    D, hole = tr.metres(depth)
    r, scale = fp["radius"], fp["range_scale"]
    rng = fp["range"].astype(np.uint64)
    num = np.zeros(D.shape, np.float64)
    den = np.zeros(D.shape, np.uint64)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                Dt, ht = shifted(D, dy, dx, 0.0), shifted(hole, dy, dx, True)
                k = np.abs(Dt - D) * scale
                ok = ~hole & ~ht & (k < 256.0)
                w = np.uint64(fp["spatial"][dy + r, dx + r]) * rng[np.where(ok, k, 0.0).astype(np.int64)]
                num = np.where(ok, num + w.astype(np.float64) * Dt, num)
                den = np.where(ok, den + w, den)
        assert int(den.max()) < 1 << 32
        out = (num / den.astype(np.float64)).astype(np.float32)
    return np.where(hole, np.float32(0.0), out)


def normals_image(F, K, edge_max):
    """the normals of a filtered image: (rows, cols, 3) float32 in the now camera's axes, (0, 0, 0) = none"""
    fx, fy, cx, cy = (float(k) for k in K)
    D, hole = tr.metres(np.asarray(F, np.float32))
    rows, cols = D.shape
    out = np.zeros((rows, cols, 3), np.float32)
    if rows < 3 or cols < 3:
        return out
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    inner = np.zeros((rows, cols), bool)
    inner[1:rows - 1, 1:cols - 1] = True

    def V(dy, dx):
        Ds = shifted(D, dy, dx, 0.0)
        return [((u + dx) - cx) / fx * Ds, ((v + dy) - cy) / fy * Ds, Ds]

    with np.errstate(all="ignore"):
        ok = inner & ~hole
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            ok &= ~shifted(hole, dy, dx, True) & (np.abs(shifted(D, dy, dx, 0.0) - D) <= edge_max)
        Vr, Vl, Vd, Vu = V(0, 1), V(0, -1), V(1, 0), V(-1, 0)
        a = [Vr[k] - Vl[k] for k in range(3)]
        b = [Vd[k] - Vu[k] for k in range(3)]
        G = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
        gg = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
        ok &= gg > 0.0
        length = np.sqrt(gg)
        for k in range(3):
            out[..., k] = np.where(ok, (G[k] / length).astype(np.float32), np.float32(0.0))
    return out


def prepare(depth, K, fp):
    F = filter_image(depth, fp)
    return F, normals_image(F, K, fp["edge_max"])


# ---- the gated alignment ----

def gated_terms(view, now_fmt, model_fmt, R, t, level, p, now_normals, cos_min):
    """(the (n, 28) entries of the sums, the (n,) validity, the (n,) mask of the pairs that pass every other test and have a now normal
    but fail c >= cos_min) of the level's list at the estimate; now_normals None: ungated"""
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
        has_normal = np.ones(len(uu), bool)
        cos_ok = np.ones(len(uu), bool)
        if now_normals is not None:
            g = np.asarray(now_normals, np.float32).astype(np.float64)
            nn = [g[vv, uu, k] for k in range(3)]
            has_normal = ~((nn[0] == 0.0) & (nn[1] == 0.0) & (nn[2] == 0.0))
            nw = [(R[k] * nn[0] + R[3 + k] * nn[1]) + R[6 + k] * nn[2] for k in range(3)]
            cos_ok = (n[0] * nw[0] + n[1] * nw[1]) + n[2] * nw[2] >= cos_min
        mc = [(um - cx) / fx * Dm, (vm - cy) / fy * Dm, Dm]
        M = [((Rm[k] * mc[0] + Rm[3 + k] * mc[1]) + Rm[6 + k] * mc[2]) + tm[k] for k in range(3)]
        d = [P[k] - M[k] for k in range(3)]
        ok &= ~((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > p["dist_max"] * p["dist_max"])
        by_cosine = ok & has_normal & ~cos_ok
        ok &= has_normal & cos_ok
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
    return out, ok, by_cosine


def align_view_gated(view, now_fmt, model_fmt, p, now_normals, cos_min):
    """(pose (12,), record dict) of one view under the gate; now_normals None: icp_reference.align_view's result"""
    R, t = [float(x) for x in view["start_pose"][:9]], [float(x) for x in view["start_pose"][9:]]
    iterations = 0

    def sweep(level):
        out, ok, _ = gated_terms(view, now_fmt, model_fmt, R, t, level, p, now_normals, cos_min)
        return ir.tree_sum(out), int(ok.sum())

    for level in range(p["levels"] - 1, -1, -1):
        for _ in range(p["iterations"][level]):
            sums, count = sweep(level)
            if count < p["min_count"]:
                return np.array(R + t), ir.record_of(ir.FEW, iterations, sums, count)
            x = ir.ldlt6(sums, p["min_pivot_ratio"])
            if x is None:
                return np.array(R + t), ir.record_of(ir.DEGENERATE, iterations, sums, count)
            R, t = ir.cayley_update(R, t, x)
            iterations += 1
            xx = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]
            if xx < p["stop_norm"] * p["stop_norm"]:
                break
    sums, count = sweep(0)
    return np.array(R + t), ir.record_of(ir.OK, iterations, sums, count)


# ---- inputs the CPU and GPU tests share ----

_cache = {}


def punched(Z, share, seed):
    rng = np.random.RandomState(9100 + seed)
    return np.where(rng.rand(*Z.shape) < share, 0.0, Z)


def filter_inputs(size, fmt):
    """five images of a size in one format: clean corner, corner with holes at a share of 0.08, all holes, the plane with holes and
    seeded noise of +-5 mm, and -- f32 only -- the corner with NaN, inf, negative and zero pixels (u16: a second holed corner)"""
    key = ("inputs", size, fmt)
    if key not in _cache:
        rows, cols = size
        K = ir.k4_for(rows, cols)
        Zc, _ = ir.raycast(ir.CORNER, K, ir.MODEL_POSES["front"], rows, cols)
        Zp, _ = ir.raycast(ir.PLANE, K, ir.MODEL_POSES["aside"], rows, cols)
        rng = np.random.RandomState(9000 + rows)
        noisy = np.where(Zp > 0.0, Zp + rng.uniform(-0.005, 0.005, Zp.shape), 0.0)
        Zs = [Zc, punched(Zc, 0.08, 1), np.zeros_like(Zc), punched(noisy, 0.08, 2), punched(Zc, 0.08, 3)]
        imgs = [ir.depth_images(Z)[0 if fmt == "u16" else 1] for Z in Zs]
        if fmt == "f32":
            bad = imgs[4].copy()
            flat = bad.reshape(-1)
            pick = rng.permutation(flat.size)[:max(4, flat.size // 10)]
            flat[pick] = np.resize(np.array([np.nan, np.inf, -np.inf, -1.25, 0.0, -0.0], np.float32), pick.size)
            imgs[4] = bad
        for a in imgs:
            a.setflags(write=False)
        _cache[key] = imgs
    return _cache[key]


def noisy_plane(size=(37, 53), seed=11):
    """(u16 image, K, the true normal in the camera's axes) of the slanted plane at 1 m with uniform noise of +-5 mm, seeded"""
    rows, cols = size
    K = ir.k4_for(rows, cols)
    Z, N = ir.raycast(ir.PLANE, K, ir.MODEL_POSES["front"], rows, cols)
    rng = np.random.RandomState(seed)
    mm = np.rint(Z * 1000.0 + rng.uniform(-5.0, 5.0, Z.shape))
    return mm.astype(np.uint16), K, np.asarray(ir.PLANE[0][1], np.float64)


def mean_angle_deg(normals, true):
    """the mean angle in degrees between the non-zero normals and `true` (a unit vector, or one per pixel)"""
    n = np.asarray(normals, np.float64)
    have = np.any(n != 0.0, axis=-1)
    c = np.clip((n * np.asarray(true, np.float64)).sum(axis=-1)[have], -1.0, 1.0)
    return float(np.degrees(np.arccos(c)).mean()), int(have.sum())


# ---- what filtering buys: measured, not assumed ----
# The mean angular error in degrees of the now-frame normals of noisy_plane() against the plane's true normal, computed by the HOST
# DEFINITION (dvo_icp_prepare_host): with radius 0 (the raw depth: the filter is the identity on a single tap) and with the default
# parameters, as printed by
#     python tests/icp_prepare_reference.py
# run from the repository root with the library built.  The test asserts filtered < raw and both values to 1e-9 degrees: the definition
# is IEEE double in a fixed order, so they repeat exactly on the host; the slack is for arccos and the mean in numpy.
#     raw: 1785 normals, filtered: 1785 normals (every inner pixel of 37 x 53)
MEASURED_NORMAL_ERRORS_DEG = dict(raw=7.079260337471, filtered=0.820023161698)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rgbd_odometry_amd import capi
    img, K, true = noisy_plane()
    for name, prm in (("raw", capi.DvoIcpPrepareParams.gaussian(0, 2.0, 0.03, 0.05)), ("filtered", capi.DvoIcpPrepareParams.default())):
        _, nrm = capi.icp_prepare_host([img], K, prm)
        print("%s: mean angular error %.12f degrees over %d normals" % ((name,) + mean_angle_deg(nrm[0], true)))
