"""numpy composer of the multi-stream tracker's views (include/dvo_amd.h: dvo_tracker_set_views): the residue histogram and the two
BGR8 images a step renders for a stream, from what is known on the host -- the stream's reference points, its now level's distance
transform, the grey image of the frame that was fed and the pose the step returned.

compose_views works from reprojections (u, v): the half-open visibility rule the oracle pins (oracle/dvo_oracle.cpp:320), pixel =
(int)u, (int)v, d = DT(py, px).  compose() takes the reprojections from the CPU oracle's eval_points and checks that the oracle's own
visibility flags and residuals are the ones compose_views derives."""
import numpy as np

HIST_BINS = 260


def jet(i):
    """(B, G, R) of entry i of the 64-entry jet map (FColorMap), closed form"""
    r = lambda j: 0 if j <= 0 else min(255, 16 * j - 1)
    return min(r(i + 9), r(39 - i)), min(r(i - 7), r(55 - i)), min(r(i - 23), r(71 - i))


JET = np.array([jet(i) for i in range(64)], np.uint8)


def grey3(g):
    return np.repeat(np.asarray(g, np.uint8)[..., None], 3, 2)


def dt_background(dt_cm, rows, cols):
    """convertTo(CV_8UC1) of the column-major float distance transform: round half to even, saturate; (rows, cols) uint8"""
    DT = np.asarray(dt_cm, np.float32).reshape(cols, rows).T
    return np.clip(np.rint(DT), 0, 255).astype(np.uint8)


def compose_views(u, v, dt_cm, grey_rm, rows, cols):
    """u, v: float32 reprojections of every point of the list.  Returns dict(hist, reproj, heat, visible, eps, marked)"""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    DT = np.asarray(dt_cm, np.float32).reshape(cols, rows).T
    with np.errstate(invalid="ignore"):
        vis = (u >= 0) & (u < np.float32(cols)) & (v >= 0) & (v < np.float32(rows))          # False for NaN
    px, py = u[vis].astype(np.int32), v[vis].astype(np.int32)
    d = DT[py, px]
    eps = np.zeros(len(u), np.float32)                        # an invisible point's residual stays 0 (getReprojectedEpsilons)
    eps[vis] = d
    hist = np.bincount(np.clip(eps.astype(np.int32) + 1, 0, HIST_BINS - 1), minlength=HIST_BINS).astype(np.uint32)
    reproj = grey3(dt_background(dt_cm, rows, cols))
    reproj[py, px] = (0, 255, 0)
    heat = grey3(np.asarray(grey_rm, np.uint8).reshape(rows, cols))
    heat[py, px] = JET[np.where(d > np.float32(60.0), 63, np.clip(d.astype(np.int32), 0, 63))]
    marked = np.zeros((rows, cols), bool)
    marked[py, px] = True
    return dict(hist=hist, reproj=reproj, heat=heat, visible=vis, eps=eps, marked=marked)


def compose(oracle, level, xyz, dt_cm, gx_cm, gy_cm, grey_rm, rows, cols, K, R, t):
    """the views of one stream at pose (R, t): reprojections from the oracle, whose visibility and residuals must be compose_views'"""
    ev = oracle.eval_points(level, xyz, dt_cm, gx_cm, gy_cm, rows, cols, K, R, t)
    out = compose_views(ev["reproj"][:, 0], ev["reproj"][:, 1], dt_cm, grey_rm, rows, cols)
    assert np.array_equal(out["visible"], ev["visible"] != 0)
    assert np.array_equal(out["eps"], ev["eps"])
    return out


def unmarked(dt_cm, grey_rm, rows, cols):
    """the views of a stream on its first frame: plain backgrounds"""
    return grey3(dt_background(dt_cm, rows, cols)), grey3(np.asarray(grey_rm, np.uint8).reshape(rows, cols))
