"""Plain float64 numpy restatement of RGBDOdometry's photometric estimator (src/RGBDOdometry.cpp of the reference), written from
the reference's text and independent of oracle/dvo_oracle_photo.cpp, so that the oracle can be pinned to something other than its
own author's reading:

    computeJacobian        :407-508   photo_jacobian
    gaussNewtonIterations  :514-597   photo_gauss_newton
    computeEpsilon         :602-700   photo_epsilon
    exponentialMap         :713-746   exponential_map (to_se_3 :753-764)

Independent on purpose where the oracle restates a library: cv::filter2D is a 3x3 correlation over a BORDER_REFLECT_101 border
(any kernel, including a length-1 axis), the scan is the literal column-major loop with the :464 assert checked before every
pixel, T.inverse() and outTr.inverse() are general inverses (np.linalg.inv), and colPivHouseholderQr().solve() goes through
LAPACK's pivoted QR (scipy.linalg.qr(pivoting=True)).  Where results must be bit-identical to the oracle (selection, J, eps) the
expressions keep the reference's evaluation order; numpy evaluates them element-wise without contraction.

`fixed` applies the corrections the engine documents at dvo_photo_params (include/dvo_amd.h): D1 (:485), D2 (:490), D4 (level-0
intrinsics at every level, :475-476) and D7 (pure translation dropped, :727-731).  Depth is in sensor units (D5)."""
import numpy as np
import scipy.linalg

KERN_X = np.array([[0, 0, 0], [0, -1.0, 1.0], [0, 0, 0]])      # :423-425
KERN_Y = np.array([[0, 0, 0], [0, -1.0, 0], [0, 1.0, 0]])      # :426-428


class CapacityAssert(AssertionError):
    """`assert( xc < const_maxJacobianSize )` (:464) failed"""


class TextureAssert(AssertionError):
    """`assert( xc > const_minimumRequiredPts )` (:500) failed"""


def reflect101(p, n):
    """BORDER_REFLECT_101 index of p on an axis of length n (gfedcb|abcdefgh|gfedcba); a length-1 axis maps everything to 0"""
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    p = np.where(p < 0, -p, p)
    return np.where(p >= n, 2 * n - 2 - p, p)


def filter2d(img, kern):
    """cv::filter2D(img, dst, CV_64F, kern) with the anchor at the kernel's centre: a correlation, dst(i, j) = sum over the taps
    kern(a, b) * img(i + a - 1, j + b - 1), borders by reflection-101"""
    img = np.asarray(img, np.float64)
    rows, cols = img.shape
    ii, jj = np.arange(rows), np.arange(cols)
    out = np.zeros((rows, cols))
    for a in range(3):
        for b in range(3):
            if kern[a, b] != 0.0:
                out += kern[a, b] * img[np.ix_(reflect101(ii + a - 1, rows), reflect101(jj + b - 1, cols))]
    return out


def _intrinsics(K, level, fixed):
    fx, fy, cx, cy = (float(k) for k in K)
    if fixed:                                                   # D4: the level's own camera matrix
        s = 0.5 ** level
        fx, fy, cx, cy = fx * s, fy * s, cx * s, cy * s
    return fx, fy, cx, cy


def photo_jacobian(grey, depth, level, K, fixed=False, grad_threshold=5, capacity=50000, min_required=None):
    """computeJacobian (:407-508) of one level: grey u8 and depth (sensor units) as (rows, cols) arrays.  Returns the selected
    pixels (sel_i, sel_j) in scan order, J (n x 6) and A = J^T J (:379).  Raises CapacityAssert / TextureAssert where the reference
    asserts (:464; :500 only when min_required is given)."""
    egx, egy = filter2d(grey, KERN_X), filter2d(grey, KERN_Y)
    dep = np.asarray(depth, np.float64)
    rows, cols = egx.shape
    sel_i, sel_j = [], []
    xc = 0
    for j in range(cols):                                       # :460-462: j outer (Eigen's column-major order)
        for i in range(rows):
            if not xc < capacity:                               # :464, before every scanned pixel
                raise CapacityAssert("xc = %d at pixel (%d, %d)" % (xc, i, j))
            if egx[i, j] < float(grad_threshold):               # :467
                continue
            sel_i.append(i)
            sel_j.append(j)
            xc += 1
    if min_required is not None and not xc > min_required:
        raise TextureAssert("xc = %d" % xc)
    i, j = np.array(sel_i, np.int64), np.array(sel_j, np.int64)
    fx, fy, cx, cy = _intrinsics(K, level, fixed)
    Z = dep[i, j]
    X = Z * (i - cx) / fx                                       # :475 (the row index with cx, fx: D3)
    Y = Z * (j - cy) / fy                                       # :476
    invZ = 1 / Z
    invZ2 = 1 / (Z * Z)
    gx, gy = egx[i, j], egy[i, j]
    J = np.empty((xc, 6))
    J[:, 0] = fx * gx * invZ if fixed else fx * fx * invZ       # :485 (D1)
    J[:, 1] = fy * gy * invZ
    J[:, 2] = -fy * gy * Y * invZ2 - fx * gx * X * invZ2
    J[:, 3] = gy * (-fy * Y * Y * invZ2 - fy) - fx * gx * X * Y * invZ2
    J[:, 4] = gx * (fx * X * X * invZ2 + fx) + fx * gy * X * Y * invZ2
    J[:, 5] = (fy * gy * X * invZ - fx * gx * Y * invZ) if fixed else (fy * gy * X * invZ - fx * gy * Y * invZ)   # :490 (D2)
    return dict(sel_i=i, sel_j=j, J=J, A=J.T @ J, n=xc)


def photo_epsilon(grey_ref, depth_ref, grey_now, level, K, jac, T, fixed=False):
    """computeEpsilon (:602-700): eps of every selected pixel under T (4x4), |eps| (Eigen's norm()), and the warped points' depth
    out(2) for diagnostics"""
    fx, fy, cx, cy = _intrinsics(K, level, fixed)
    gr, gn = np.asarray(grey_ref, np.float64), np.asarray(grey_now)
    rows, cols = gn.shape
    i, j = jac["sel_i"], jac["sel_j"]
    Z = np.asarray(depth_ref, np.float64)[i, j]
    X = Z * (i - cx) / fx                                       # :660-662
    Y = Z * (j - cy) / fy
    Ti = np.linalg.inv(np.asarray(T, np.float64))               # T.inverse() :665
    out = Ti[:3, :3] @ np.vstack([X, Y, Z]) + Ti[:3, 3:4]       # Transform * Vector3d: linear part, then the translation
    with np.errstate(divide="ignore", invalid="ignore"):
        outu = out[0] * fx / out[2] + cx                        # :670
        outv = out[1] * fy / out[2] + cy                        # :671
        inside = (outu >= 0) & (outu < rows) & (outv >= 0) & (outv < cols)       # :683; NaN compares false
    eps = np.zeros(len(i))
    fu = np.floor(outu[inside]).astype(np.int64)
    fv = np.floor(outv[inside]).astype(np.int64)
    eps[inside] = gr[i[inside], j[inside]] - gn[fu, fv]        # :685
    return eps, float(np.sqrt(np.sum(eps * eps))), out[2]


def to_se_3(w):
    """:753-764"""
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exponential_map(psi, fixed=False):
    """exponentialMap (:713-746): psi = [t; w] -> 4x4.  |w| < 1e-12 gives the identity (D7), or [I t] with fixed."""
    psi = np.asarray(psi, np.float64)
    t, w = psi[:3], psi[3:]
    wx = to_se_3(w)
    theta = np.linalg.norm(w)
    out = np.eye(4)
    if theta < 1e-12:                                           # :727-731
        if fixed:
            out[:3, 3] = t
        return out
    I3 = np.eye(3)
    R = I3 + np.sin(theta) / theta * wx + (1.0 - np.cos(theta)) / (theta * theta) * wx @ wx
    V = I3 + (1 - np.cos(theta)) / (theta * theta) * wx + (theta - np.sin(theta)) / (theta * theta * theta) * wx @ wx
    out[:3, :3] = R
    out[:3, 3] = V @ t
    return out


def solve_colpiv_qr(A, b):
    """A.colPivHouseholderQr().solve(b): A P = Q R; pivots with |R_kk| <= eps * size * |R_00| (Eigen's default threshold) count
    as zero, and the components of x they would set are zero (the basic solution)"""
    A = np.asarray(A, np.float64)
    Q, R, P = scipy.linalg.qr(A, pivoting=True)
    d = np.abs(np.diag(R))
    thr = np.finfo(np.float64).eps * A.shape[0] * (d[0] if len(d) else 0.0)
    r = int(np.sum(d > thr)) if d[0] > 0 else 0
    x = np.zeros(A.shape[1])
    if r:
        x[P[:r]] = scipy.linalg.solve_triangular(R[:r, :r], (Q.T @ b)[:r])
    return x


def photo_gauss_newton(grey_ref, depth_ref, grey_now, level, K, jac, T, fixed=False, max_iters=3, eps_stop=200.0):
    """gaussNewtonIterations (:514-597) of one level (the reference: 3 iterations, :545).  Returns T, |eps| of every iteration
    (-1 where not run), the number of updates and eps of the first iteration."""
    T = np.array(T, np.float64)
    norms = np.full(max_iters, -1.0)
    updates, eps0 = 0, None
    for itr in range(max_iters):
        eps, nrm, _ = photo_epsilon(grey_ref, depth_ref, grey_now, level, K, jac, T, fixed)
        if eps0 is None:
            eps0 = eps
        norms[itr] = nrm
        if nrm < eps_stop:                                      # :556
            break
        b = -jac["J"].T @ eps                                   # :566
        psi = solve_colpiv_qr(jac["A"], b)                      # :568
        outTr = exponential_map(psi, fixed)                     # :575
        T = T @ np.linalg.inv(outTr)                            # :579
        updates += 1
    return T, norms, updates, eps0
