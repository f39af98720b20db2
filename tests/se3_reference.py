"""The SE(3) helpers of the pose update, restated in mpmath at 50 digits.  TEST INFRASTRUCTURE ONLY (CPU side: the generator of
tests/golden/se3_golden.npz and the one CPU test that regenerates it; nothing that runs on the GPU box imports this module).

Plain definitions, no series and no thresholds other than the reference's own:
  exp    R = I + (sin th/th) W + ((1 - cos th)/th^2) W^2,  t = V upsilon,  V = I + ((1 - cos th)/th^2) W + ((th - sin th)/th^3) W^2;
         for th < 1e-10 the reference's own definition V = R (Sophus::SE3d::exp, restated at oracle/dvo_oracle.cpp:496), which the
         device mirrors on purpose
  log    Sophus' atan form: unit quaternion of the matrix (Eigen::Quaterniond(R), normalised), th = 2 atan(|q.vec| / q.w) in
         (-pi, pi], omega = th q.vec/|q.vec|;  V^-1 = I - W/2 + c W^2,  c = (1 - th/(2 tan(th/2)))/th^2, c = 1/12 for |th| < 1e-10
  polar  U V^T of A = U S V^T from mpmath.svd_r
Matrices are lists of rows of mpf; every input is a double and enters exactly.
"""
import mpmath
from mpmath import mp, mpf

DPS = 50
SOPHUS_EPS = mpf("1e-10")


def _use_precision():
    mp.dps = DPS


def vec(x):
    _use_precision()
    return [mpf(float(v)) for v in x]


def mat(A):
    _use_precision()
    return [[mpf(float(A[i][j])) for j in range(3)] for i in range(3)]


def eye():
    return [[mpf(1 if i == j else 0) for j in range(3)] for i in range(3)]


def hat(w):
    z = mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def mmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def mvec(A, x):
    return [sum(A[i][k] * x[k] for k in range(3)) for i in range(3)]


def norm(x):
    return mp.sqrt(sum(v * v for v in x))


def _I_aW_bW2(w, a, b):
    W = hat(w)
    W2 = mmul(W, W)
    I = eye()
    return [[I[i][j] + a * W[i][j] + b * W2[i][j] for j in range(3)] for i in range(3)]


def so3_exp(omega):
    w = vec(omega)
    th = norm(w)
    if th == 0:
        return eye()
    return _I_aW_bW2(w, mp.sin(th) / th, (1 - mp.cos(th)) / (th * th))


def exp(psi):
    """psi = [upsilon(3), omega(3)] (doubles) -> (R, t) in mpf"""
    _use_precision()
    u, w = vec(psi[:3]), vec(psi[3:])
    th = norm(w)
    R = so3_exp(psi[3:])
    if th < SOPHUS_EPS:
        V = R
    else:
        V = _I_aW_bW2(w, (1 - mp.cos(th)) / (th * th), (th - mp.sin(th)) / (th * th * th))
    return R, mvec(V, u)


def quat_of_matrix(m):
    """Eigen::Quaterniond(R): (w, x, y, z), normalised like Sophus' setRotationMatrix does"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [mpf(0)] * 4
    if t > 0:
        t = mp.sqrt(t + 1)
        q[0] = t / 2
        t = 1 / (2 * t)
        q[1] = (m[2][1] - m[1][2]) * t
        q[2] = (m[0][2] - m[2][0]) * t
        q[3] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
        q[1 + i] = t / 2
        t = 1 / (2 * t)
        q[0] = (m[k][j] - m[j][k]) * t
        q[1 + j] = (m[j][i] + m[i][j]) * t
        q[1 + k] = (m[k][i] + m[i][k]) * t
    n = mp.sqrt(sum(v * v for v in q))
    return [v / n for v in q]


def log(R, t):
    """(R, t) doubles -> psi = [upsilon(3), omega(3)] in mpf"""
    _use_precision()
    q = quat_of_matrix(mat(R))
    tv = vec(t)
    n = norm(q[1:])
    w = q[0]
    if n == 0:
        k = 2 / w
    elif w == 0:
        k = mp.pi / n
    else:
        k = 2 * mp.atan(n / w) / n
    th = k * n
    om = [k * q[1], k * q[2], k * q[3]]
    if abs(th) < SOPHUS_EPS:
        c = mpf(1) / 12
    else:
        c = (1 - th / (2 * mp.tan(th / 2))) / (th * th)
    return mvec(_I_aW_bW2(om, mpf(-1) / 2, c), tv) + om


def singular_values(A):
    _use_precision()
    S = mp.svd_r(mp.matrix(mat(A)), compute_uv=False)
    return sorted((S[i] for i in range(3)), reverse=True)


def polar(A):
    """U V^T of the double matrix A, in mpf"""
    _use_precision()
    U, _, Vt = mp.svd_r(mp.matrix(mat(A)))
    P = U * Vt
    return [[P[i, j] for j in range(3)] for i in range(3)]


def to_double(x):
    """round an mpf / list / list of lists to double(s)"""
    if isinstance(x, list):
        return [to_double(v) for v in x]
    return float(x)


def max_abs_diff(got, want):
    """max |double - mpf| over matching (nested) lists, as an mpf"""
    if isinstance(want, list):
        return max(max_abs_diff(g, w) for g, w in zip(got, want))
    return abs(mpf(float(got)) - want)
