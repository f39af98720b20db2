"""Alignment inputs whose FIRST energy sits on a float rounding boundary.  TEST INFRASTRUCTURE ONLY (CPU, seeded, exact).

The engine's energy is E = (float)sqrt(S), S the correctly rounded double of the exact sum of eps^2 (dvo_device_math.h: "the energy
without an order of summation").  The packed fused kernel adds eps^2 in its own order and certifies that no order could have given
another float; where the certificate refuses -- about N 2^-28 of the iterations -- one more sweep adds the residuals exactly.  A
suite of ordinary scenes never meets that transition.  This module builds it on purpose:

  * iteration 0 of a run starts at the caller's pose (the identity here) and reads the caller's DT image, so its residuals are the DT
    values of the pixels the reference points project to.  WHICH pixel a point reads is asked of the oracle (eval_points on an
    image that holds pixel indices): at the identity the points sit on pixel corners and float rounding decides;
  * a target float e and the midpoint m to its upper neighbour are chosen; M2 = m^2 is exact on the grid of 2^-68 (and a double);
  * the DT values are assigned so that the exact sum of c_p dt_p^2 (c_p = points reading pixel p, Python ints in units of 2^-68)
    lands within 2^28 units of T = M2 + k ulp_double(M2): the bulk is distance-like (sqrt(d2) 255/178.9), five pixels read by
    exactly one point each carry the fix-up -- a term of about half the gap, the largest float square that leaves at least 2^56
    units, one more that leaves 2^50..2^50+2^37, and two small terms a, b found by a scan that close the gap;
  * every DT value is a float in [2^-11, 2^12): the range of the exact limbs.

Two flavours of image.  "A" (free): a few thousand distinct DT values, arbitrary gradients -- 16-byte texels.  "B" (compact-form
friendly): at most 120 distinct values (every horizontal rank step fits +-127) and gx / gy = imageGradient(DT) in float32 with
reflect-101 borders, computed AFTER the fix-up: dvo_now_prepare's verification accepts it.

The expected energy is the definition itself, np.float32(math.sqrt(math.fsum(eps^2))) over the generator's own residuals: at
k = 0, +-1 the double rounding of S and of sqrt gives m exactly, a tie that narrows to even -- not "the side S is on".
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

GRID = 68                      # exact sums are Python ints in units of 2^-68
LAND = 1 << 28                 # the exact sum lands within this many units of its target
DEPTH_MM = 2000.0              # the reference plane: whole millimetres, so that 4-byte point lists validate
#: N wanted -> (rows, cols); every pixel is a reference edge (N = rows * cols: 768, 3072, 19200)
SHAPES = {700: (24, 32), 3000: (48, 64), 15000: (120, 160)}


def ks(N):
    return [0, 1, -1, 2, -2, 3, -3, 8, -8, 64, -64, N // 4, -(N // 4), 8 * N, -8 * N]


#: the committed case set: (N wanted, flavour, seed, which k).  Every (size, flavour) gets the whole list of k once; the teeth condition
#: (tests/test_energy_boundary_cpu.py) is met by weighting towards the largest size and |k| in {2, 3, 8}, where a sequential double sum
#: is wrong by more ulps than the target is away from the boundary
CASE_SET = [(n, fl, 0, None) for n in (700, 3000, 15000) for fl in "AB"] + \
           [(15000, fl, seed, (2, -2, 3, -3, 8, -8)) for fl in "AB" for seed in (1, 2)]


def sq_units(f) -> int:
    """f^2 of a float32 value in [2^-11, 2^12), exactly, in units of 2^-68"""
    m, e = math.frexp(float(f))
    mi = int(m * (1 << 24))
    assert mi * 2.0 ** (e - 24) == float(f) and 2 * e + 20 >= 0 and e <= 12, f
    return (mi * mi) << (2 * e + 20)


def _floor_root(x: int) -> int:
    """the largest r = (24-bit integer) 2^s with r^2 <= x: a float32 in units of 2^-34"""
    r = math.isqrt(x)
    s = max(r.bit_length() - 24, 0)
    r = (r >> s) << s
    assert (1 << 23) <= r < (1 << 46), x            # a float in [2^-11, 2^12)
    return r


def _next_root(r: int) -> int:
    s = max(r.bit_length() - 24, 0)
    return r + (1 << s)


def _close_gap(R: int):
    """five float32 values (in units of 2^-34) whose squares add to R within LAND units"""
    assert R >= 1 << 62, R
    out = []
    g = _floor_root(R // 2); out.append(g); R -= g * g
    g = _floor_root(R - (1 << 56)); out.append(g); R -= g * g
    assert (1 << 56) <= R < (1 << 59), R
    g = _floor_root(R - (1 << 50)); out.append(g); R -= g * g
    assert (1 << 50) <= R < (1 << 50) + (1 << 37), R
    best = None
    for b in range(1 << 23, (1 << 23) + 16384):      # b^2 = 2^46 + ...: steps of 2^24 units; a's own grid is ~2^28 units
        rest = R - b * b
        a = _floor_root(rest)
        for cand in (a, _next_root(a)):
            err = rest - cand * cand
            if best is None or abs(err) < abs(best[0]):
                best = (err, cand, b)
        if abs(best[0]) < (1 << 18):
            break
    err, a, b = best
    assert abs(err) <= LAND, err
    return out + [a, b], err


def image_gradient(dt, rows, cols):
    """imageGradient (SolveDVO.cpp:1063-1098) of a column-major float32 image: 0.5 * central differences, reflect-101 borders"""
    a = np.asarray(dt, np.float32).reshape(cols, rows).T
    px = np.pad(a, ((0, 0), (1, 1)), mode="reflect")
    py = np.pad(a, ((1, 1), (0, 0)), mode="reflect")
    gx = (np.float32(0.5) * (px[:, 2:] - px[:, :-2])).astype(np.float32)
    gy = (np.float32(0.5) * (py[2:, :] - py[:-2, :])).astype(np.float32)
    return np.ascontiguousarray(gx.T).ravel(), np.ascontiguousarray(gy.T).ravel()


def exact_sum_units(eps) -> int:
    """the exact sum of eps^2 (float32 residuals, zeros allowed) in units of 2^-68"""
    v, c = np.unique(np.asarray(eps, np.float32), return_counts=True)
    return sum(int(n) * sq_units(x) for x, n in zip(v.tolist(), c.tolist()) if x != 0.0)


def rounded_double(units: int) -> float:
    """the correctly rounded double of units 2^-68 (int / int division of Python rounds correctly)"""
    return units / (1 << GRID)


class Base:
    """one (size, flavour, seed): reference list, who reads which pixel, bulk image, target float"""

    def __init__(self, oracle, n_key, flavour, seed):
        rows, cols = SHAPES[n_key]
        self.n_key, self.flavour, self.seed = n_key, flavour, seed
        self.rows, self.cols = rows, cols
        fx = cols * 525.0 / 640.0                              # float32-exact for these sizes
        self.K = (fx, fx, (cols - 1) / 2.0, (rows - 1) / 2.0)
        assert all(float(np.float32(v)) == v for v in self.K)
        n = rows * cols
        self.edge = np.full(n, 255, np.int32)
        self.depth = np.full(n, DEPTH_MM, np.float32)
        self.xyz, _ = oracle.enlist_ref_points(0, self.edge, self.depth, rows, cols, self.K)
        self.N = len(self.xyz)
        assert self.N == n
        # which pixel does every point read at the identity?  The oracle says: an image of pixel indices (+1: index 0 is a pixel too)
        idx = np.arange(1, n + 1, dtype=np.float32)
        z = np.zeros(n, np.float32)
        ev = oracle.eval_points(0, self.xyz, idx, z, z, rows, cols, self.K, np.eye(3), np.zeros(3))
        self.vis = ev["visible"].astype(bool)
        self.pix = np.where(self.vis, ev["eps"].astype(np.int64) - 1, -1)
        assert self.vis.sum() > 0.9 * self.N and np.all(self.pix[self.vis] >= 0)
        count = np.bincount(self.pix[self.vis], minlength=n)
        # bulk: distance-like values of integer squared distances >= 1
        rng = np.random.default_rng([n_key, ord(flavour), seed])
        if flavour == "A":
            d2 = rng.integers(1, 3000, n)
            self.gx = rng.normal(0, 3, n).astype(np.float32)
            self.gy = rng.normal(0, 3, n).astype(np.float32)
        else:
            pal = np.sort(rng.choice(np.arange(1, 3000), 100, replace=False))
            d2 = pal[rng.integers(0, len(pal), n)]
            self.gx = self.gy = None                           # derived per case, after the fix-up
        self.dt = (np.sqrt(d2.astype(np.float64)) * (255.0 / 178.9)).astype(np.float32)
        # five pixels read by exactly one point, their readers spread over the point list (first / last workgroup shares, resident
        # and streamed parts of the list)
        single = np.flatnonzero(self.vis & (count[np.maximum(self.pix, 0)] == 1))
        self.fix_points = [int(single[int(q * (len(single) - 1))]) for q in (0.03, 0.3, 0.55, 0.8, 0.985)]
        self.fix_pix = [int(self.pix[i]) for i in self.fix_points]
        assert len(set(self.fix_pix)) == 5
        eps = self.residuals(self.dt)
        s_full = exact_sum_units(eps)
        eps[self.fix_points] = 0.0
        self.s_bulk = exact_sum_units(eps)
        # the target float: the one the plain image's energy rounds to; M2 = the squared midpoint to its upper neighbour
        self.e = np.float32(math.sqrt(rounded_double(s_full)))
        e_up = np.nextafter(self.e, np.float32(np.inf), dtype=np.float32)
        m = 0.5 * (float(self.e) + float(e_up))                # exact in double
        q = Fraction(m) ** 2 * (1 << GRID)
        assert q.denominator == 1
        self.M2 = int(q)
        assert float(self.M2) == self.M2                       # 50 bits: M2 is a double
        self.ulp = 1 << (self.M2.bit_length() - 53)            # ulp_double(M2) in units
        self.e_up = e_up

    def residuals(self, dt):
        """eps of iteration 0 at the identity from the pixel map (invisible points: 0, :429)"""
        return np.where(self.vis, np.asarray(dt, np.float32)[np.maximum(self.pix, 0)], np.float32(0)).astype(np.float32)


class Case:
    def __init__(self, base: Base, k: int):
        self.base, self.k = base, k
        self.rows, self.cols, self.K, self.N = base.rows, base.cols, base.K, base.N
        self.edge, self.depth, self.xyz = base.edge, base.depth, base.xyz
        self.target = base.M2 + k * base.ulp
        roots, err = _close_gap(self.target - base.s_bulk)
        dt = base.dt.copy()
        for p, r in zip(base.fix_pix, roots):
            dt[p] = np.float32(r * 2.0 ** -34)
            assert sq_units(dt[p]) == r * r
        self.dt = dt
        if base.flavour == "A":
            self.gx, self.gy = base.gx, base.gy
        else:
            self.gx, self.gy = image_gradient(dt, base.rows, base.cols)
            assert len(np.unique(dt)) <= 120
        assert np.all(dt >= np.float32(2.0 ** -11)) and np.all(dt < np.float32(4096.0))
        self.eps = base.residuals(dt)
        self.n_visible = int(base.vis.sum())
        self.sum_units = base.s_bulk + sum(r * r for r in roots)
        assert self.sum_units == self.target - err and abs(err) <= LAND
        # the definition, on the generator's own residuals
        self.S = math.fsum((self.eps.astype(np.float64) ** 2).tolist())
        self.expected = np.float32(math.sqrt(self.S))
        self.boundary = abs(k) <= base.N // 4                  # the certificate must refuse; |k| = 8N: it must not
        self.id = "%d%s%d_k%+d" % (base.n_key, base.flavour, base.seed, k)


_cache = {}


def cases(oracle):
    """the committed case set, generated once per process"""
    if "cases" not in _cache:
        out = []
        for n_key, fl, seed, which in CASE_SET:
            b = Base(oracle, n_key, fl, seed)
            out += [Case(b, k) for k in (ks(b.N) if which is None else which)]
        _cache["cases"] = out
    return _cache["cases"]


def reference(oracle, case: Case, iters: int):
    """the oracle's run from the identity, computed once per (case, iterations) and shared: callers do not modify it"""
    key = (case.id, iters)
    if key not in _cache:
        _cache[key] = oracle.run_iterations(0, iters, case.xyz, case.dt, case.gx, case.gy, case.rows, case.cols, case.K,
                                            np.eye(3), np.zeros(3))
    return _cache[key]


# ---- plain double sums of eps^2: what an engine WITHOUT the definition would compute ----------------------------------------
def plain_sums(eps):
    t = np.asarray(eps, np.float32).astype(np.float64) ** 2            # exact: 48-bit products
    seq = float(np.cumsum(t)[-1])                                      # one by one
    pad = np.concatenate([t, np.zeros(-len(t) % 64)]).reshape(-1, 64)
    lanes = np.cumsum(pad, axis=0)[-1]                                 # 64 lanes, each its stride one by one ...
    while len(lanes) > 1:
        lanes = lanes[0::2] + lanes[1::2]                              # ... then a tree
    n2 = 1 << max(len(t) - 1, 0).bit_length()
    pw = np.concatenate([t, np.zeros(n2 - len(t))])
    while len(pw) > 1:
        pw = pw[0::2] + pw[1::2]                                       # pairwise
    return dict(sequential=seq, strided=float(lanes[0]), pairwise=float(pw[0]))
