"""The boundary cases of tests/energy_boundary.py against the CPU oracle, and the condition that they have teeth.

Every case: the exact integer sum of the oracle's own residuals is the generator's; the oracle's first energy is the definition
np.float32(math.sqrt(math.fsum(eps^2))); the oracle's three limbs give math.fsum.

Teeth (a condition on the INPUTS, not on the engine): over the committed case set, a plain double sum of eps^2 -- one by one, 64
strided lanes then a tree, or pairwise -- gives another float than the definition in at least a quarter of the cases with
|k| <= N / 4.  Measured share of the committed set: 58 of 102 cases (0.57); by order: sequential 40, strided 22, pairwise 2.
"""
import math

import numpy as np

import energy_boundary as eb


def test_generated_sums_are_the_oracles(oracle):
    for c in eb.cases(oracle):
        ev = oracle.eval_points(0, c.xyz, c.dt, c.gx, c.gy, c.rows, c.cols, c.K, np.eye(3), np.zeros(3))
        assert np.array_equal(ev["eps"], c.eps) and int(ev["visible"].sum()) == c.n_visible, c.id
        assert eb.exact_sum_units(ev["eps"]) == c.sum_units, c.id
        assert abs(c.sum_units - c.target) <= eb.LAND, c.id
        assert eb.rounded_double(c.sum_units) == c.S, c.id                  # math.fsum is the correctly rounded exact sum
        lo, hi = np.float32(2.0 ** -11), np.float32(4096.0)
        assert np.all((c.dt >= lo) & (c.dt < hi)), c.id


def test_oracle_first_energy_is_the_definition(oracle):
    sides = set()
    for c in eb.cases(oracle):
        r = oracle.run_iterations(0, 1, c.xyz, c.dt, c.gx, c.gy, c.rows, c.cols, c.K, np.eye(3), np.zeros(3), trace=True)
        assert r["energy"][0] == c.expected, (c.id, r["energy"][0], c.expected)
        assert r["trace"][0]["sum_eps2"] == c.S and r["trace"][0]["n_visible"] == c.n_visible, c.id
        assert c.expected in (c.base.e, c.base.e_up), c.id                  # the two floats around the constructed midpoint
        sides.add((c.k > 0, c.expected == c.base.e_up))
        if abs(c.k) >= 2:                                                   # beyond the tie: the side S is on
            assert (c.expected == c.base.e_up) == (c.k > 0), c.id
    assert len(sides) >= 2


def test_oracle_limbs_give_fsum(oracle):
    for c in eb.cases(oracle):
        limbs = oracle.e2_limbs(c.eps)
        assert all(float(v).is_integer() and 0 <= v < 2.0 ** 53 for v in limbs), (c.id, limbs)
        assert int(limbs[0]) + (int(limbs[1]) << 32) + (int(limbs[2]) << 64) == c.sum_units, c.id
        assert oracle.e2_from_limbs(limbs) == c.S, c.id
        # shards add exactly, in any order (what the tiled path all-reduces)
        cut = [0, c.N // 3, c.N // 3 + 1, c.N]
        parts = [oracle.e2_limbs(c.eps[a:b]) for a, b in zip(cut[:-1], cut[1:])]
        assert oracle.e2_from_limbs(parts[2] + parts[0] + parts[1]) == c.S, c.id


def test_cases_have_teeth(oracle):
    """plain double sums must get a fair share of the boundary cases wrong, or bit-equality on them would prove nothing"""
    n = teeth = 0
    by_order = {}
    for c in eb.cases(oracle):
        if not c.boundary:
            continue
        n += 1
        wrong = [name for name, s in eb.plain_sums(c.eps).items() if np.float32(math.sqrt(s)) != c.expected]
        teeth += bool(wrong)
        for name in wrong:
            by_order[name] = by_order.get(name, 0) + 1
    print("teeth: %d of %d boundary cases (%.2f); by order: %s" % (teeth, n, teeth / n, sorted(by_order.items())))
    assert 4 * teeth >= n, (teeth, n)
