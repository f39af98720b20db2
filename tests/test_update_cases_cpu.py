"""tests/update_cases.py on the CPU: every case reaches, on the oracle's trace, the branch it exists for (the GPU tests assert the same
again before they run), and the arrangements the GPU paths need -- the 3 -> 2 pyramid whose level 3 stops early while level 2 still
runs, the 4-pair batch with early and full runs side by side -- hold on the oracle."""
import numpy as np
import pytest

import update_cases as uc


@pytest.mark.parametrize("case", uc.CASES, ids=[c.name for c in uc.CASES])
def test_case_reaches_its_branch(oracle, case):
    uc.assert_reaches_branch(oracle, case)


def test_table(oracle):
    uc.assert_table(oracle)
    names = {c.name for c in uc.CASES}
    for c in uc.CASES:
        assert c.branch and (c.base is None or c.base in names)
        assert set(c.overrides) <= {"beta", "precond_rot", "reg_lambda", "step_a", "step_b", "step_decay_after", "step_decay_offset",
                                    "trust_radius", "psi_norm_stop", "enable_rotationize"}
    touched = set().union(*(c.overrides for c in uc.CASES))
    assert touched == {"beta", "precond_rot", "reg_lambda", "step_a", "step_b", "step_decay_after", "step_decay_offset",
                       "trust_radius", "psi_norm_stop", "enable_rotationize"}
    assert {c.level for c in uc.in_place()} == {2, 3}


def test_a_perturbed_parameter_would_show(oracle):
    """the teeth of the comparison: the oracle itself, run with one parameter of a case put back to its default, gives other
    energies -- so an engine path that ignored the parameter cannot match bit for bit"""
    sc, lv = uc.scene(oracle)
    for name, drop in (("unclamped", "step_a"), ("unclamped-stop", "psi_norm_stop"), ("radius-0.05", "trust_radius"),
                       ("no-rotation", "precond_rot"), ("beta-0", "beta"), ("lambda-50", "reg_lambda"),
                       ("decay-2-1", "step_decay_after"), ("decay-2-1", "step_decay_offset"), ("step-b-0.02", "step_b")):
        c = uc.BY_NAME[name]
        ov = {k: v for k, v in c.overrides.items() if k != drop}
        L = lv[c.level]
        r = oracle.run_iterations(c.level, c.iters, c.xyz(oracle), L["dt"], L["gx"], L["gy"], L["rows"], L["cols"], sc.intrinsics,
                                  c.R0, c.t0, params=uc.params(oracle, ov))
        assert not np.array_equal(r["energy"], uc.reference(oracle, c)["energy"]), (name, drop)


def test_pyramid_level_3_stops_early_and_level_2_still_runs(oracle):
    ref = uc.pyramid_reference(oracle, uc.BY_NAME["unclamped-stop"])
    assert 2 <= ref["levels"][3]["iters_run"] < uc.ITERS
    assert ref["levels"][2]["iters_run"] >= 2 and np.count_nonzero(ref["levels"][2]["energy"]) == ref["levels"][2]["iters_run"]


def test_batch_has_early_and_full_runs(oracle):
    refs = uc.batch_references(oracle)
    assert len(refs) == 4
    assert len({r["energy"].tobytes() for _, _, r in refs}) == 4          # four different alignments


@pytest.mark.parametrize("name", sorted(uc.TRACKER_SETS))
def test_tracker_frames_reach_the_branch(oracle, name):
    uc.assert_tracker_reaches_branch(oracle, name)
