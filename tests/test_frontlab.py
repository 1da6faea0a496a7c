"""-m "not gpu": the batched multifrontal LU front by front (tests/frontlab) on the host simulator, against a float64 LAPACK
reference.  This proves the harness, the patterns, the tolerances and the coverage bookkeeping on a machine without a GPU;
tests/test_frontlab_gpu.py runs the same cases (and larger ones) through the product library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "frontlab"))
import cases as fl  # noqa: E402

SIM_CASES = [c for c in fl.CASES if c.sim]
_results = {}


@pytest.fixture(scope="module")
def sim():
    return fl.load("sim")


def result(sim, case):
    if case.name not in _results:
        _results[case.name] = fl.run_case(sim, case)
    return _results[case.name]


@pytest.mark.parametrize("case", SIM_CASES, ids=[c.name for c in SIM_CASES])
def test_front_case_matches_lapack(sim, case):
    res = result(sim, case)
    main = res["main"]
    assert fl.canary_failures(case, main) == []
    if case.tweak:
        # the simulator flags zero / non-finite pivots; element growth is measured by the device kernels only
        if case.tweak == "zero":
            assert main["flag"] & 1
        return
    assert main["flag"] == 0
    assert fl.accuracy_failures(case, main, fl.reference(case)) == []
    if case.repro:
        assert main["chunk"] == case.nb and res["chunked"]["passes"] > 1
        for key in ("S", "x"):
            assert fl.same_bits(res["chunked"][key], main[key]), "chunked run differs from the unchunked one"
            assert fl.same_bits(res["alone"][key][0], main[key][1]), "member 1 factored alone differs from the batch"


def test_case_list_covers_every_branch(sim):
    got = fl.coverage([(c, result(sim, c)["main"]) for c in SIM_CASES] +
                      [(c, result(sim, c)["chunked"]) for c in SIM_CASES if c.repro])
    assert sorted(fl.REQUIRED_SIM - got) == []


def test_coverage_notices_a_missing_case(sim):
    """The coverage check itself: without the w = 129 case the scalar pivot piece of one column and the 129-wide front
    are no longer reached."""
    keep = [c for c in SIM_CASES if c.name != "dense_w129_s33_wide"]
    got = fl.coverage([(c, result(sim, c)["main"]) for c in keep])
    assert "wide_w=129" not in got
    assert fl.REQUIRED_SIM - got


def test_reference_bounds_catch_a_perturbed_panel(sim):
    """A separator block off by 1e-9 in one entry (what a wrong panel entry does to the Schur update) fails the bound."""
    case = fl.BY_NAME["dense_w129_s33_wide"]
    res = result(sim, case)["main"]
    ref = fl.reference(case)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    bad["S"][0, 3, 5] += 1e-9
    assert fl.accuracy_failures(case, bad, ref)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    bad["x"][2, 0, 7] *= 1 + 1e-9
    assert fl.accuracy_failures(case, bad, ref)
