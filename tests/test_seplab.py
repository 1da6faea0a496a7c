"""-m "not gpu": the separator-side, vector and table launchers one by one (tests/seplab) on the host simulator, against the
numpy references of the lab.  This proves the harness, the references, the canaries, the bounds and the coverage bookkeeping
on a machine without a GPU; tests/test_seplab_gpu.py runs the same cases through the product library."""
import importlib.util
import os
import sys

import numpy as np
import pytest

LAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seplab")


def _load(name):
    """tests/seplab/<name>.py as module seplab_<name> (tests/frontlab has modules of the same file names)."""
    key = "seplab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


sl = _load("cases")

SIM_CASES = [c for c in sl.CASES if c.sim]
_results = {}


@pytest.fixture(scope="module")
def sim():
    return sl.load("sim")


def result(sim, case):
    if case.name not in _results:
        _results[case.name] = sl.run_case(sim, case)
    return _results[case.name]


def copy_of(res):
    return {k: v.copy() for k, v in res.items()}


@pytest.mark.parametrize("case", SIM_CASES, ids=[c.name for c in SIM_CASES])
def test_case_matches_reference(sim, case):
    fails, ratio = sl.check_case(case, result(sim, case))
    print("seplab sim: %-28s error / bound %.3g" % (case.name, ratio))
    assert fails == []


def test_test_vectors_are_clear_of_the_identity_threshold():
    bad = [m for c in sl.CASES if c.family == "householder" for m in sl.tv_rule_failures(c)]
    assert bad == []


def test_case_list_covers_every_branch(sim):
    got = sl.coverage(sim, SIM_CASES)
    assert sorted(sl.REQUIRED_SIM - got) == []


def test_coverage_notices_a_missing_case(sim):
    """The coverage check itself: without the 64 x 8 shapes no linked block has more than 256 entries."""
    keep = [c for c in SIM_CASES if not c.name.startswith("hh_64x8") and not c.name.startswith("hh_300x40")]
    got = sl.coverage(sim, keep)
    assert "kept_block>256" not in got
    assert sl.REQUIRED_SIM - got
    got = sl.coverage(sim, [c for c in SIM_CASES if c.name != "pull_sum_blocks_16389"])
    assert sl.REQUIRED_SIM - got == {"pull_blocks_tail"}


# ---- sharpness of every bound: a relative perturbation of 1e-9 in one output entry fails it
SHARP = [("spmv_65_L4", "y2", 40), ("dot_257", "dot", 0), ("ot_33", "x", 11), ("apply_129", "y", None), ("apply_all_tiles130", "y", None),
         ("apply_mv3_mixed", "y", None), ("hh_64x8_nbc3", "kept", 5), ("hh_64x8_nbc3", "two_pass", 70), ("hh_300x260_nbc1", "kept", 9),
         ("invert_all_b", "flat", 9), ("pull_sum", "out", 1201), ("gs_scatter_add", "dst", 3)]


@pytest.mark.parametrize("name,key,pos", SHARP, ids=["%s-%s" % (n, k) for n, k, _ in SHARP])
def test_bound_catches_a_perturbed_entry(sim, name, key, pos):
    case = sl.BY_NAME[name]
    res = result(sim, case)
    assert sl.check_case(case, res)[0] == []
    bad = copy_of(res)
    if pos is None:     # the first entry the kernel wrote
        raw = bad[key].view(np.uint64)
        pos = int(np.flatnonzero(raw != np.uint64(sl.CANARY))[0])
    assert bad[key][pos] != 0.0
    bad[key][pos] *= 1 + 1e-9
    assert sl.check_case(case, bad)[0] != []


HH_CASES = [c for c in sl.CASES if c.family == "householder"]


@pytest.mark.parametrize("mutant,names", [("swap_ij", ["hh_40x6_nbc1", "hh_64x8_nbc3", "hh_300x40_nbc1", "hh_300x260_nbc3"]),
                                          ("no_identity", [c.name for c in HH_CASES if c.name != "hh_5x1_nbc1"])])
def test_householder_bound_catches_a_mutant(sim, mutant, names):
    """A numpy restatement that swaps the roles of I and J in a linked block, and one that drops the identity cases (leading
    entry 0, zero slice, tiny norm): each must fail the bound of every case that has such a block / slice."""
    for name in names:
        case = sl.BY_NAME[name]
        res = result(sim, case)
        rec = sl.hh_mutant_record(case, mutant)
        bad = copy_of(res)
        stride = rec.shape[1] + sl.HH_PAD
        view = bad["kept"][:case.p["nbc"] * stride].reshape(case.p["nbc"], stride)
        view[:, :rec.shape[1]] = rec
        fails = sl.check_case(case, bad)[0]
        assert any(f.startswith("kept") for f in fails), (mutant, name)
        # ... while the unmutated float64 restatement passes the same bound
        good = copy_of(res)
        view = good["kept"][:case.p["nbc"] * stride].reshape(case.p["nbc"], stride)
        view[:, :rec.shape[1]] = sl.hh_mutant_record(case, None)
        assert sl.check_case(case, good)[0] == []


def test_canary_check_notices_a_stray_write(sim):
    case = sl.BY_NAME["apply_all_tile_alone"]
    res = result(sim, case)
    bad = copy_of(res)
    raw = bad["y"].view(np.uint64)
    stray = int(np.flatnonzero(raw == np.uint64(sl.CANARY))[0])
    bad["y"][stray] = 0.0
    assert sl.check_case(case, bad)[0] != []
    assert int((res["y"].view(np.uint64)[:sl.inputs(case)["n"]] != np.uint64(sl.CANARY)).sum()) == 64   # exactly the tile's rows
