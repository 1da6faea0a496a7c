"""-m "not gpu": the fused interior solve and its panel layouts (tests/fusedlab) on the host simulator, against the numpy
references of the lab.  This proves the harness, the references, the error bound, the canaries and the coverage tags on a
machine without a GPU; tests/test_fusedlab_gpu.py runs the same cases through the product library."""
import importlib.util
import os
import sys

import numpy as np
import pytest

LAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fusedlab")


def _load(name):
    """tests/fusedlab/<name>.py as module fusedlab_<name> (the other labs have modules of the same file names)."""
    key = "fusedlab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


fc = _load("cases")

SIM_CASES = [c for c in fc.CASES if c.sim]
_results = {}


@pytest.fixture(scope="module")
def sim():
    return fc.load("sim")


def result(sim, case):
    if case.name not in _results:
        _results[case.name] = fc.run_case(sim, case)
    return _results[case.name]


@pytest.mark.parametrize("case", SIM_CASES, ids=[c.name for c in SIM_CASES])
def test_fused_case(sim, case):
    R = result(sim, case)
    assert all(T["fits"] for T in fc.tables_of(R))
    assert fc.exact_failures(case, R) == []
    ratios = fc.panel_ratios(case, R)
    print("fusedlab %s: error / bound (simulator) %s" % (case.name, ratios))
    assert max(ratios.values()) <= 1.0, ratios
    assert fc.end_to_end_failures(case, R) == []


@pytest.mark.parametrize("case", SIM_CASES, ids=[c.name for c in SIM_CASES])
def test_bound_holds_for_a_float64_restatement(sim, case):
    """Validity of the bound, shown without any kernel: the reference's own sweeps in float64, plain order."""
    ratios = fc.panel_ratios(case, result(sim, case), x_of=fc.float64_restatement)
    print("fusedlab %s: error / bound (float64 numpy) %s" % (case.name, ratios))
    assert max(ratios.values()) <= 1.0, ratios


def test_demote_and_round_panels(sim):
    assert fc.demote_failures(sim) == []


def test_case_list_covers_every_branch(sim):
    got = fc.coverage([(c, result(sim, c)) for c in SIM_CASES])
    assert sorted(fc.REQUIRED_SIM - got) == []


def test_coverage_notices_a_missing_case(sim):
    """The coverage check itself: without the arrowhead of seven leaves no assembly row takes the list route."""
    keep = [c for c in SIM_CASES if c.name != "arrow_7x24_top37"]
    got = fc.coverage([(c, result(sim, c)) for c in keep])
    assert "rec_list" not in got
    assert fc.REQUIRED_SIM - got


def test_harness_checks_its_index_arrays(sim):
    """Every host-side check of the harness answers with its error code and launches nothing."""
    case = fc.BY_NAME["arrow_2x5_top3"]
    c = case.classes[0]
    pat = c.pattern()
    sim.reset()
    T = sim.plan(pat, [0, pat.nI], c.leaf, c.max_width, True)
    kval = np.concatenate([fc.class_values(case, 0, pat, b)[pat.rows, pat.cols] for b in range(2)])
    sim.factor(T, kval)
    nI, n = pat.nI, 2 * pat.nI
    subs = [(T["id"], 0, 0), (T["id"], 1, nI)]
    I = fc.io_inputs(case, n)

    def io(**kw):
        a = dict(I, **kw)
        return sim.solve_io(kw.get("subs", subs), n, a["nuser"], a["perm"], a["a_row"], a["a_col"], a["a_val"], a["x2"], a["z"], a["b"],
                            case.a_lanes, a["hint"])

    def code(fn):
        with pytest.raises(fc.HarnessError) as e:
            fn()
        return e.value.code

    io()
    perm = I["perm"].copy()
    perm[1] = perm[0]
    assert code(lambda: io(perm=perm)) == fc.ERRORS["perm"]
    perm[1] = I["nuser"]
    assert code(lambda: io(perm=perm)) == fc.ERRORS["perm"]
    a_col = I["a_col"].copy()
    a_col[0] = len(I["x2"])
    assert code(lambda: io(a_col=a_col)) == fc.ERRORS["a_col"]
    a_row = I["a_row"].copy()
    a_row[3] = a_row[4] + 1
    assert code(lambda: io(a_row=a_row)) == fc.ERRORS["a_row"]
    a_row = I["a_row"].copy()
    a_row[-1] -= 1
    assert code(lambda: io(a_row=a_row)) == fc.ERRORS["a_row"]
    assert code(lambda: io(subs=[(T["id"], 0, 0), (T["id"], 1, nI - 1)])) == fc.ERRORS["xoff"]
    assert code(lambda: sim.solve(0, [(T["id"], 0, 0), (T["id"], 1, nI - 1)], np.zeros(n), n)) == fc.ERRORS["xoff"]
    assert code(lambda: sim.solve(0, [(T["id"], 0, 0), (T["id"], 1, nI + 1)], np.zeros(n), n)) == fc.ERRORS["xoff"]
    # a class outside fused_solve_fits: the whole shell of a 10^3 box puts its root front on the multi-workgroup path
    sim.reset()
    big = fc.fl.grid_box(10, 10, 10, 7)
    Tb = sim.plan(big, [0], 24, 256, True)
    assert not Tb["fits"]
    kval = fc.fl.member_values(big, 1)[big.rows, big.cols]
    sim.factor(Tb, kval)
    assert code(lambda: sim.solve(0, [(Tb["id"], 0, 0)], np.zeros(big.nI), big.nI)) == fc.ERRORS["fits"]
    sim.reset()


# ------------------------------------------------------------------ sharpness: what the checks must catch
SHARP = "grid27_6"


def test_bound_catches_a_perturbed_entry(sim):
    """1e-9 max|x| added to one output entry fails the panel bound."""
    case = fc.BY_NAME[SHARP]
    R = result(sim, case)

    def perturbed(kind, T, slab, rhs, x):
        y = x.copy()
        y[len(y) // 3] += 1e-9 * np.abs(x).max()
        return y

    assert max(fc.panel_ratios(case, R).values()) <= 1.0
    assert min(fc.panel_ratios(case, R, x_of=perturbed).values()) > 1.0


def test_repack_equality_catches_a_swapped_pair(sim):
    """One swapped pair in the numpy repack permutation fails the equality."""
    case = fc.BY_NAME[SHARP]
    R = result(sim, case)
    T = fc.tables_of(R)[0]
    U = R["c0_slab"]
    members = range(T["nb"])
    assert fc.same_bits(R["c0_repacked"], fc.repack_reference(T, U, members))
    s = int(np.argmax(T["fronts"][:, 0]))
    assert not fc.same_bits(R["c0_repacked"], fc.repack_reference(T, U, members, swap=(s, 1, 2)))


def test_bound_catches_a_dropped_assembly_source(sim):
    """One dropped assembly source in the numpy reference fails the bound."""
    case = fc.BY_NAME[SHARP]
    R = result(sim, case)
    T = fc.tables_of(R)[0]
    child = int(np.flatnonzero(T["fronts"][:, 1] > 0)[0])     # a front with update rows: it contributes to its parent
    assert max(fc.panel_ratios(case, R, drop=(child, 0)).values()) > 1.0
