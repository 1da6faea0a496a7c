"""-m "not gpu": the level-solve lab (tests/lvllab) on the TEST-ONLY simulator: the merged level solve of one class on the
FP32 slab against the FP64 launchers on float-rounded panels (bitwise), column groups, and the bound against the
longdouble sweeps.  This pins the harness, the tables MergedSolve::set_storage writes and the plain-loop launchers of
tests/lvllab/lvl_f32_sim.cpp; tests/test_lvllab_gpu.py runs the same checks on the HIP kernels."""
import importlib.util
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _cases():
    key = "lvllab_cases"
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(HERE, "lvllab", "cases.py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


lc = _cases()
# (dense_w2100 is there for the LDS attribute of the HIP launch; on the simulator it checks the tables of a tile-task front
# of more than 2048 rows and takes 20 s, so it runs without the two extra column-group settings)
SIM_CASES = list(lc.CASES)


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    return lc.load("sim", str(tmp_path_factory.mktemp("lvllab_sim")))


@pytest.fixture(scope="module")
def results(lab):
    return {}


@pytest.mark.parametrize("case", SIM_CASES, ids=[c.name for c in SIM_CASES])
def test_level_solve_f32_sim(lab, results, case):
    R = lc.run_case(lab, case, groups=(None,) if case is lc.BIG else (None, 1, 2))
    results[case.name] = lc.task_kinds(R)
    bad = lc.exact_failures(case, R) + lc.bound_failures(case, R)
    assert not bad, "\n".join(bad)


def test_cases_reach_both_task_kinds(lab, results):
    for case in SIM_CASES:
        if case.name not in results:
            results[case.name] = lc.task_kinds(lc.run_case(lab, case))
    assert set().union(*results.values()) == {"whole", "tile"}
