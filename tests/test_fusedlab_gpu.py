"""-m gpu: the fused interior solve and its panel layouts on the MI355X (tests/fusedlab through the product library),
against the numpy references of the lab, under every switch of the fused launchers.

Every environment variant runs in a child process of its own (the switches are read per process) with a time limit;
after the first child that fails, times out or dies from a signal no further GPU child is started."""
import importlib.util
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LAB = os.path.join(HERE, "fusedlab")


def _load(name):
    """tests/fusedlab/<name>.py as module fusedlab_<name> (the other labs have modules of the same file names)."""
    key = "fusedlab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


fc = _load("cases")
fchild = _load("child")

VARIANTS = [
    ("default", {}),
    ("mv_group_1", {"HYMLS_MI_MV_GROUP_FUSED": "1"}),      # every column through the single-vector kernel
    ("mv_group_2", {"HYMLS_MI_MV_GROUP_FUSED": "2"}),      # groups of two columns at the most
    ("fused_prof", {"HYMLS_MI_FUSED_PROF": "1"}),          # the kernels with the per-phase clock reads
]
MV_CAP = {"default": 4, "mv_group_1": 1, "mv_group_2": 2, "fused_prof": 4}
CHILD_TIMEOUT = 240
_SWITCHES = {k for _, env in VARIANTS for k in env}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """variant -> output directory, or the reason it has no results."""
    fc.build("gpu")
    base = tmp_path_factory.mktemp("fusedlab")
    out, failed = {}, None
    for name, env in VARIANTS:
        if failed:
            out[name] = "not started: variant %s failed before" % failed
            continue
        e = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        e.update(env)
        d = str(base / name)
        try:
            p = subprocess.run([sys.executable, os.path.join(LAB, "child.py"), d], env=e,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            out[name] = "timed out after %d s" % CHILD_TIMEOUT
            failed = name
            continue
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            out[name] = "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
            failed = name
            continue
        out[name] = d
    return out


_cache = {}


def results(runs, variant):
    d = runs[variant]
    assert os.path.isdir(d), "variant %s: %s" % (variant, d)
    if variant not in _cache:
        _cache[variant] = {c.name: fchild.load(d, c) for c in fc.CASES}
    return _cache[variant]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [v for v, _ in VARIANTS])
def test_fused_cases(runs, variant):
    res = results(runs, variant)
    with open(os.path.join(runs[variant], "demote.txt")) as f:
        bad = [line for line in f.read().split("\n") if line]
    worst = {}
    for case in fc.CASES:
        R = res[case.name]
        bad += ["%s: class %d outside fused_solve_fits" % (case.name, T["id"]) for T in fc.tables_of(R) if not T["fits"]]
        bad += ["%s: %s" % (case.name, m) for m in fc.exact_failures(case, R)]
        for kind, ratio in fc.panel_ratios(case, R).items():
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            if not ratio <= 1.0:
                bad.append("%s: %s solve: error / bound = %.3g" % (case.name, kind, ratio))
        if variant == "default":
            bad += ["%s: %s" % (case.name, m) for m in fc.end_to_end_failures(case, R)]
    print("fusedlab %s: largest error / bound on the GPU %s" % (variant, worst))
    assert bad == []


@pytest.mark.gpu
def test_phase_profiling_gives_the_same_solution(runs):
    ref, prof = results(runs, "default"), results(runs, "fused_prof")
    diff = [c.name for c in fc.CASES for key in ("x_single", "x_mv7", "x_f32", "io_user_fused")
            if key in ref[c.name] and not fc.same_bits(ref[c.name][key], prof[c.name][key])]
    assert diff == []


@pytest.mark.gpu
def test_column_groups_give_the_same_solution(runs):
    ref = results(runs, "default")
    for variant in ("mv_group_1", "mv_group_2"):
        other = results(runs, variant)
        diff = [c.name for c in fc.CASES for nv in fc.NV_LIST
                if "x_mv%d" % nv in ref[c.name] and not fc.same_bits(ref[c.name]["x_mv%d" % nv], other[c.name]["x_mv%d" % nv])]
        assert diff == [], "%s differs from the default groups" % variant


@pytest.mark.gpu
def test_case_list_covers_every_branch(runs):
    got = set()
    for variant in ("default", "mv_group_1", "mv_group_2"):
        res = results(runs, variant)
        got |= fc.coverage([(c, res[c.name]) for c in fc.CASES], gpu=True, mv_cap=MV_CAP[variant])
    assert sorted(fc.REQUIRED_GPU - got) == []
    # the halvings are the default launcher's own: no cap may be needed to see them
    res = results(runs, "default")
    own = fc.coverage([(c, res[c.name]) for c in fc.CASES], gpu=True)
    assert {"lds>64KiB", "mv_group=4", "mv_halved_to_2", "mv_halved_to_1"} <= own
