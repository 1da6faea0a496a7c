"""-m gpu: the separator-side, vector and table kernels one by one on the MI355X (tests/seplab through the product library),
against the numpy references of the lab, under the switches that select another kernel.

Every environment variant runs in a child process of its own (the switches are read once per process) with a time limit;
after the first child that fails, times out or dies from a signal no further GPU child is started."""
import importlib.util
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LAB = os.path.join(HERE, "seplab")


def _load(name):
    """tests/seplab/<name>.py as module seplab_<name> (tests/frontlab has modules of the same file names)."""
    key = "seplab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


sl = _load("cases")
slchild = _load("child")

CHILD_TIMEOUT = 120
_SWITCHES = {k for _, env in sl.VARIANTS for k in env} | {"HYMLS_MI_SBLOCK_TWO_PASS"}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """variant -> output directory, or the reason it has no results."""
    sl.build("gpu")
    base = tmp_path_factory.mktemp("seplab")
    out, failed = {}, None
    for name, env in sl.VARIANTS:
        if failed:
            out[name] = "not started: variant %s failed before" % failed
            continue
        e = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        e.update(env)
        d = str(base / name)
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "seplab", "child.py"), d, name], env=e,
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


def directory(runs, variant):
    d = runs[variant]
    assert os.path.isdir(d), "variant %s: %s" % (variant, d)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [v for v, _ in sl.VARIANTS])
def test_kernels_match_reference(runs, variant):
    d = directory(runs, variant)
    bad, worst = [], {}
    for case in sl.cases_of(variant):
        fails, ratio = sl.check_case(case, slchild.load(d, case))
        bad += ["%s: %s" % (case.name, m) for m in fails]
        worst[case.family] = max(worst.get(case.family, 0.0), ratio)
    for fam in sorted(worst):
        print("seplab %s: %-22s largest error / bound %.3g" % (variant, fam, worst[fam]))
    assert bad == []


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [v for v, _ in sl.VARIANTS])
def test_case_list_covers_every_branch(runs, variant):
    got = slchild.load_coverage(directory(runs, variant))
    assert sorted(sl.REQUIRED_GPU[variant] - got) == []


@pytest.mark.gpu
def test_column_groups_give_identical_bits(runs):
    """The 4-, 2- and 1-column kernels form every sum in the same order."""
    ref = directory(runs, "default")
    for variant in ("mv_group_1", "mv_group_2"):
        d = directory(runs, variant)
        diff = [c.name for c in sl.cases_of(variant) if not sl.same_bits(slchild.load(ref, c)["y"], slchild.load(d, c)["y"])]
        assert diff == [], "%s differs from the default grouping" % variant
