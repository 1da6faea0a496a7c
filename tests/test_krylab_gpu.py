"""-m gpu: the vector, reduction and update kernels of the native Krylov solver, the orthogonalisation passes A, B and C pass
by pass (both basis types), the projection and border-product kernels, their batched (lock-step) forms and k_spmv_mv one
by one on the MI355X (tests/krylab through the product library), against the numpy references of the lab.
The simulator run (tests/test_krylab.py) proves the harness, the references and the bounds; this run pins the kernels:
every case within its bound or bit-exact, every partial of a tiled pass against its own rows, every batched column bit for
bit the single launch, every spmv_mv column bit for bit spmv(), nothing written outside the output set (the scratch of a
batched column is as long as that column's own grid needs), a refused launch writes nothing.

One child process (tests/krylab/child.py) runs every case, with a time limit; after a child that failed, timed out or died
from a signal nothing more is started on the GPU, and every test reports that child."""
import importlib.util
import os
import shutil
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LAB = os.path.join(HERE, "krylab")


def _load(name):
    """tests/krylab/<name>.py as module krylab_<name> (the other labs have modules of the same file names)."""
    key = "krylab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


kl = _load("cases")
klchild = _load("child")

CHILD_TIMEOUT = 120


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The output directory of the one child, or the reason it has no results.  The directory (a few hundred MB of whole
    output buffers) is removed when the module is done."""
    kl.build("gpu")
    d = str(tmp_path_factory.mktemp("krylab") / "out")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(LAB, "child.py"), d], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        yield "timed out after %d s" % CHILD_TIMEOUT
    else:
        sys.stdout.write(p.stdout[-4000:])
        print("krylab gpu: the child took %.1f s" % (time.time() - t0))
        yield d if p.returncode == 0 else "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    shutil.rmtree(d, ignore_errors=True)


def directory(run):
    assert os.path.isdir(run), "the child has no results: %s" % run
    return run


@pytest.mark.gpu
def test_kernels_match_reference(run):
    d = directory(run)
    bad, worst = [], {}
    for case in kl.CASES:
        fails, ratio = kl.check_case(case, klchild.load(d, case))
        bad += ["%s: %s" % (case.name, m) for m in fails]
        worst[case.family] = max(worst.get(case.family, 0.0), ratio)
    for fam in sorted(worst):
        print("krylab gpu: %-18s largest error / bound %.3g" % (fam, worst[fam]))
    ulps = kl.SQRT_ULPS.values()
    print("krylab gpu: out[k] of pass C against sqrt(out[k + 1]) of numpy: %d norms, %d bit-equal, largest distance %d ulp"
          % (len(ulps), sum(u == 0 for u in ulps), max(ulps, default=0)))
    assert bad == []


@pytest.mark.gpu
def test_case_list_covers_every_branch(run):
    got = klchild.load_coverage(directory(run))
    assert sorted(kl.REQUIRED - got) == []
