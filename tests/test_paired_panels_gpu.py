"""-m gpu: the panels of the wide levels of the fused interior solve in column pairs (device.hpp: FrontD::pair) on the MI355X,
through tests/fusedlab and the development switch HYMLS_MI_FORCE_PAIRED_PANELS: the repacked slab is the numpy
restatement of the layout, and every solve has the bits of the same solve with packed panels.

One child process (tests/paired_worker.py) runs all cases, with a time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import paired_cases as pc
import paired_layout as pl
import paired_worker

fc = pc.fc
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240
SOLVES = ["x", "x_f32", "io10", "io21", "x_mv2", "x_mv3", "x_mv5", "x_mv3_f32", "x_transposed"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    fc.build("gpu")
    d = str(tmp_path_factory.mktemp("paired"))
    env = {k: v for k, v in os.environ.items() if k not in ("HYMLS_MI_FORCE_PAIRED_PANELS", "HYMLS_MI_MV_GROUP_FUSED", "HYMLS_MI_FUSED_PROF")}
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "paired_worker.py"), d], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        return "timed out after %d s" % CHILD_TIMEOUT
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        return "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    return d


_cache = {}


def results(run, case):
    assert os.path.isdir(run), run
    if case.name not in _cache:
        _cache[case.name] = paired_worker.load(run, case)
    return _cache[case.name]


def tables(R):
    ci = 0
    while "c%d_fronts" % ci in R:
        yield ci, {"fronts": R["c%d_fronts" % ci], "fw_ptr": R["c%d_fw_ptr" % ci], "bw_ptr": R["c%d_bw_ptr" % ci]}
        ci += 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", pc.CASES, ids=repr)
def test_repack_is_the_numpy_layout(run, case):
    R = results(run, case)
    assert not R["flags"].any(), "a factor flag was raised or a guard tail was written: %s" % R["flags"]
    for ci, T in tables(R):
        U = R["c%d_slab" % ci]
        members = range(U.shape[0])
        assert fc.same_bits(R["c%d_packed" % ci], fc.repack_reference(T, U, members)), "class %d, packed" % ci
        assert fc.same_bits(R["c%d_paired" % ci], pl.paired_reference(T, U, members)), "class %d, paired" % ci


@pytest.mark.gpu
@pytest.mark.parametrize("case", pc.CASES, ids=repr)
def test_solves_have_the_bits_of_packed_panels(run, case):
    R = results(run, case)
    n = int(R["n"])
    for key in SOLVES:
        a, b = R[key + "_packed"], R[key + "_paired"]
        assert fc.same_bits(a, b), "%s: paired panels change the bits of %s" % (case.name, key)
        assert np.isfinite(a[..., :n][~fc.is_canary(a[..., :n])]).all(), key


@pytest.mark.gpu
def test_cases_reach_every_branch(run):
    reached, paired_differs = set(), False
    for case in pc.CASES:
        R = results(run, case)
        for ci, T in tables(R):
            reached |= pc.tags_of(T)
            paired_differs |= not fc.same_bits(R["c%d_packed" % ci], R["c%d_paired" % ci])
    assert pc.REQUIRED - reached == set()
    assert paired_differs, "the development switch did not pair a single panel"


@pytest.mark.gpu
def test_repack_check_is_sharp(run):
    """The two halves of one pair exchanged in the numpy permutation: the comparison of test_repack_is_the_numpy_layout fails."""
    case = fc.BY_NAME["grid7_8"]
    R = results(run, case)
    ci, T = next(tables(R))
    U = R["c%d_slab" % ci]
    s = next(s for s, p in enumerate(pl.front_pairs(T)) if p & pl.PAIR_L and T["fronts"][s, 0] >= 2 and T["fronts"][s, 1] >= 1)
    w, ri = (int(v) for v in T["fronts"][s, :2])
    t0, t1 = w, w + (w + ri)              # entries (w, 0) and (w, 1): the first pair of the first update row
    mutant = pl.paired_reference(T, U, range(U.shape[0]), swap=(s, t0, t1))
    assert not fc.same_bits(R["c%d_paired" % ci], mutant)
