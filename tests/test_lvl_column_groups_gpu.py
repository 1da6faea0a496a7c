"""-m gpu: the merged level solve (k_lvl_fwd<NV> / k_lvl_bwd<NV>) gives every column the same bits whatever group it is
solved in.  Stokes-C 16^3, separator length 8, one level, Skew Cartesian, with the fused interior solve switched off
(the setting of test_merged_level_solve_path_gpu), whole-front tasks and 64-row tile tasks; 7 right-hand sides, which
the launcher solves as 4 + 2 + 1, as 2 + 2 + 2 + 1 under HYMLS_MI_MV_GROUP_LVL=2 and one by one under =1.

The switches are read once per process, so every combination runs in a child process of its own with a time limit;
after the first child that fails, times out or dies from a signal no further GPU child is started."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import problem, oracle_prec, rel_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_ROWS = ("256", "32")          # whole-front tasks / 64-row tile tasks
CAPS = (None, "2", "1")             # HYMLS_MI_MV_GROUP_LVL
NVEC = 7
CHILD_TIMEOUT = 120

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, "tests")
from common import problem, xml_params, product_prec
import hymls_amd
A, tv = problem("Stokes-C", 16)
P = product_prec(A, tv, xml_params("Stokes-C", 16, 8, 1, partitioner="Skew Cartesian"), hymls_amd.load_library())
B = np.random.default_rng(31).uniform(-1, 1, (A.shape[0], %d))
X = P.ApplyInverse(B)
singles = np.stack([P.ApplyInverse(B[:, j].copy()) for j in range(B.shape[1])], axis=1)
np.savez(sys.argv[1], B=B, X=X, singles=singles)
''' % NVEC


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(small_rows, cap) -> arrays of the child, or the reason it has none."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = tmp_path_factory.mktemp("lvl_groups")
    out, failed = {}, None
    for rows in SMALL_ROWS:
        for cap in CAPS:
            key = (rows, cap)
            if failed:
                out[key] = "not started: %s failed before" % (failed,)
                continue
            env = {k: v for k, v in os.environ.items() if k != "HYMLS_MI_MV_GROUP_LVL"}
            env.update(HYMLS_MI_NO_FUSED_SOLVE="1", HYMLS_MI_LVL_SMALL_ROWS=rows)
            if cap:
                env["HYMLS_MI_MV_GROUP_LVL"] = cap
            path = str(base / ("rows%s_cap%s.npz" % (rows, cap)))
            try:
                p = subprocess.run([sys.executable, "-c", CHILD, path], cwd=ROOT, env=env, capture_output=True, text=True,
                                   timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                out[key], failed = "timed out after %d s" % CHILD_TIMEOUT, key
                continue
            if p.returncode != 0:
                out[key], failed = "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:]), key
                continue
            out[key] = dict(np.load(path))
    return out


@pytest.fixture(scope="module")
def oracle_column0():
    A, tv = problem("Stokes-C", 16)
    O = oracle_prec(A, tv, "Stokes-C", 16, 8, 1, partitioner="Skew Cartesian")
    b = np.random.default_rng(31).uniform(-1, 1, (A.shape[0], NVEC))[:, 0]
    return b, O.apply_inverse(b)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_lvl_column_groups_give_the_same_bits(runs, oracle_column0, rows):
    res = {}
    for cap in CAPS:
        res[cap] = runs[(rows, cap)]
        assert isinstance(res[cap], dict), "rows %s, cap %s: %s" % (rows, cap, res[cap])
    ref = res[None]
    b0, x0 = oracle_column0
    assert same_bits(ref["B"][:, 0], b0)
    for cap in CAPS:
        R = res[cap]
        worst = max(rel_diff(R["X"][:, j], R["singles"][:, j]) for j in range(NVEC))
        print("rows %s, cap %s: largest relative difference of a column from its single-vector solve %.3g, column 0 from "
              "the oracle %.3g" % (rows, cap, worst, rel_diff(R["X"][:, 0], x0)))
    for cap in CAPS[1:]:
        assert same_bits(res[cap]["X"], ref["X"]), "HYMLS_MI_MV_GROUP_LVL=%s differs from the default groups" % cap
    diff = [j for j in range(NVEC) if not same_bits(ref["X"][:, j], ref["singles"][:, j])]
    assert diff == [], "columns %s differ from their single-vector solves" % diff
    assert rel_diff(ref["X"][:, 0], x0) < 1e-8
