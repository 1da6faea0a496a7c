"""-m gpu: the solve kernels whose leftover panel loads are issued as one batch (k_interior_fused, k_interior_fused_io,
k_interior_fused_mv, fused_spmv_rows, k_lvl_fwd / k_lvl_bwd) give, bit for bit, the solutions recorded before that change.

The batches move loads only: every entry is still added to the same accumulator in the same order, so the results may
not change in a single bit.  The fixtures under tests/golden/solve_tails/ are the solutions of the cases of
tests/solve_tails_cases.py computed by the kernels with the scalar leftover loops.  They are bound to the order of the
additions AND to the compiler's contraction of `a += l * f` into a fused multiply-add: after a deliberate change of the
summation, or with a compiler that contracts differently, record them again on the MI355X with
`python tools/record_solve_tails.py` (at the commit whose bits are to be kept) and say so in the commit.

All cases run in one child process with a time limit (a fault then ends the child, not the test session)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import solve_tails_cases as st

fc, fl = st.fc, st.fl
pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 180


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    fc.build("gpu")
    fl.build("gpu")
    d = str(tmp_path_factory.mktemp("solve_tails"))
    p = subprocess.run([sys.executable, os.path.join(st.HERE, "solve_tails_cases.py"), d], capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    sys.stdout.write(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    return d


def _npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", st.FUSED_CASES, ids=repr)
def test_fused_solves_keep_their_bits(out_dir, case):
    R = _npz(os.path.join(out_dir, "full_%s.npz" % case.name))
    assert fc.exact_failures(case, R) == []          # _mv = single, FusedIO = separate kernels, FP32 = rounded, guards
    assert st.fused_failures(case, R, st.load_golden("fused", case)) == []


@pytest.mark.parametrize("case", st.LVL_CASES, ids=repr)
def test_merged_level_solves_keep_their_bits(out_dir, case):
    z = _npz(os.path.join(out_dir, "lvl_%s.npz" % case.name))
    res = {"x": z["x"], "merged": int(z["info"][0]), "flag": int(z["info"][1]), "canary": int(z["info"][2])}
    gold = st.load_golden("lvl", case)
    assert np.array_equal(z["fronts"], gold["fronts"]), "the front table differs from the recorded one"
    assert st.lvl_failures(case, res, gold) == []


def test_cases_reach_every_changed_loop(out_dir):
    got = fc.coverage([(c, _npz(os.path.join(out_dir, "full_%s.npz" % c.name))) for c in st.FUSED_CASES], gpu=True)
    assert sorted(st.FUSED_TAGS - got) == []
    assert {"mv_group=4", "mv_group=2", "mv_group=1"} <= got
    assert {c.a_lanes for c in st.FUSED_CASES} == {1, 2, 4, 8}
    for c in st.FUSED_CASES:     # an empty A12 row among the first four row slots of the first thread (row 0)
        I = fc.io_inputs(c, 300)
        assert I["a_row"][1] == I["a_row"][0]
    shapes = st.lvl_shapes([_npz(os.path.join(out_dir, "lvl_%s.npz" % c.name)) for c in st.LVL_CASES])
    whole = {(w, ri) for kind, w, ri in shapes if kind == "whole"}
    assert {w for w, ri in whole} >= set(range(1, 10))
    assert {ri % 4 for w, ri in whole if ri} == {0, 1, 2, 3} and any(ri == 0 for w, ri in whole)
    assert {min(w, 3) for w, ri in whole} == {1, 2, 3} and any(w > 128 for w, ri in whole)
    tails = set()
    for kind, w, ri in shapes:
        if kind == "tile":
            tails |= st.lvl_tile_tails(w, ri)
    assert tails >= {(loop, t) for loop in ("fwd", "bwd_pivot", "bwd_uside") for t in range(1, 8)}
    assert any(kind == "tile" and ri == 0 for kind, w, ri in shapes) and any(kind == "tile" and ri % 4 for kind, w, ri in shapes)
