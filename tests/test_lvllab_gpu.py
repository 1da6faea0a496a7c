"""-m gpu: the level-solve lab (tests/lvllab) on the MI355X: k_lvl_fwd / k_lvl_bwd<NV, float> on the demoted slab against
<NV, double> on float-rounded panels, bit for bit, for nv in {1, 2, 3, 4, 7}, with ld = n + 5 and with column groups
capped at 1 and 2; every column against its single-vector solve; the bound against the longdouble sweeps and its
sharpness.  One child process (tests/lvllab/child.py) runs every case; its record is read here."""
import json
import os
import subprocess
import sys

import pytest

from test_lvllab import lc

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("HYMLS_MI_MV_GROUP_LVL", "HYMLS_MI_LVL_SMALL_ROWS")


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    path = str(tmp_path_factory.mktemp("lvllab_gpu") / "lvllab.json")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "lvllab", "child.py"), path], env=env, capture_output=True,
                           text=True, timeout=300)
        note = "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
        sys.stdout.write(p.stdout)
    except subprocess.TimeoutExpired:
        note = "timed out after 300 s"
    rec = {}
    if os.path.exists(path):
        with open(path) as f:
            rec = json.load(f)
    return rec, note


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c.name for c in lc.CASES])
def test_level_solve_f32_gpu(record, case):
    rec, note = record
    assert case in rec, "the child did not reach this case: " + note
    assert not rec[case]["failures"], "\n".join(rec[case]["failures"])


@pytest.mark.gpu
def test_task_kinds_and_lds_attribute_gpu(record):
    """both task kinds are reached, and dense_w2100 at NV = 4 needs more LDS than a kernel gets without the attribute"""
    rec, note = record
    assert set(rec) == {c.name for c in lc.CASES}, note
    assert {k for r in rec.values() for k in r["kinds"]} == {"whole", "tile"}
    assert 64 * 1024 < rec[lc.BIG.name]["lds_bytes_nv4"] <= 160 * 1024
