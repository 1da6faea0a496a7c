"""-m gpu: FP32 storage of the merged level-solve panels ("MI Merged Factor Storage" = "single") on the MI355X: the
checks of tests/merged_f32_cases.py on the product library.  Bitwise equality with FP64 storage of float-rounded panels
pins the float instantiations of k_lvl_fwd / k_lvl_bwd entry by entry: nvec 1, 2, 3 and 5 run NV = 1, 2 and 4.

Every group runs in a child process of its own (tests/merged_f32_child.py) with a time limit; after the first child that
fails a check, times out or dies no further GPU child is started."""
import json
import os
import subprocess
import sys

import pytest

import merged_f32_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("HYMLS_MI_ROUND_PANELS", "HYMLS_MI_NO_FUSED_SOLVE", "HYMLS_MI_MV_GROUP_LVL")   # (HYMLS_MI_LVL_F32_COLS passes through)
# group, time limit in seconds
GROUPS = [("run:" + r, 300) for r in mc.RUN_IDS] + [("defaults_lifecycle", 300), ("python_xml", 300), ("solver", 600)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """group -> record written by the child, or the reason there is none"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = tmp_path_factory.mktemp("merged_f32_gpu")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out, failed = {}, None
    for group, limit in GROUPS:
        if failed:
            out[group] = "not started: group %s failed before" % failed
            continue
        path = str(base / (group.replace(":", "_") + ".json"))
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "merged_f32_child.py"), group, path], env=env,
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[group] = "timed out after %d s" % limit
            failed = group
            continue
        sys.stdout.write(p.stdout)
        if p.returncode != 0 or not os.path.exists(path):
            out[group] = "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
            failed = group
            continue
        with open(path) as f:
            out[group] = json.load(f)
        if not out[group]["ok"]:
            failed = group
    return out


def passed(runs, group):
    rec = runs[group]
    assert isinstance(rec, dict), "%s: %s" % (group, rec)
    assert rec["ok"], "%s:\n%s" % (group, rec["message"])
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("run", mc.RUN_IDS)
def test_bitwise_against_rounded_fp64_panels_gpu(runs, run):
    """nvec 1, 2, 3, 5 equal FP64 storage of rounded panels bit for bit (merged alone, and merged + fused against both
    rounded), differ from plain FP64 by less than sqrt(2^-24) and by more than 0; which = 10 halves, which = 9 falls by
    half the demoted bytes"""
    passed(runs, "run:" + run)


@pytest.mark.gpu
def test_defaults_lifecycle_and_overflow_gpu(runs):
    passed(runs, "defaults_lifecycle")


@pytest.mark.gpu
def test_python_and_xml_gpu(runs):
    passed(runs, "python_xml")


@pytest.mark.gpu
def test_solver_gpu(runs):
    """GMRES(100) to 1e-8, Stokes-C 32^3 three-level, hymls_amd.Solver and the native solver, both merged storages: true
    residual below the tolerance, the iteration counts of the simulator"""
    passed(runs, "solver")

