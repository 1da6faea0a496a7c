"""-m gpu: FP32 storage of the interior factor panels ("MI Factor Storage" = "single") on the MI355X: the checks of
tests/f32_cases.py on the product library.  Bitwise equality with FP64 storage of float-rounded panels pins the FP32
instantiations of k_interior_fused / k_interior_fused_mv and k_demote_panels entry by entry.

Every group runs in a child process of its own (tests/f32_child.py) with a time limit; after the first child that
fails a check, times out or dies no further GPU child is started."""
import json
import os
import subprocess
import sys

import pytest

import f32_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
# group, time limit in seconds
GROUPS = [("case:" + c, 300) for c in fc.CASE_IDS] + [("defaults_lifecycle", 300), ("python_xml", 300), ("solver32", 600),
                                                      ("solver64", 900), ("memory64", 600)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """group -> record written by the child, or the reason there is none"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = tmp_path_factory.mktemp("f32_gpu")
    env = {k: v for k, v in os.environ.items() if k != "HYMLS_MI_ROUND_PANELS"}
    out, failed = {}, None
    for group, limit in GROUPS:
        if failed:
            out[group] = "not started: group %s failed before" % failed
            continue
        path = str(base / (group.replace(":", "_") + ".json"))
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "f32_child.py"), group, path], env=env,
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
@pytest.mark.parametrize("case", fc.CASE_IDS)
def test_bitwise_against_rounded_fp64_panels_gpu(runs, case):
    """cases 1, 2 and 5: nvec 1, 2, 3, 5 equal FP64 storage of rounded panels bit for bit, differ from plain FP64 by less
    than sqrt(2^-24) and by more than 0; the byte figures halve"""
    passed(runs, "case:" + case)


@pytest.mark.gpu
def test_defaults_and_lifecycle_gpu(runs):
    passed(runs, "defaults_lifecycle")


@pytest.mark.gpu
def test_python_and_xml_gpu(runs):
    passed(runs, "python_xml")


@pytest.mark.gpu
def test_solver_gpu(runs):
    """GMRES(100) to 1e-8, Stokes-C 32^3 three-level, hymls_amd.Solver and the native solver, both storages"""
    passed(runs, "solver32")


@pytest.mark.gpu
def test_solver_stokes64_gpu(runs):
    passed(runs, "solver64")


@pytest.mark.gpu
def test_device_memory_gpu(runs):
    """free device memory grows by at least 90 % of half the demoted panel bytes, Stokes-C 64^3"""
    passed(runs, "memory64")


def test_both_instantiations_in_the_code_object():
    """(no GPU needed: reads the built library) the gfx950 code object of the product library holds the FP64 and the FP32 form of both fused kernels and the
    demotion kernel (mangled names: ...k_interior_fusedILb0EdEE / ...ILb0EfEE, ...k_interior_fused_mvILi4EdEE / ...EfEE)"""
    with open(os.path.join(os.path.dirname(HERE), "hymls_amd", "libhymls_mi.so"), "rb") as f:
        blob = f.read()
    for name in (b"k_interior_fusedILb0EdEE", b"k_interior_fusedILb0EfEE", b"k_interior_fused_mvILi4EdEE", b"k_interior_fused_mvILi4EfEE",
                 b"k_interior_fused_mvILi2EdEE", b"k_interior_fused_mvILi2EfEE", b"k_demote_panels"):
        assert name in blob, name
