"""-m "not gpu": FP32 storage of the interior factor panels ("MI Factor Storage" = "single") on the TEST-ONLY simulator
tests/f32_sim -- the host simulator of tests/hostsim compiled with the option's macro, plus plain-loop versions of the
launchers it adds -- built here in a temporary directory.  This pins the host logic (slabs, tables, lifecycle, byte
figures, error codes); tests/test_f32_panels_gpu.py runs the same checks on the HIP kernels.  The checks themselves are
in tests/f32_cases.py."""
import json
import os
import subprocess
import sys

import pytest

import hymls_amd
import f32_cases as fc
from common import problem, xml_params, product_prec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def f32sim(tmp_path_factory):
    out = tmp_path_factory.mktemp("f32_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "f32_sim"), "OUT=%s" % out])
    path = str(out / "libhymls_mi_f32_sim.so")
    return path, hymls_amd.load_library(path)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_bitwise_against_rounded_fp64_panels_sim(f32sim, case):
    fc.check_case(f32sim[1], "cpu", case)


def test_defaults_untouched_sim(f32sim):
    fc.check_defaults(f32sim[1], "cpu")


def test_lifecycle_sim(f32sim):
    fc.check_lifecycle(f32sim[1], "cpu")


def test_build_without_fp32_kernels_refuses(hostsim_lib):
    """the unchanged simulator of tests/hostsim is built without the macro: both symbols exist, 32 is refused with -99"""
    A, tv = problem("Laplace", 8)
    P = product_prec(A, tv, xml_params("Laplace", 8, 4, 1), hostsim_lib)
    assert hostsim_lib.hymls_mi_factor_storage(P._h) == 64
    assert hostsim_lib.hymls_mi_set_factor_storage(P._h, 32) == -99
    assert "FP32" in hostsim_lib.hymls_mi_last_error(P._h).decode()
    assert hostsim_lib.hymls_mi_set_factor_storage(P._h, 64) == 0
    assert hostsim_lib.hymls_mi_set_factor_storage(P._h, 16) == -2
    assert hostsim_lib.hymls_mi_factor_storage(P._h) == 64 and P.IsComputed()
    assert P.apply_bytes(9) > 0


def test_overflow_guard_sim(f32sim):
    fc.check_overflow(f32sim[1], "cpu")


def test_solver_sim(f32sim):
    fc.check_solver(f32sim[1], "cpu", 32)


def test_sharded_sim(f32sim):
    """2 gloo ranks, Stokes-C 16^3, FP32 storage on every rank: the assembled result equals one rank in FP32 storage to
    the tolerance tests/test_sharded.py uses for FP64 storage"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29688", os.path.join(ROOT, "tests", "f32_dist_worker.py"), f32sim[0]]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("F32_DIST_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("F32_DIST_RESULT "):])
    print(res)
    assert res["cover_ok"] and res["storage"] == ["single", "single"]
    assert res["rel_err"] < 1e-12
    assert 0.0 < res["rel_to_double"] < fc.CAP
    assert res["bytes1_ratio"] == 0.5


def test_python_and_xml_sim(f32sim, tmp_path):
    fc.check_python_and_xml(f32sim[1], "cpu", tmp_path)
