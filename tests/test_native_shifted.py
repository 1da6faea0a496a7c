"""The mass matrix and the shifted operator a K + b B of the native Krylov solver (hymls_mi_solver_set_mass_matrix,
hymls_mi_solver_set_shift, hymls_mi_shifted_product, hymls_amd.NativeSolver.SetMassMatrix / setShift) on CPU tensors through a
TEST-ONLY simulator library (tests/krylov_shift_sim: the sources of tests/krylov_proj_sim plus a plain-loop shifted product
with the kernel's lane decomposition), built here in a temporary directory.  The checks themselves are in
tests/native_shifted_cases.py; tests/test_native_shifted_gpu.py runs them on the product library."""
import json
import os
import subprocess
import sys

import pytest

import hymls_amd
import native_shifted_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ssim(tmp_path_factory):
    out = tmp_path_factory.mktemp("krylov_shift_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_shift_sim"), "OUT=%s" % out])
    path = str(out / "libhymls_mi_krylov_shift_sim.so")
    return path, hymls_amd.load_library(path)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_shifted_product_sim(ssim, n):
    cases.check_shifted_product(ssim[1], "cpu", n)


def test_refusals_sim(ssim):
    cases.check_refusals(ssim[1], "cpu")


def test_solver_properties_sim(ssim):
    cases.check_solver_properties(ssim[1], "cpu")


def test_exact_scaled_sim(ssim):
    cases.check_exact_scaled(ssim[1], "cpu")


@pytest.mark.parametrize("name", ["laplace", "stokes"])
def test_shifted_solve_sim(ssim, name):
    cases.check_shifted_solve(ssim[1], "cpu", name)


def test_correction_equation_sim(ssim):
    cases.check_correction_equation(ssim[1], "cpu")


def test_lockstep_sim(ssim):
    cases.check_lockstep(ssim[1], "cpu")


def test_bordered_sim(ssim):
    cases.check_bordered(ssim[1], "cpu")


def test_sharded_handle_is_refused_sim(ssim):
    """two ranks (torch.distributed.run, gloo, as tests/dist_worker.py): a solve with a shift returns -99 on every rank, and
    the plain sharded solve works again after setShift(1, 0)"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29743", os.path.join(ROOT, "tests", "native_shifted_worker.py")]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HYMLS_KRYLOV_SIM_LIB=ssim[0])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("NSHIFT_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("NSHIFT_RESULT "):])
    assert res["set"] == [0, 0] and res["codes"] == [-99, -99] and res["plain_ok"], res


def test_simulator_without_the_macro_returns_m99(tmp_path):
    """tests/krylov_proj_sim, built from this tree without HYMLS_MI_SHIFTED_SOLVER and without the shifted product, still loads,
    and every new symbol returns -99"""
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_proj_sim"), "OUT=%s" % tmp_path])
    cases.missing_symbols_return_m99(hymls_amd.load_library(str(tmp_path / "libhymls_mi_krylov_proj_sim.so")))
