"""The bordered solve of the native Krylov solver (hymls_mi_solver_solve_bordered, hymls_amd.NativeBorderedSolver) on CPU
tensors through a TEST-ONLY simulator library (tests/krylov_border_sim: the sources of tests/krylov_f32_sim plus a
plain-loop border product with the kernel's decomposition), built here in a temporary directory.  The checks themselves
are in tests/native_bordered_cases.py; tests/test_native_bordered_gpu.py runs them on the product library."""
import json
import os
import subprocess
import sys

import pytest

import hymls_amd
import native_bordered_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bsim(tmp_path_factory):
    out = tmp_path_factory.mktemp("krylov_border_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_border_sim"), "OUT=%s" % out])
    path = str(out / "libhymls_mi_krylov_border_sim.so")
    return path, hymls_amd.load_library(path)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_border_product_sim(bsim, n):
    cases.check_border_product(bsim[1], "cpu", n)


def test_border_product_refusals_sim(bsim):
    cases.check_border_product_refusals(bsim[1], "cpu")


@pytest.mark.parametrize("with_c", [True, False])
def test_exact_sim(bsim, with_c):
    cases.check_exact(bsim[1], "cpu", with_c)


def test_stokes_random_border_sim(bsim):
    cases.check_stokes_random_border(bsim[1], "cpu")


def test_singular_stokes_sim(bsim):
    cases.check_singular_stokes(bsim[1], "cpu")


def test_laplace_variants_sim(bsim):
    cases.check_laplace_variants(bsim[1], "cpu")


def test_previous_repeat_sim(bsim):
    cases.check_previous_repeat(bsim[1], "cpu")


def test_life_cycle_sim(bsim):
    cases.check_life_cycle(bsim[1], "cpu")
    cases.check_too_many_border_columns(bsim[1], "cpu")


def test_driver_stokes4_3d_native_sim(bsim, tmp_path):
    cases.check_driver(bsim[1], "cpu", tmp_path)


def test_sharded_handle_is_refused_sim(bsim):
    """two ranks (torch.distributed.run, gloo, as tests/dist_worker.py): the bordered entry returns -99 on every rank"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29733", os.path.join(ROOT, "tests", "native_bordered_worker.py")]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HYMLS_KRYLOV_SIM_LIB=bsim[0])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("NBORDER_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("NBORDER_RESULT "):])
    assert res["codes"] == [-99, -99] and res["codes_bordered"] == [-99, -99] and res["plain_ok"], res


def test_simulator_without_the_macro_returns_m99(tmp_path):
    """tests/krylov_sim, built from this tree without HYMLS_MI_BORDERED_SOLVER and without a border product launcher,
    still loads, and both new symbols return -99"""
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_sim"), "OUT=%s" % tmp_path])
    cases.missing_symbols_return_m99(hymls_amd.load_library(str(tmp_path / "libhymls_mi_krylov_sim.so")))
