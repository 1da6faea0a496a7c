"""The mass matrix and the shifted operator of the native Krylov solver on the MI355X: the checks of
tests/native_shifted_cases.py on the product library (hymls_amd/libhymls_mi.so, the HIP kernel k_kry_shifted of
krylov_hip.hip)."""
import os
import subprocess

import pytest

import native_shifted_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099, 2 ** 20 + 3])
def test_shifted_product_gpu(gpu_lib, n):
    cases.check_shifted_product(gpu_lib, "cuda", n)


def test_refusals_gpu(gpu_lib):
    cases.check_refusals(gpu_lib, "cuda")


def test_solver_properties_gpu(gpu_lib):
    cases.check_solver_properties(gpu_lib, "cuda")


def test_exact_scaled_gpu(gpu_lib):
    cases.check_exact_scaled(gpu_lib, "cuda")


@pytest.mark.parametrize("name", ["laplace", "stokes"])
def test_shifted_solve_gpu(gpu_lib, name):
    cases.check_shifted_solve(gpu_lib, "cuda", name)


def test_correction_equation_gpu(gpu_lib):
    cases.check_correction_equation(gpu_lib, "cuda")


def test_lockstep_gpu(gpu_lib):
    cases.check_lockstep(gpu_lib, "cuda")


def test_bordered_gpu(gpu_lib):
    cases.check_bordered(gpu_lib, "cuda")


def test_shifted_solve_from_plain_c(gpu_lib, tmp_path):
    exe = str(tmp_path / "capi_solve_shifted")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi", "capi_solve_shifted.c"),
                           "-o", exe, "-L", os.path.join(ROOT, "hymls_amd"), "-lhymls_mi", "-Wl,-rpath," + os.path.join(ROOT, "hymls_amd"), "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CAPI_SOLVE_SHIFTED" in out.stdout, out.stdout + out.stderr
