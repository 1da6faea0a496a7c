"""The bordered solve of the native Krylov solver on the MI355X: the checks of tests/native_bordered_cases.py on the
product library (hymls_amd/libhymls_mi.so, the HIP border product of krylov_hip.hip)."""
import os
import subprocess

import pytest

import native_bordered_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099, 2 ** 20 + 3])
def test_border_product_gpu(gpu_lib, n):
    cases.check_border_product(gpu_lib, "cuda", n)


def test_border_product_refusals_gpu(gpu_lib):
    cases.check_border_product_refusals(gpu_lib, "cuda")


@pytest.mark.parametrize("with_c", [True, False])
def test_exact_gpu(gpu_lib, with_c):
    cases.check_exact(gpu_lib, "cuda", with_c)


def test_stokes_random_border_gpu(gpu_lib):
    cases.check_stokes_random_border(gpu_lib, "cuda")


def test_singular_stokes_gpu(gpu_lib):
    cases.check_singular_stokes(gpu_lib, "cuda")


def test_laplace_variants_gpu(gpu_lib):
    cases.check_laplace_variants(gpu_lib, "cuda")


def test_previous_repeat_gpu(gpu_lib):
    cases.check_previous_repeat(gpu_lib, "cuda")


def test_life_cycle_gpu(gpu_lib):
    cases.check_life_cycle(gpu_lib, "cuda")
    cases.check_too_many_border_columns(gpu_lib, "cuda")


def test_driver_stokes4_3d_native_gpu(gpu_lib, tmp_path):
    cases.check_driver(gpu_lib, "cuda", tmp_path)


def test_bordered_solve_from_plain_c(gpu_lib, tmp_path):
    exe = str(tmp_path / "capi_solve_bordered")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi", "capi_solve_bordered.c"),
                           "-o", exe, "-L", os.path.join(ROOT, "hymls_amd"), "-lhymls_mi", "-Wl,-rpath," + os.path.join(ROOT, "hymls_amd"), "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CAPI_SOLVE_BORDERED" in out.stdout, out.stdout + out.stderr
