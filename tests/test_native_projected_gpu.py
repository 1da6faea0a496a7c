"""The projection vectors of the native Krylov solver on the MI355X: the checks of tests/native_projected_cases.py on the
product library (hymls_amd/libhymls_mi.so, the HIP kernels k_kry_proj_* of krylov_hip.hip)."""
import os
import subprocess

import pytest

import native_projected_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099, 2 ** 20 + 3])
def test_oblique_project_gpu(gpu_lib, n):
    cases.check_oblique_project(gpu_lib, "cuda", n)


def test_oblique_project_refusals_gpu(gpu_lib):
    cases.check_oblique_project_refusals(gpu_lib, "cuda")


@pytest.mark.parametrize("with_b", [False, True])
def test_unit_properties_gpu(gpu_lib, with_b):
    cases.check_unit_properties(gpu_lib, "cuda", with_b)


def test_set_projection_refusals_gpu(gpu_lib):
    cases.check_set_projection_refusals(gpu_lib, "cuda")


@pytest.mark.parametrize("lor", ["Right", "Left"])
@pytest.mark.parametrize("with_b", [False, True])
def test_exact_gpu(gpu_lib, with_b, lor):
    cases.check_exact(gpu_lib, "cuda", with_b, lor)


@pytest.mark.parametrize("name", ["laplace", "stokes"])
def test_inexact_gpu(gpu_lib, name):
    cases.check_inexact(gpu_lib, "cuda", name)


def test_variants_gpu(gpu_lib):
    cases.check_variants(gpu_lib, "cuda")


def test_life_cycle_gpu(gpu_lib):
    cases.check_life_cycle(gpu_lib, "cuda")


def test_projected_solve_from_plain_c(gpu_lib, tmp_path):
    exe = str(tmp_path / "capi_solve_projected")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi", "capi_solve_projected.c"),
                           "-o", exe, "-L", os.path.join(ROOT, "hymls_amd"), "-lhymls_mi", "-Wl,-rpath," + os.path.join(ROOT, "hymls_amd"), "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CAPI_SOLVE_PROJECTED" in out.stdout, out.stdout + out.stderr
