"""Lock-step columns of the native Krylov solver on the MI355X: the checks of tests/lockstep_cases.py on the product
library (hymls_amd/libhymls_mi.so: k_spmv_mv of device_hip.hip and the batched kernels of krylov_hip.hip).  Only this run
pins the batched kernels: on the simulator of tests/test_lockstep.py a batched launcher is the single-column one per
column."""
import os
import subprocess

import pytest

import lockstep_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ks", cases.K_SETS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099, 2 ** 20 + 3])
def test_orthogonalize_mv_gpu(gpu_lib, n, ks, f32):
    cases.check_orthogonalize_mv(gpu_lib, "cuda", n, ks, f32)


def test_orthogonalize_mv_refusals_gpu(gpu_lib):
    cases.check_orthogonalize_mv_refusals(gpu_lib, "cuda")


@pytest.mark.parametrize("name", ["laplace8", "stokes16", "oseen8"])
def test_matvec_mv_gpu(gpu_lib, name):
    cases.check_matvec_mv(gpu_lib, "cuda", name)


@pytest.mark.parametrize("storage", ["double", "single"])
@pytest.mark.parametrize("nvec,width", [(5, 4), (3, 2)])
@pytest.mark.parametrize("start", ["Zero", "Random"])
@pytest.mark.parametrize("right", [True, False])
def test_gmres_lockstep_gpu(gpu_lib, right, start, nvec, width, storage):
    cases.check_gmres(gpu_lib, "cuda", storage, right, start, nvec, width)


@pytest.mark.parametrize("storage", ["double", "single"])
@pytest.mark.parametrize("variant", ["maxit", "norestart"])
def test_gmres_lockstep_limits_gpu(gpu_lib, variant, storage):
    cases.check_gmres(gpu_lib, "cuda", storage, True, "Zero", 5, 4, variant)


@pytest.mark.parametrize("storage", ["double", "single"])
def test_gmres_lockstep_stokes32_gpu(gpu_lib, storage):
    cases.check_gmres_large(gpu_lib, "cuda", storage)


def test_gmres_lockstep_stokes32_single_factors_gpu(gpu_lib):
    cases.check_gmres_large(gpu_lib, "cuda", "double", "stokes32_single")


@pytest.mark.parametrize("width", [2, 4])
def test_cg_lockstep_gpu(gpu_lib, width):
    cases.check_cg(gpu_lib, "cuda", width)


def test_previous_gpu(gpu_lib):
    cases.check_previous(gpu_lib, "cuda")


def test_life_cycle_gpu(gpu_lib):
    cases.check_life_cycle(gpu_lib, "cuda")


def test_bordered_ignores_width_gpu(gpu_lib):
    cases.check_bordered_ignores_width(gpu_lib, "cuda")


def test_code_object_has_the_batched_kernels():
    """libhymls_mi.so carries k_spmv_mv and the batched Krylov kernels for both basis types"""
    lib = os.path.join(ROOT, "hymls_amd", "libhymls_mi.so")
    data = open(lib, "rb").read()
    for name in (b"k_spmv_mv", b"k_kry_tile_mvILb0Ed", b"k_kry_tile_mvILb1Ed", b"k_kry_tile_mvILb0Ef", b"k_kry_tile_mvILb1Ef",
                 b"k_kry_rows_mvId", b"k_kry_rows_mvIf", b"k_kry_reduce_mv", b"k_kry_reduce_norm_mv", b"k_kry_scale_by_mv",
                 b"k_kry_round_scale_by_mv", b"k_kry_widen_mv", b"k_kry_dot_mv", b"k_kry_cg_xr_mv", b"k_kry_cg_p_mv"):
        assert name in data, name


def test_lockstep_solve_from_plain_c(gpu_lib, tmp_path):
    exe = str(tmp_path / "capi_solve_lockstep")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi", "capi_solve_lockstep.c"),
                           "-o", exe, "-L", os.path.join(ROOT, "hymls_amd"), "-lhymls_mi", "-Wl,-rpath," + os.path.join(ROOT, "hymls_amd"), "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CAPI_SOLVE_LOCKSTEP" in out.stdout, out.stdout + out.stderr
