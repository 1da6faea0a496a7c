"""-m "not gpu": the vector passes fused into the interior solve of ApplyInverse against the separate kernels
(HYMLS_MI_NO_FUSED_IO=1) on the TEST-ONLY host simulators: tests/hostsim, and tests/f32_sim for FP32 panel storage.
This pins the host logic of LevelSolver::apply_inverse_mv (which launch gets which FusedIO, which passes are dropped,
the halo exchanges of the sharded path in between, the byte model); tests/test_fused_io_gpu.py runs the same checks on
the HIP kernels.  The checks are in tests/fused_io_cases.py."""
import os
import subprocess

import pytest

import hymls_amd
import fused_io_cases as fio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", fio.CASES, ids=fio.CASE_IDS)
def test_fused_io_equals_separate_kernels_sim(hostsim_lib, case):
    fio.check_equal(hostsim_lib, "cpu", case)


def test_classes_outside_the_fused_kernel_keep_the_separate_kernels_sim(hostsim_lib):
    """HYMLS_MI_NO_FUSED_SOLVE=1: no class is solved by the fused kernel, the condition is false, the old sequence runs"""
    fio.check_equal(hostsim_lib, "cpu", fio.STOKES16, env={"HYMLS_MI_NO_FUSED_SOLVE": "1"}, expect_fused=False)


def test_fused_io_sharded_sim(hostsim_lib):
    """2 gloo ranks: the exchanges sit between the two launches; same bits as the separate kernels on every rank, and the
    assembled result equals the one-rank one to the tolerance of tests/test_sharded.py"""
    res = fio.run_worker(2, fio.STOKES16, "hostsim", 29702)
    assert res["differ"] == 0 and res["repeat_differ"] == 0
    assert all(s > 0 for s in res["bytes_saved"])          # the fusion is on on every rank
    assert res["rel_err"] < 1e-12


@pytest.fixture(scope="module")
def f32sim(tmp_path_factory):
    out = tmp_path_factory.mktemp("f32_sim_fused_io")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "f32_sim"), "OUT=%s" % out])
    return hymls_amd.load_library(str(out / "libhymls_mi_f32_sim.so"))


def test_fused_io_with_fp32_panels_sim(f32sim):
    _, Pon, Poff = fio.check_equal(f32sim, "cpu", fio.STOKES16, storage="single")
    assert Pon.FactorStorage() == "single" and Poff.FactorStorage() == "single"
