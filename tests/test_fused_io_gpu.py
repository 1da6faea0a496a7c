"""-m gpu: the vector passes fused into the interior solve of ApplyInverse (k_interior_fused_io<.., 1, 0> and <.., 2, 1>)
against the separate k_gather / k_spmv / k_axpby / k_scatter kernels (HYMLS_MI_NO_FUSED_IO=1) on the MI355X: equal bits
on every case of tests/fused_io_cases.py, with FP32 panel storage, sharded, and the oracle comparison of
tests/test_gpu_parity.py with the fusion on."""
import numpy as np
import pytest

import fused_io_cases as fio
from common import problem, oracle_prec, rel_diff

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", fio.CASES, ids=fio.CASE_IDS)
def test_fused_io_equals_separate_kernels_gpu(gpu_lib, case):
    """the A12 rows of these levels average 1.4 to 75 entries, so every lane count of the SpMV (1, 2, 8) is compared"""
    A, Pon, _ = fio.check_equal(gpu_lib, "cuda", case)
    eq, n, sx, levels, cx, part = case
    _, tv = problem(eq, n)
    O = oracle_prec(A, tv, eq, n, sx, levels, cx, partitioner=part)
    b = np.random.default_rng(42).uniform(-1, 1, A.shape[0])
    d = rel_diff(fio.apply(Pon, b, "cuda"), O.apply_inverse(b))
    print("  fusion on against the oracle: rel. diff %.3e" % d, flush=True)
    assert d < 1e-8


def test_classes_outside_the_fused_kernel_keep_the_separate_kernels_gpu(gpu_lib):
    fio.check_equal(gpu_lib, "cuda", fio.STOKES16, env={"HYMLS_MI_NO_FUSED_SOLVE": "1"}, expect_fused=False)


@pytest.mark.parametrize("case", [fio.STOKES16, fio.STOKES32], ids=fio.CASE_IDS[:2])
def test_fused_io_with_fp32_panels_gpu(gpu_lib, case):
    _, Pon, Poff = fio.check_equal(gpu_lib, "cuda", case, storage="single")
    assert Pon.FactorStorage() == "single" and Poff.FactorStorage() == "single"


def test_fused_io_sharded_gpu(gpu_lib):
    """2 ranks sharing the card, gloo staging (as tests/test_gpu_parity.py::test_sharded_matches_single_gpu)"""
    res = fio.run_worker(2, fio.STOKES16, "gpu", 29712)
    assert res["differ"] == 0 and res["repeat_differ"] == 0
    assert all(s > 0 for s in res["bytes_saved"])
    assert res["rel_err"] < 1e-12
