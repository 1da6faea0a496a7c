"""-m "not gpu": FP32 storage of the merged level-solve panels ("MI Merged Factor Storage" = "single") on the TEST-ONLY
simulator tests/lvllab -- the simulator of tests/f32_sim compiled with the option's macro as well, plus plain-loop
versions of the two launchers it adds -- built here in a temporary directory.  This pins the host logic (slabs, the
table of the merged solve, lifecycle, byte figures, error codes); tests/test_merged_f32_gpu.py runs the same checks on
the HIP kernels.  The checks themselves are in tests/merged_f32_cases.py."""
import json
import os
import subprocess
import sys

import pytest

import hymls_amd
import merged_f32_cases as mc
from common import problem, xml_params, product_prec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def msim(tmp_path_factory):
    out = tmp_path_factory.mktemp("merged_f32_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "lvllab"), "simlib", "OUT=%s" % out])
    path = str(out / "libhymls_mi_merged_f32_sim.so")
    return path, hymls_amd.load_library(path)


@pytest.mark.parametrize("run", mc.RUNS, ids=mc.RUN_IDS)
def test_bitwise_against_rounded_fp64_panels_sim(msim, run):
    mc.check_run(msim[1], "cpu", run)


def test_defaults_untouched_sim(msim):
    mc.check_defaults(msim[1], "cpu")


def test_lifecycle_sim(msim):
    mc.check_lifecycle(msim[1], "cpu")


def test_overflow_guard_sim(msim):
    mc.check_overflow(msim[1], "cpu")


def test_python_and_xml_sim(msim, tmp_path):
    mc.check_python_and_xml(msim[1], "cpu", tmp_path)


def test_solver_sim(msim):
    mc.check_solver(msim[1], "cpu")


def test_build_without_the_level_kernels_refuses(hostsim_lib):
    """the unchanged simulator of tests/hostsim is built without the macro: both symbols exist, 32 is refused with -99"""
    A, tv = problem("Laplace", 8)
    P = product_prec(A, tv, xml_params("Laplace", 8, 4, 1), hostsim_lib)
    assert hostsim_lib.hymls_mi_merged_factor_storage(P._h) == 64
    assert hostsim_lib.hymls_mi_set_merged_factor_storage(P._h, 32) == -99
    assert "FP32" in hostsim_lib.hymls_mi_last_error(P._h).decode()
    assert hostsim_lib.hymls_mi_set_merged_factor_storage(P._h, 64) == 0
    assert hostsim_lib.hymls_mi_set_merged_factor_storage(P._h, 16) == -2
    assert hostsim_lib.hymls_mi_merged_factor_storage(P._h) == 64 and P.IsComputed()
    assert P.apply_bytes(10) == 0       # (every class of this problem is solved by the fused kernel)


def test_adapter_key_sim(msim, tmp_path):
    """include/hymls_mi_epetra.hpp reads "MI Merged Factor Storage" in SetParameters and passes it on at Initialize"""
    exe = str(tmp_path / "adapter_merged_storage")
    libdir = os.path.dirname(msim[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "mock_epetra"),
                           os.path.join(ROOT, "tests", "mock_epetra", "adapter_merged_storage.cpp"), "-o", exe,
                           "-L", libdir, "-lhymls_mi_merged_f32_sim", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, HYMLS_MI_NO_FUSED_SOLVE="1"))
    assert out.returncode == 0 and "ADAPTER_MERGED_STORAGE_OK" in out.stdout, out.stdout + out.stderr


def test_sharded_sim(msim):
    """2 gloo ranks, Stokes-C 16^3 with every class on the merged route, FP32 merged storage on every rank: the assembled
    result equals one rank in FP32 merged storage to the tolerance tests/test_sharded.py uses for FP64 storage"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29689", os.path.join(ROOT, "tests", "merged_f32_dist_worker.py"), msim[0]]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HYMLS_MI_NO_FUSED_SOLVE="1")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("MERGED_F32_DIST_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("MERGED_F32_DIST_RESULT "):])
    print(res)
    assert res["cover_ok"] and res["storage"] == ["single", "single"]
    assert res["rel_err"] < 1e-12
    assert 0.0 < res["rel_to_double"] < mc.CAP
    assert res["bytes10_64"] > 0 and res["bytes10_ratio"] == 0.5


def test_all_instantiations_in_the_code_object():
    """(reads the product library that build() makes; no GPU needed) the gfx950 code object of the product library holds the double and the float
    form of both level kernels for NV = 1, 2 and 4, the float form with 8 and with 16 columns per step (mangled names:
    ...k_lvl_fwdILi4EdLb0EE / ...ILi4EfLb0EE / ...ILi4EfLb1EE)"""
    with open(os.path.join(ROOT, "hymls_amd", "libhymls_mi.so"), "rb") as f:
        blob = f.read()
    for sweep in (b"fwd", b"bwd"):
        for nv in (b"1", b"2", b"4"):
            for pt in (b"dLb0", b"fLb0", b"fLb1"):
                name = b"k_lvl_" + sweep + b"ILi" + nv + b"E" + pt + b"EE"
                assert name in blob, name
