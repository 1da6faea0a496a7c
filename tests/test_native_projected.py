"""The projection vectors of the native Krylov solver (hymls_mi_solver_set_projection, hymls_mi_oblique_project,
hymls_amd.NativeSolver.setProjectionVectors) on CPU tensors through a TEST-ONLY simulator library (tests/krylov_proj_sim:
the sources of tests/krylov_lockstep_sim plus plain-loop projection launchers with the kernels' decomposition), built here
in a temporary directory.  The checks themselves are in tests/native_projected_cases.py;
tests/test_native_projected_gpu.py runs them on the product library."""
import json
import os
import subprocess
import sys

import pytest

import hymls_amd
import native_projected_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def psim(tmp_path_factory):
    out = tmp_path_factory.mktemp("krylov_proj_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_proj_sim"), "OUT=%s" % out])
    path = str(out / "libhymls_mi_krylov_proj_sim.so")
    return path, hymls_amd.load_library(path)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_oblique_project_sim(psim, n):
    cases.check_oblique_project(psim[1], "cpu", n)


def test_oblique_project_refusals_sim(psim):
    cases.check_oblique_project_refusals(psim[1], "cpu")


@pytest.mark.parametrize("with_b", [False, True])
def test_unit_properties_sim(psim, with_b):
    cases.check_unit_properties(psim[1], "cpu", with_b)


def test_set_projection_refusals_sim(psim):
    cases.check_set_projection_refusals(psim[1], "cpu")


@pytest.mark.parametrize("lor", ["Right", "Left"])
@pytest.mark.parametrize("with_b", [False, True])
def test_exact_sim(psim, with_b, lor):
    cases.check_exact(psim[1], "cpu", with_b, lor)


@pytest.mark.parametrize("name", ["laplace", "stokes"])
def test_inexact_sim(psim, name):
    cases.check_inexact(psim[1], "cpu", name)


def test_variants_sim(psim):
    cases.check_variants(psim[1], "cpu")


def test_life_cycle_sim(psim):
    cases.check_life_cycle(psim[1], "cpu")


def test_sharded_handle_is_refused_sim(psim):
    """two ranks (torch.distributed.run, gloo, as tests/dist_worker.py): a solve with projection vectors returns -99 on
    every rank, and the plain sharded solve works once they are removed"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29741", os.path.join(ROOT, "tests", "native_projected_worker.py")]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HYMLS_KRYLOV_SIM_LIB=psim[0])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("NPROJ_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("NPROJ_RESULT "):])
    assert res["set"] == [0, 0] and res["codes"] == [-99, -99] and res["plain_ok"], res


def test_simulator_without_the_macro_returns_m99(tmp_path):
    """tests/krylov_sim, built from this tree without HYMLS_MI_PROJECTED_SOLVER and without the projection launchers, still
    loads, and every new symbol returns -99"""
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_sim"), "OUT=%s" % tmp_path])
    cases.missing_symbols_return_m99(hymls_amd.load_library(str(tmp_path / "libhymls_mi_krylov_sim.so")))
