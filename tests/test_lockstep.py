"""Lock-step columns of the native Krylov solver on CPU tensors through a TEST-ONLY simulator library
(tests/krylov_lockstep_sim: the sources of tests/krylov_border_sim plus plain-loop batched launchers and a plain-loop
multi-vector K x), built here in a temporary directory.  The checks are in tests/lockstep_cases.py;
tests/test_lockstep_gpu.py runs them on the product library.  On the simulator a batched launcher is the single-column
launcher called per column, so the bitwise checks pin the host state machine here; the batched kernels are pinned on the
GPU only."""
import json
import os
import subprocess
import sys

import pytest

import hymls_amd
import lockstep_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lsim(tmp_path_factory):
    out = tmp_path_factory.mktemp("krylov_lockstep_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_lockstep_sim"), "OUT=%s" % out])
    path = str(out / "libhymls_mi_krylov_lockstep_sim.so")
    return path, hymls_amd.load_library(path)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ks", cases.K_SETS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_orthogonalize_mv_sim(lsim, n, ks, f32):
    cases.check_orthogonalize_mv(lsim[1], "cpu", n, ks, f32)


def test_orthogonalize_mv_refusals_sim(lsim):
    cases.check_orthogonalize_mv_refusals(lsim[1], "cpu")


@pytest.mark.parametrize("name", ["laplace8", "stokes16", "oseen8"])
def test_matvec_mv_sim(lsim, name):
    cases.check_matvec_mv(lsim[1], "cpu", name)


@pytest.mark.parametrize("storage", ["double", "single"])
@pytest.mark.parametrize("nvec,width", [(5, 4), (3, 2)])
@pytest.mark.parametrize("start", ["Zero", "Random"])
@pytest.mark.parametrize("right", [True, False])
def test_gmres_lockstep_sim(lsim, right, start, nvec, width, storage):
    cases.check_gmres(lsim[1], "cpu", storage, right, start, nvec, width)


@pytest.mark.parametrize("storage", ["double", "single"])
@pytest.mark.parametrize("variant", ["maxit", "norestart"])
def test_gmres_lockstep_limits_sim(lsim, variant, storage):
    cases.check_gmres(lsim[1], "cpu", storage, True, "Zero", 5, 4, variant)


@pytest.mark.parametrize("width", [2, 4])
def test_cg_lockstep_sim(lsim, width):
    cases.check_cg(lsim[1], "cpu", width)


def test_previous_sim(lsim):
    cases.check_previous(lsim[1], "cpu")


def test_life_cycle_sim(lsim):
    cases.check_life_cycle(lsim[1], "cpu")


def test_bordered_ignores_width_sim(lsim):
    cases.check_bordered_ignores_width(lsim[1], "cpu")


def test_simulator_without_the_macro_returns_m99(tmp_path):
    """tests/krylov_sim, built from this tree without HYMLS_MI_LOCKSTEP_SOLVER and without batched launchers, still loads;
    a width above 1 and the three building blocks return -99"""
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_sim"), "OUT=%s" % tmp_path])
    cases.missing_launchers_return_m99(hymls_amd.load_library(str(tmp_path / "libhymls_mi_krylov_sim.so")))


def test_sharded_handle_is_refused_sim(lsim):
    """two ranks (torch.distributed.run, gloo): a lock-step solve and the three building blocks return -99 on every rank,
    and the plain width-1 solve still works"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29741", os.path.join(ROOT, "tests", "lockstep_worker.py")]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HYMLS_KRYLOV_SIM_LIB=lsim[0])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("LOCKSTEP_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("LOCKSTEP_RESULT "):])
    assert res["solve"] == [-99, -99] and res["blocks"] == [[-99, -99, -99]] * 2 and res["plain_ok"], res
