"""The native Krylov solver of include/hymls_mi_solver.h (hymls_amd.NativeSolver): restarted GMRES and CG in the library,
with the three-pass ICGS(2) orthogonalisation on the device.  -m "not gpu": CPU torch tensors through a TEST-ONLY
simulator library (tests/krylov_sim: the host simulator of tests/hostsim plus plain-loop versions of the solver's
launchers), built here in a temporary directory.  -m gpu: the product library on the MI355X.  The iteration counts
are checked against the oracle's Krylov loops and against hymls_amd.Solver on the same preconditioner."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hymls_amd
from hymls_amd.native_solver import orthogonalize
from common import problem, xml_params, product_prec, oracle_prec
from oracle import krylov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ksim_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("krylov_sim")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "tests", "krylov_sim"), "OUT=%s" % out])
    path = str(out / "libhymls_mi_krylov_sim.so")
    return path, hymls_amd.load_library(path)


def _system(lib, eq, n, sx, levels, part, seed):
    A, tv = problem(eq, n)
    P = product_prec(A, tv, xml_params(eq, n, sx, levels, -1, part), lib)
    b = A @ np.random.default_rng(seed).uniform(-1, 1, A.shape[0])
    return A, P, b, tv


def _relres(A, b, x):
    return np.linalg.norm(b - A @ x) / np.linalg.norm(b)


def _native(P, b, dev, prm):
    S = hymls_amd.NativeSolver(P, {"Solver": prm})
    x = S.ApplyInverse(torch.from_numpy(b).to(dev))
    return S, x.cpu().numpy()


def _python(P, b, dev, prm):
    S = hymls_amd.Solver(P, P, {"Solver": prm})
    x = S.ApplyInverse(torch.from_numpy(b).to(dev))
    return S, x.cpu().numpy()


def check_cg(lib, dev):
    # threeD1.xml shape: Laplace 32^3, sx = 4, 3-level, CG 1e-10
    A, P, b, tv = _system(lib, "Laplace", 32, 4, 2, "Cartesian", 3)
    O = oracle_prec(A, tv, "Laplace", 32, 4, 2)
    S, x = _native(P, b, dev, {"Krylov Method": "CG", "Iterative Solver": {"Convergence Tolerance": 1e-10, "Maximum Iterations": 100}})
    _, its_o, _ = krylov.pcg(lambda v: A @ v, b, O.apply_inverse, tol=1e-10, maxit=100)
    assert abs(S.getNumIter() - its_o) <= 1 and S.getNumIter() <= 35, (S.getNumIter(), its_o)
    assert _relres(A, b, x) < 1e-9


def check_gmres(lib, dev):
    # stokes1_3D.xml shape at 16^3: Stokes-C, Skew Cartesian, sx = 8, 1-level, GMRES 1e-8
    A, P, b, tv = _system(lib, "Stokes-C", 16, 8, 1, "Skew Cartesian", 6)
    prm = {"Krylov Method": "GMRES", "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 400, "Num Blocks": 250}}
    S, x = _native(P, b, dev, prm)
    O = oracle_prec(A, tv, "Stokes-C", 16, 8, 1, partitioner="Skew Cartesian")
    _, its_o, _ = krylov.gmres(lambda v: A @ v, b, O.apply_inverse, tol=1e-8, maxit=250)
    its = S.getNumIter()
    assert abs(its - its_o) <= 1 and its <= 130, (its, its_o)
    assert _relres(A, b, x) < 1e-7 and S.achievedTol() <= 1e-8
    Sp, xp = _python(P, b, dev, prm)
    assert abs(its - Sp.getNumIter()) <= 1, (its, Sp.getNumIter())
    prm["Iterative Solver"]["Num Blocks"] = 30
    S30, x30 = _native(P, b, dev, prm)
    assert S30.getNumIter() > its and _relres(A, b, x30) < 1e-7
    prm["Left or Right Preconditioning"] = "Left"
    prm["Iterative Solver"]["Num Blocks"] = 250
    SL, xl = _native(P, b, dev, prm)
    assert SL.getNumIter() <= 140


def check_not_converged(lib, dev):
    A, tv = problem("Laplace", 16)
    P = product_prec(A, tv, xml_params("Laplace", 16, 4, 1), lib)
    S = hymls_amd.NativeSolver(P, {"Krylov Method": "CG", "Iterative Solver": {"Convergence Tolerance": 1e-12, "Maximum Iterations": 2}})
    b = torch.ones(A.shape[0], dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError):
        S.ApplyInverse(b)
    assert S.getNumIter() == 2
    x = torch.empty_like(b)
    assert S._lib.hymls_mi_solver_solve(S._s, b.data_ptr(), b.numel(), x.data_ptr(), b.numel(), 1, 1) == -1
    assert S.getNumIter() == 2 and S.achievedTol() > 1e-12


def check_previous(lib, dev):
    # a solve capped at 5 iterations, then one to the tolerance from its result: both as hymls_amd.Solver
    A, P, b, _ = _system(lib, "Stokes-C", 16, 8, 1, "Skew Cartesian", 6)
    capped = {"Krylov Method": "GMRES", "Initial Vector": "Previous",
              "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 5, "Num Blocks": 250}}
    full = {"Krylov Method": "GMRES", "Initial Vector": "Previous",
            "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 400, "Num Blocks": 250}}
    its = []
    for S in (hymls_amd.NativeSolver(P, {"Solver": capped}), hymls_amd.Solver(P, P, {"Solver": capped})):
        with pytest.raises(RuntimeError):
            S.ApplyInverse(torch.from_numpy(b).to(dev))
        first = S.getNumIter()
        S.setParameterList({"Solver": full})
        x = S.ApplyInverse(torch.from_numpy(b).to(dev)).cpu().numpy()
        its.append((first, S.getNumIter()))
        assert _relres(A, b, x) < 1e-7
    (n1, n2), (p1, p2) = its
    assert n1 == p1 == 5 and abs(n2 - p2) <= 1, its


def cgs2_reference(V, w):
    h1 = V.T @ w
    w1 = w - V @ h1
    h2 = V.T @ w1
    w2 = w1 - V @ h2
    return h1 + h2, w2


def check_orthogonalize(lib, dev, n, k, ld, orthonormal=False):
    A, tv = problem("Laplace", 8)
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 1), testVector=tv, lib=lib)
    rng = np.random.default_rng(n * 1000 + k)
    if orthonormal:
        V = np.linalg.qr(rng.uniform(-1, 1, (n, k)))[0]
    else:
        V = rng.uniform(-1, 1, (n, k))
        V /= np.linalg.norm(V, axis=0)
    w = rng.uniform(-1, 1, n)
    # exactly (k - 1) * ld + n doubles: a read past the last column is not absorbed by padding
    flat = np.zeros((k - 1) * ld + n)
    for j in range(k):
        flat[j * ld:j * ld + n] = V[:, j]
    Vt = torch.from_numpy(flat).to(dev)
    wt = torch.from_numpy(w.copy()).to(dev)
    h, nrm = orthogonalize(P, n, k, Vt, ld, wt)
    h_ref, w_ref = cgs2_reference(V, w)
    wn = np.linalg.norm(w)
    # unit columns: the rounding of every product is bounded by eps |w|; with k > n the projections of a
    # non-orthonormal V grow the vectors, so the scale is the largest value involved
    scale = max(wn, np.abs(h_ref).max(), np.abs(w_ref).max())
    assert np.abs(h - h_ref).max() <= 1e-13 * scale, (n, k, ld)
    wo = wt.cpu().numpy()
    assert np.abs(wo - w_ref).max() <= 1e-12 * scale, (n, k, ld)
    assert abs(nrm - np.linalg.norm(w_ref)) <= 1e-12 * scale
    if orthonormal:
        assert np.linalg.norm(V.T @ wo) <= 1e-13 * max(np.linalg.norm(w), 1e-300)
    wt2 = torch.from_numpy(w.copy()).to(dev)
    h2, nrm2 = orthogonalize(P, n, k, Vt, ld, wt2)
    assert np.array_equal(h, h2) and nrm == nrm2 and torch.equal(wt, wt2)


def run_worker(world, args, mode, port, env_extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "native_solver_worker.py")]
    cmd += [str(a) for a in args] + [mode]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    env.update(env_extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("NSOLVE_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("NSOLVE_RESULT "):])


def check_sharded(res):
    assert all(abs(i - res["its_one_rank"]) <= 1 for i in res["its_sharded"]), res
    assert res["x_diff"] < 1e-8 and res["residual"] < 1e-7, res


# ---------------------------------------------------------------- simulator (-m "not gpu")
def test_native_cg_sim(ksim_lib):
    check_cg(ksim_lib[1], "cpu")


def test_native_gmres_sim(ksim_lib):
    check_gmres(ksim_lib[1], "cpu")


def test_native_not_converged_sim(ksim_lib):
    check_not_converged(ksim_lib[1], "cpu")


def test_native_previous_sim(ksim_lib):
    check_previous(ksim_lib[1], "cpu")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("k", [1, 2, 31, 33, 100, 251])
def test_orthogonalize_sim(ksim_lib, n, k):
    for ld in (n, n + 5):
        check_orthogonalize(ksim_lib[1], "cpu", n, k, ld)
    if k <= n:
        check_orthogonalize(ksim_lib[1], "cpu", n, k, n, orthonormal=True)


def test_orthogonalize_rejects_bad_shapes_sim(ksim_lib):
    A, tv = problem("Laplace", 8)
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 1), testVector=tv, lib=ksim_lib[1])
    V, w = torch.zeros(257 * 8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    with pytest.raises(hymls_amd.HymlsError):
        orthogonalize(P, 8, 257, V, 8, w)
    with pytest.raises(hymls_amd.HymlsError):
        orthogonalize(P, 8, 2, V, 7, w)


@pytest.mark.parametrize("world,method", [(2, "GMRES"), (4, "CG")])
def test_native_sharded_sim(ksim_lib, world, method):
    eq = "Stokes-C" if method == "GMRES" else "Laplace"
    part = "Skew Cartesian" if method == "GMRES" else "Cartesian"
    res = run_worker(world, (eq, 16, 4, 1, part, method), "sim", 29640 + world, {"HYMLS_KRYLOV_SIM_LIB": ksim_lib[0]})
    check_sharded(res)


def test_symbols_bound_lazily(hostsim_lib):
    # the existing simulator has no solver symbols and still loads; NativeSolver on it fails loudly
    assert not hasattr(hostsim_lib, "_hymls_solver_bound") or not hostsim_lib._hymls_solver_bound
    A, tv = problem("Laplace", 8)
    P = product_prec(A, tv, xml_params("Laplace", 8, 4, 1), hostsim_lib)
    with pytest.raises(AttributeError):
        hymls_amd.NativeSolver(P, {})


# ---------------------------------------------------------------- MI355X (-m gpu)
@pytest.mark.gpu
def test_orthogonalize_gpu(gpu_lib):
    for n in (1, 63, 64, 65, 4099, 2 ** 20 + 3):
        for k in (1, 2, 31, 32, 33, 100, 251):
            for ld in (n, n + 5):
                check_orthogonalize(gpu_lib, "cuda", n, k, ld)
            if k <= n and n < 2 ** 20:
                check_orthogonalize(gpu_lib, "cuda", n, k, n, orthonormal=True)


@pytest.mark.gpu
def test_native_cg_gpu(gpu_lib):
    check_cg(gpu_lib, "cuda")


@pytest.mark.gpu
def test_native_gmres_gpu(gpu_lib):
    check_gmres(gpu_lib, "cuda")


@pytest.mark.gpu
def test_native_not_converged_and_previous_gpu(gpu_lib):
    check_not_converged(gpu_lib, "cuda")
    check_previous(gpu_lib, "cuda")


@pytest.mark.gpu
def test_native_stokes64_gpu(gpu_lib):
    """Stokes3D 64^3, 3-level, GMRES(100): as hymls_amd.Solver, reproducible to the bit, host and device pointers alike,
    and nvec = 2 column by column equal to single solves"""
    A, P, b, _ = _system(gpu_lib, "Stokes-C", 64, 8, 2, "Skew Cartesian", 11)
    prm = {"Krylov Method": "GMRES", "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 1000,
                                                          "Num Blocks": 100, "Maximum Restarts": 40}}
    S = hymls_amd.NativeSolver(P, {"Solver": prm})
    bt = torch.from_numpy(b).cuda()
    x1 = S.ApplyInverse(bt)
    its = S.getNumIter()
    x2 = S.ApplyInverse(bt)
    assert torch.equal(x1, x2) and S.getNumIter() == its
    Sp = hymls_amd.Solver(P, P, {"Solver": prm})
    Sp.ApplyInverse(bt)
    assert abs(its - Sp.getNumIter()) <= 1, (its, Sp.getNumIter())
    x = x1.cpu().numpy()
    assert _relres(A, b, x) < 1e-7
    xh = S.ApplyInverse(b)                                   # on_device = 0
    assert np.array_equal(xh, x)
    b2 = A @ np.random.default_rng(12).uniform(-1, 1, A.shape[0])
    B = torch.from_numpy(np.stack([b, b2])).cuda()
    X = S.ApplyInverse(B)
    y2 = S.ApplyInverse(torch.from_numpy(b2).cuda())
    assert torch.equal(X[0], x1) and torch.equal(X[1], y2)


@pytest.mark.gpu
def test_native_solver_from_plain_c(gpu_lib, tmp_path):
    exe = str(tmp_path / "capi_solve")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi", "capi_solve.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "hymls_amd"), "-lhymls_mi", "-Wl,-rpath," + os.path.join(ROOT, "hymls_amd"), "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CAPI_SOLVE" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_native_sharded_gpu(gpu_lib):
    """two ranks sharing cuda:0 (gloo transport): the iteration count of one rank"""
    res = run_worker(2, ("Stokes-C", 16, 4, 1, "Skew Cartesian", "GMRES"), "gpu", 29662, {})
    check_sharded(res)
