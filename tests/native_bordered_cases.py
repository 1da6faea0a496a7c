"""Checks of the bordered solve of the native Krylov solver (hymls_mi_solver_solve_bordered, hymls_mi_border_product,
hymls_amd.NativeBorderedSolver), shared by tests/test_native_bordered.py (the TEST-ONLY simulator of
tests/krylov_border_sim, CPU tensors) and tests/test_native_bordered_gpu.py (the product library on the MI355X).
Every check takes (lib, dev)."""
import functools
import os

import numpy as np
import pytest
import torch

import hymls_amd
from hymls_amd.native_solver import border_product, bind_bordered
from common import problem, xml_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
BORDER_M = (1, 2, 7, 8, 9, 32)


def small_prec(lib):
    A, tv = problem("Laplace", 8)
    return hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 1), testVector=tv, lib=lib)


def _flat(cols, m, ld):
    """columns 0..m-1 of cols (n x 32) with leading dimension ld in exactly (m - 1) * ld + n doubles: a read past the last
    column is not absorbed by padding"""
    n = cols.shape[0]
    flat = np.zeros((m - 1) * ld + n)
    for j in range(m):
        flat[j * ld:j * ld + n] = cols[:, j]
    return flat


# ---------------------------------------------------------------- 1. the border product alone
def check_border_product(lib, dev, n):
    """against numpy in extended precision (np.longdouble, column by column), so that the bounds only have to cover the
    error of the kernel: head (m + 2) u (|y| + sum_j |V_ij s_j|), a sum of m products and one add in any order;
    tail (n + m + 1) u (sum_i |W_ij x_i| + sum_l |C_jl s_l|), a sum of n + m products in any order.  u = 2^-53."""
    P = small_prec(lib)
    rng = np.random.default_rng(1000 + n % 9973)
    mmax = max(BORDER_M)
    Vc, Wc = rng.uniform(-1, 1, (n, mmax)), rng.uniform(-1, 1, (n, mmax))
    x, s, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, mmax), rng.uniform(-1, 1, n)
    Cf = rng.uniform(-1, 1, (mmax, mmax))
    # references for every m at once: s and C of a smaller m are the leading part of the largest
    L = np.longdouble
    head, ahead = y0.astype(L), np.abs(y0)
    heads, aheads = {}, {}
    wx, awx = np.zeros(mmax, L), np.zeros(mmax)
    xl = x.astype(L)
    for j in range(mmax):
        head = head + Vc[:, j].astype(L) * L(s[j])
        ahead = ahead + np.abs(Vc[:, j] * s[j])
        wx[j] = (Wc[:, j].astype(L) * xl).sum()
        awx[j] = np.abs(Wc[:, j] * x).sum()
        if j + 1 in BORDER_M:
            heads[j + 1], aheads[j + 1] = head.copy(), ahead.copy()
    for m in BORDER_M:
        z = torch.from_numpy(np.concatenate([x, s[:m]])).to(dev)
        for ld in (n, n + 5):
            Vt, Wt = torch.from_numpy(_flat(Vc, m, ld)).to(dev), torch.from_numpy(_flat(Wc, m, ld)).to(dev)
            for Cm in (Cf[:m, :m], None):
                outs = []
                for _ in range(2):
                    y = torch.from_numpy(np.concatenate([y0, np.full(m, np.nan)])).to(dev)   # the tail is written, not added to
                    border_product(P, n, m, Vt, ld, Wt, ld, Cm, z, y)
                    outs.append(y.cpu().numpy())
                assert np.array_equal(outs[0], outs[1]), (n, m, ld)                          # two calls: the same bits
                got = outs[0]
                assert (np.abs(got[:n].astype(L) - heads[m]) <= (m + 2) * U * aheads[m]).all(), (n, m, ld)
                tail = wx[:m].copy()
                atail = awx[:m].copy()
                if Cm is not None:
                    tail = tail + Cm.astype(L) @ s[:m].astype(L)
                    atail = atail + np.abs(Cm) @ np.abs(s[:m])
                assert (np.abs(got[n:].astype(L) - tail) <= (n + m + 1) * U * atail).all(), (n, m, ld, got[n:], tail)


def check_border_product_refusals(lib, dev):
    P = small_prec(lib)
    n = 64
    V = torch.zeros(33 * n, dtype=torch.float64, device=dev)
    z, y = torch.zeros(n + 33, dtype=torch.float64, device=dev), torch.zeros(n + 33, dtype=torch.float64, device=dev)
    for args in ((n, 0, V, n, V, n, None, z, y), (n, 33, V, n, V, n, None, z, y), (n, 2, V, n - 1, V, n, None, z, y),
                 (n, 2, V, n, V, n - 1, None, z, y), (n, 2, None, n, V, n, None, z, y), (n, 2, V, n, None, n, None, z, y),
                 (n, 2, V, n, V, n, None, None, y), (n, 2, V, n, V, n, None, z, None)):
        with pytest.raises(hymls_amd.HymlsError) as e:
            border_product(P, *args)
        assert e.value.code == -2, args[:2]
    border_product(P, n, 2, V, n, V, n, None, z, y)        # and the valid call next to them passes


# ---------------------------------------------------------------- helpers of the solves
def _aug_residual(A, V, W, Cm, b, t, x, s):
    r = np.concatenate([b - A @ x - V @ s, t - W.T @ x - Cm @ s])
    return np.linalg.norm(r) / np.linalg.norm(np.concatenate([b, t]))


def _prm(tol=1e-8, maxit=300, blocks=250, **sol):
    d = {"Krylov Method": "GMRES", "Iterative Solver": {"Convergence Tolerance": tol, "Maximum Iterations": maxit, "Num Blocks": blocks}}
    d.update(sol)
    return d


def _python_count(P, V, W, Cm, b, t, dev, prm):
    S = hymls_amd.BorderedSolver(P, P, prm)
    # (the border of P is set already: only the operator's copy is needed)
    S._V, S._W, S._C = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (V, W, Cm))
    S.ApplyInverse(torch.from_numpy(b).to(dev), t)
    return S.getNumIter()


# ---------------------------------------------------------------- 2. exactness
def check_exact(lib, dev, with_c):
    """the reference's BorderedApplyInverse unit test as a solve: a one-level preconditioner is the exact bordered solve"""
    A, tv = problem("Laplace", 8)
    N, m = A.shape[0], 2
    rng = np.random.default_rng(41)
    V, W = rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (N, m))
    Cm = rng.uniform(-1, 1, (m, m)) if with_c else None
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 0), testVector=tv, lib=lib)
    P.Initialize()
    S = hymls_amd.NativeBorderedSolver(P, _prm(tol=1e-10))
    assert S.SetBorder(V, W, Cm) == 0
    P.Compute()
    x_ex, s_ex = rng.uniform(-1, 1, N), (rng.uniform(-1, 1, m) if with_c else np.zeros(m))
    b = A @ x_ex + V @ s_ex
    t = W.T @ x_ex + (Cm @ s_ex if with_c else 0.0)
    x, s = S.ApplyInverse(torch.from_numpy(b).to(dev), t)
    assert S.getNumIter() == 1
    assert np.abs(x.cpu().numpy() - x_ex).max() < 1e-10 and np.abs(s - s_ex).max() < 1e-10
    if not with_c:
        # T = None is T = 0; S may be dropped (a null pointer in C)
        b0 = A @ x_ex
        bt = torch.from_numpy(b0).to(dev)
        x1, s1 = S.ApplyInverse(bt, np.zeros(m))
        x2, s2 = S.ApplyInverse(bt)
        assert torch.equal(x1, x2) and np.array_equal(s1, s2)
        x3 = torch.empty_like(bt)
        assert S._lib.hymls_mi_solver_solve_bordered(S._s, bt.data_ptr(), None, x3.data_ptr(), None, 1) == 0
        assert torch.equal(x1, x3)


# ---------------------------------------------------------------- 3. Stokes-C 16^3, random border
@functools.lru_cache(maxsize=None)
def stokes_random_border():
    """the system of tests/test_bordered.py::bordered_krylov (seed 43) and the iteration count of the oracle's loop"""
    from oracle import krylov
    from oracle.partition import Params
    from oracle.hymls import Preconditioner as OraclePrec
    eq, n, sx, levels, part = "Stokes-C", 16, 8, 1, "Skew Cartesian"
    A, tv = problem(eq, n)
    N, m = A.shape[0], 2
    rng = np.random.default_rng(43)
    V, W, Cm = rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (m, m))
    x_ex, s_ex = rng.uniform(-1, 1, N), rng.uniform(-1, 1, m)
    b, t = A @ x_ex + V @ s_ex, W.T @ x_ex + Cm @ s_ex
    O = OraclePrec(A, Params(nx=n, ny=n, nz=n, sx=sx, levels=levels, equations=eq, partitioner=part).finalize(), testvector=tv)
    O.set_border(V, W, Cm)
    O.compute()

    def op(z):
        return np.concatenate([A @ z[:N] + V @ z[N:], W.T @ z[:N] + Cm @ z[N:]])

    def pr(z):
        xx, ss = O.apply_inverse_bordered(z[:N], z[N:])
        return np.concatenate([xx, ss])

    _, its_o, _ = krylov.gmres(op, np.concatenate([b, t]), pr, tol=1e-8, maxit=300)
    return A, tv, V, W, Cm, b, t, its_o


def check_stokes_random_border(lib, dev):
    """"Num Blocks" 300 for the oracle's loop and for hymls_amd.BorderedSolver; the native solver takes at most
    HYMLS_MI_SOLVER_MAX_BLOCKS = 256 columns and gets 256: no loop restarts before the ~117 iterations are done"""
    A, tv, V, W, Cm, b, t, its_o = stokes_random_border()
    P = hymls_amd.Preconditioner(A, xml_params("Stokes-C", 16, 8, 1, -1, "Skew Cartesian"), testVector=tv, lib=lib)
    P.Initialize()
    S = hymls_amd.NativeBorderedSolver(P, _prm(blocks=256))
    S.SetBorder(V, W, Cm)
    P.Compute()
    bt = torch.from_numpy(b).to(dev)
    x, s = S.ApplyInverse(bt, t)
    its = S.getNumIter()
    its_p = _python_count(P, V, W, Cm, b, t, dev, _prm(blocks=300))
    print("Stokes-C 16^3 random border: native %d, oracle %d, BorderedSolver %d iterations" % (its, its_o, its_p))
    assert abs(its - its_o) <= 1, (its, its_o)
    assert abs(its - its_p) <= 1, (its, its_p)
    xn = x.cpu().numpy()
    assert np.linalg.norm(A @ xn + V @ s - b) <= 1e-7 * np.linalg.norm(b) and np.abs(W.T @ xn + Cm @ s - t).max() < 1e-6
    assert S.achievedTol() <= 1e-8 and S.getNumRestarts() == 0
    x2, s2 = S.ApplyInverse(bt, t)                      # a second identical solve: the same bits
    assert torch.equal(x, x2) and np.array_equal(s, s2) and S.getNumIter() == its
    xh, sh = S.ApplyInverse(b, t)                       # host pointers
    assert np.array_equal(xh, xn) and np.array_equal(sh, s) and S.getNumIter() == its


# ---------------------------------------------------------------- 4. singular Stokes-C, constant-pressure border
def check_singular_stokes(lib, dev):
    eq, n, sx, part = "Stokes-C", 16, 8, "Skew Cartesian"
    A, tv = problem(eq, n)
    N = A.shape[0]
    v = np.zeros((N, 1)); v[3::4, 0] = 1.0
    Cz = np.zeros((1, 1))
    P = hymls_amd.Preconditioner(A, xml_params(eq, n, sx, 1, -1, part, extra={"Fix Pressure Level": False}), testVector=tv, lib=lib)
    P.Initialize()
    S = hymls_amd.NativeBorderedSolver(P, _prm(blocks=250))
    S.SetBorder(v)
    P.Compute()
    rng = np.random.default_rng(44)
    x_ex, s_ex = rng.uniform(-1, 1, N), rng.uniform(-1, 1, 1)
    b, t = A @ x_ex + v @ s_ex, v.T @ x_ex
    bt = torch.from_numpy(b).to(dev)
    for blocks, min_restarts in ((250, 0), (30, 3)):
        prm = _prm(blocks=blocks, **{"Left or Right Preconditioning": "Right"})
        S.setParameterList(prm)
        x, s = S.ApplyInverse(bt, t)
        its, its_p = S.getNumIter(), _python_count(P, v, v, Cz, b, t, dev, prm)
        print("singular Stokes-C 16^3, Num Blocks %d: native %d, BorderedSolver %d iterations, %d restarts"
              % (blocks, its, its_p, S.getNumRestarts()))
        assert abs(its - its_p) <= 1, (blocks, its, its_p)
        assert S.getNumRestarts() >= min_restarts
        assert _aug_residual(A, v, v, Cz, b, t, x.cpu().numpy(), s) <= 1e-7
    # not converged: -1 from C, RuntimeError from Python; X and S hold the last iterate
    S.setParameterList(_prm(maxit=20, blocks=250))
    X, Sb = torch.full_like(bt, np.nan), np.full(1, np.nan)
    with pytest.raises(RuntimeError):
        S.ApplyInverse(bt, t, X=X, S=Sb)
    assert S.getNumIter() == 20
    res = _aug_residual(A, v, v, Cz, b, t, X.cpu().numpy(), Sb)
    print("singular Stokes-C 16^3 after 20 iterations: relative residual %.3e" % res)
    assert np.isfinite(X.cpu().numpy()).all() and np.isfinite(Sb).all() and res < 1.0
    tc = np.ascontiguousarray(t)
    assert S._lib.hymls_mi_solver_solve_bordered(S._s, bt.data_ptr(), tc.ctypes.data, X.data_ptr(), Sb.ctypes.data, 1) == -1
    assert S.getNumIter() == 20 and S.achievedTol() > 1e-8


# ---------------------------------------------------------------- 5. Laplace 16^3, random border
def _laplace_system(lib, dev):
    A, tv = problem("Laplace", 16)
    N, m = A.shape[0], 2
    rng = np.random.default_rng(45)
    V, W, Cm = rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (m, m))
    x_ex, s_ex = rng.uniform(-1, 1, N), rng.uniform(-1, 1, m)
    b, t = A @ x_ex + V @ s_ex, W.T @ x_ex + Cm @ s_ex
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 16, 4, 1), testVector=tv, lib=lib)
    P.Initialize()
    P.SetBorder(V, W, Cm)
    P.Compute()
    return A, V, W, Cm, b, t, P, torch.from_numpy(b).to(dev)


def check_previous_repeat(lib, dev):
    """with a "Previous" start a repeated solve of the same system takes 0 iterations: the start vector already has a true
    residual within the tolerance of |[b; t]| and is returned as it is.  (hymls_amd.BorderedSolver has no such test and
    iterates again, 28 times after 26, relative to the tiny first residual of the repeated solve.)"""
    A, V, W, Cm, b, t, P, bt = _laplace_system(lib, dev)
    S = hymls_amd.NativeBorderedSolver(P, _prm(**{"Initial Vector": "Previous"}))
    x, s = S.ApplyInverse(bt, t)
    first = S.getNumIter()
    x2, s2 = S.ApplyInverse(bt, t)
    print("Previous start: first solve %d iterations, repeated solve %d" % (first, S.getNumIter()))
    assert first > 0 and S.getNumIter() == 0
    assert torch.equal(x, x2) and np.array_equal(s, s2) and S.achievedTol() <= 1e-8
    assert _aug_residual(A, V, W, Cm, b, t, x2.cpu().numpy(), s2) <= 1e-8
    # another right-hand side: the previous solution does not solve it, and the iteration runs from there
    x3, s3 = S.ApplyInverse(2.0 * bt + 1.0, t)
    assert S.getNumIter() > 0
    assert _aug_residual(A, V, W, Cm, 2.0 * b + 1.0, t, x3.cpu().numpy(), s3) <= 1e-7


def check_laplace_variants(lib, dev):
    A, V, W, Cm, b, t, P, bt = _laplace_system(lib, dev)

    def res(x, s):
        return _aug_residual(A, V, W, Cm, b, t, x.cpu().numpy(), s)

    for lor, blocks in (("Right", 250), ("Left", 250), ("Right", 10)):
        prm = _prm(blocks=blocks, **{"Left or Right Preconditioning": lor})
        S = hymls_amd.NativeBorderedSolver(P, prm)
        x, s = S.ApplyInverse(bt, t)
        its, its_p = S.getNumIter(), _python_count(P, V, W, Cm, b, t, dev, prm)
        print("Laplace 16^3 %s, Num Blocks %d: native %d, BorderedSolver %d iterations" % (lor, blocks, its, its_p))
        assert abs(its - its_p) <= 1, (lor, blocks, its, its_p)
        assert res(x, s) <= 1e-7
        assert (S.getNumRestarts() > 0) == (blocks == 10)
    # "Previous" after a solve that was cut short: the iteration goes on from its last iterate, relative to the first
    # residual of the new solve, as hymls_amd.BorderedSolver does
    capped = _prm(maxit=5, **{"Initial Vector": "Previous"})
    full = _prm(**{"Initial Vector": "Previous"})
    S = hymls_amd.NativeBorderedSolver(P, capped)
    Sp = hymls_amd.BorderedSolver(P, P, capped)
    Sp._V, Sp._W, Sp._C = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (V, W, Cm))
    counts = []
    for solver in (S, Sp):
        with pytest.raises(RuntimeError):
            solver.ApplyInverse(bt, t)
        first = solver.getNumIter()
        solver.setParameterList(full)
        x, s = solver.ApplyInverse(bt, t)
        counts.append((first, solver.getNumIter()))
        assert res(x, s) <= 1e-7
    assert counts[0][0] == counts[1][0] == 5 and abs(counts[0][1] - counts[1][1]) <= 1, counts
    # "Random": converges, and two solvers with the same seed give the same bits
    outs = []
    for _ in range(2):
        S = hymls_amd.NativeBorderedSolver(P, _prm(**{"Initial Vector": "Random", "Random Seed": 7}))
        x, s = S.ApplyInverse(bt, t)
        assert res(x, s) <= 1e-7 and S.getNumIter() > 0
        outs.append((x, s, S.getNumIter()))
    assert torch.equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    # FP32 basis: the explicitly computed augmented residual reaches the tolerance (numpy's residual differs from the
    # solver's own by rounding only: 1e-12 is far above N u cond)
    S = hymls_amd.NativeBorderedSolver(P, _prm(**{"MI Basis Storage": "single"}))
    assert S.getBasisStorage() == "single"
    x, s = S.ApplyInverse(bt, t)
    print("Laplace 16^3 FP32 basis: %d iterations, achieved %.3e, numpy residual %.3e" % (S.getNumIter(), S.achievedTol(), res(x, s)))
    assert S.achievedTol() <= 1e-8 and res(x, s) <= 1e-8 + 1e-12


# ---------------------------------------------------------------- 6. life cycle and refusals
def check_life_cycle(lib, dev):
    A, tv = problem("Laplace", 8)
    N = A.shape[0]
    rng = np.random.default_rng(46)
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 0), testVector=tv, lib=lib)
    P.Initialize()
    S = hymls_amd.NativeBorderedSolver(P, _prm(tol=1e-10))
    x_ex = rng.uniform(-1, 1, N)
    for m in (2, 3, 1):                                  # another m re-sizes the buffers
        V, W, Cm = rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (m, m))
        s_ex = rng.uniform(-1, 1, m)
        S.SetBorder(V, W, Cm)
        P.Compute()
        b, t = A @ x_ex + V @ s_ex, W.T @ x_ex + Cm @ s_ex
        bt = torch.from_numpy(b).to(dev)
        x, s = S.ApplyInverse(bt, t)
        assert S.getNumIter() == 1 and np.abs(x.cpu().numpy() - x_ex).max() < 1e-10 and np.abs(s - s_ex).max() < 1e-10
    # the plain entry keeps refusing the bordered handle
    xo = torch.empty_like(bt)
    assert S._lib.hymls_mi_solver_solve(S._s, bt.data_ptr(), N, xo.data_ptr(), N, 1, 1) == -2
    # CG: the bordered operator is indefinite
    Scg = hymls_amd.NativeBorderedSolver(P, {"Krylov Method": "CG"})
    assert Scg._lib.hymls_mi_solver_solve_bordered(Scg._s, bt.data_ptr(), None, xo.data_ptr(), None, 1) == -99
    with pytest.raises(hymls_amd.HymlsError) as e:
        Scg.ApplyInverse(bt)
    assert e.value.code == -99
    # without the border: the plain solve, bit for bit, and the plain entry works again
    S.SetBorder(None)
    P.Compute()
    sb = np.full(1, 7.0)
    bp = torch.from_numpy(A @ x_ex).to(dev)
    x, s = S.ApplyInverse(bp)
    assert s.size == 0
    xc = torch.empty_like(bp)
    assert S._lib.hymls_mi_solver_solve_bordered(S._s, bp.data_ptr(), None, xc.data_ptr(), sb.ctypes.data, 1) == 0 and sb[0] == 7.0
    Sn = hymls_amd.NativeSolver(P, _prm(tol=1e-10))
    xn = Sn.ApplyInverse(bp)
    assert torch.equal(x, xn) and torch.equal(xc, xn) and S.getNumIter() == Sn.getNumIter()
    assert S._lib.hymls_mi_solver_solve(S._s, bp.data_ptr(), N, xo.data_ptr(), N, 1, 1) == 0 and torch.equal(xo, xn)
    assert np.abs(xn.cpu().numpy() - x_ex).max() < 1e-10


def check_too_many_border_columns(lib, dev):
    A, tv = problem("Laplace", 8)
    N, m = A.shape[0], 33
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 0), testVector=tv, lib=lib)
    P.Initialize()
    S = hymls_amd.NativeBorderedSolver(P, _prm())
    S.SetBorder(np.random.default_rng(47).uniform(-1, 1, (N, m)), None, np.eye(m))
    P.Compute()
    with pytest.raises(hymls_amd.HymlsError) as e:
        S.ApplyInverse(torch.ones(N, dtype=torch.float64, device=dev))
    assert e.value.code == -2


# ---------------------------------------------------------------- 7. the reference's stokes4_3D.xml through the driver
NATIVE_OVERLAY = """<ParameterList name="native solver">
  <ParameterList name="Solver">
    <Parameter name="MI Native Solver" type="bool" value="true"/>
  </ParameterList>
</ParameterList>
"""


def check_driver(lib, dev, tmp_path):
    from hymls_amd import driver
    ov = tmp_path / "native.xml"
    ov.write_text(NATIVE_OVERLAY)
    seen = []
    orig = hymls_amd.native_solver.NativeBorderedSolver.ApplyInverse

    def spy(self, *a, **k):
        seen.append(type(self).__name__)
        return orig(self, *a, **k)

    hymls_amd.native_solver.NativeBorderedSolver.ApplyInverse = spy
    try:
        out = driver.run(os.path.join(ROOT, "tests", "golden", "stokes4_3D.xml"), str(ov), lib=lib, device=dev)
    finally:
        hymls_amd.native_solver.NativeBorderedSolver.ApplyInverse = orig
    assert seen == ["NativeBorderedSolver"]
    assert out["iterations"] == 1
    assert out["relative_residual"] <= 5e-11 and out["relative_error"] <= 5e-11


def missing_symbols_return_m99(lib):
    """a library whose krylov.cpp was built without HYMLS_MI_BORDERED_SOLVER has both symbols, and both return -99"""
    bind_bordered(lib)
    P = small_prec(lib)
    P.Initialize()
    P.Compute()
    S = hymls_amd.NativeBorderedSolver(P, _prm())
    b = torch.ones(P._n, dtype=torch.float64)
    x = torch.empty_like(b)
    assert lib.hymls_mi_solver_solve_bordered(S._s, b.data_ptr(), None, x.data_ptr(), None, 1) == -99
    V = torch.zeros(2 * 8, dtype=torch.float64)
    z, y = torch.zeros(10, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)
    assert lib.hymls_mi_border_product(P._h, 8, 2, V.data_ptr(), 8, V.data_ptr(), 8, None, z.data_ptr(), y.data_ptr()) == -99
    assert S._lib.hymls_mi_solver_solve(S._s, b.data_ptr(), P._n, x.data_ptr(), P._n, 1, 1) == 0      # the plain solve is untouched
