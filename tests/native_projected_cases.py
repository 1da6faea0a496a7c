"""Checks of the projection vectors of the native Krylov solver (hymls_mi_solver_set_projection, hymls_mi_oblique_project,
hymls_amd.NativeSolver.setProjectionVectors), shared by tests/test_native_projected.py (the TEST-ONLY simulator of
tests/krylov_proj_sim, CPU tensors) and tests/test_native_projected_gpu.py (the product library on the MI355X).
Every check takes (lib, dev).  The references are numpy restatements of the formulas

    operator         y = (I - BV V') K (I - V BV') x
    preconditioner   y = M^-1 (I - BV H^-1 BV' M^-1) x,   H = BV' M^-1 BV
    primitive        y = x - P (G (Q' x))
"""
import functools
import os

import numpy as np
import pytest
import torch

import hymls_amd
from hymls_amd.native_solver import bind_bordered, bind_projection, oblique_project
from common import problem, xml_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
PROJ_M = (1, 2, 7, 8, 9, 32)
SLACK = 10.0     # true residual over the tolerance: what tests/native_bordered_cases.py allows (1e-7 at tol 1e-8)


def small_prec(lib, levels=1):
    A, tv = problem("Laplace", 8)
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, levels), testVector=tv, lib=lib)
    P.Initialize()
    P.Compute()
    return A, P


def _flat(cols, m, ld):
    """columns 0..m-1 of cols with leading dimension ld in exactly (m - 1) * ld + n doubles: a read past the last column is
    not absorbed by padding"""
    n = cols.shape[0]
    flat = np.zeros((m - 1) * ld + n)
    for j in range(m):
        flat[j * ld:j * ld + n] = cols[:, j]
    return flat


def _prm(tol=1e-8, maxit=300, blocks=250, **sol):
    d = {"Krylov Method": "GMRES", "Iterative Solver": {"Convergence Tolerance": tol, "Maximum Iterations": maxit, "Num Blocks": blocks}}
    d.update(sol)
    return d


# ---------------------------------------------------------------- 1. the primitive alone
def check_oblique_project(lib, dev, n):
    """y = x - P (G (Q' x)) against numpy in extended precision (np.longdouble, column by column), with worst-case bounds
    built from absolute values.  u = 2^-53, gamma_k = k u / (1 - k u), a_l = sum_i |Q_il x_i|.

    Coefficients.  c_l is a sum of n products in any order (fused or not): |c^_l - c_l| <= gamma_n a_l, and |c_l| <= a_l.
    d_j = sum_l G_jl c^_l is a sum of m products: |d^_j - d_j| <= gamma_m sum_l |G_jl| |c^_l| + sum_l |G_jl| |c^_l - c_l|
    <= (gamma_n + gamma_m + gamma_n gamma_m) sum_l |G_jl| a_l <= E_j := (n + m + 1) u (|G| a)_j, because the terms of second
    order, about (n u)^2 + n m u^2, stay below u for every n here ((2^20 u)^2 = 1.4e-20).  Without G, d = c and the same E
    with |G| = I holds.

    Rows.  s^_i = fl(sum_j P_ij d^_j) has |s^_i - sum_j P_ij d^_j| <= gamma_m t_i with t_i = sum_j |P_ij| |d^_j|, and the one
    subtraction adds u |x_i - s^_i| <= u (|x_i| + (1 + gamma_m) t_i): together (m + 2) u (|x_i| + t_i).  With
    |d^_j| <= |d_j| + E_j and the propagated coefficient error sum_j |P_ij| E_j:
        |y^_i - y_i| <= (m + 2) u (|x_i| + sum_j |P_ij| (|d_j| + E_j)) + sum_j |P_ij| E_j.
    (The longdouble reference itself is off by at most (n + m + 1) 2^-64 of the same sums, 2^-11 of the bound.)
    The kernel returns only y, so the coefficient bound is checked through the rows; on the CPU the numpy double evaluation
    (BLAS, another order) is checked against both bounds as well.  Two out-of-place calls and one in-place call: equal bits."""
    _, P = small_prec(lib)
    rng = np.random.default_rng(2000 + n % 9973)
    mmax = max(PROJ_M)
    Qc, Pc = rng.uniform(-1, 1, (n, mmax)), rng.uniform(-1, 1, (n, mmax))
    x, Gf = rng.uniform(-1, 1, n), rng.uniform(-1, 1, (mmax, mmax))
    L = np.longdouble
    xl = x.astype(L)
    c = np.array([(Qc[:, j].astype(L) * xl).sum() for j in range(mmax)], dtype=L)
    a = np.array([np.abs(Qc[:, j] * x).sum() for j in range(mmax)])
    xt = torch.from_numpy(x).to(dev)
    for m in PROJ_M:
        refs = []
        for G in (None, Gf[:m, :m]):
            absG = np.eye(m) if G is None else np.abs(G)
            d = c[:m] if G is None else G.astype(L) @ c[:m]
            E = (n + m + 1) * U * (absG @ a[:m])
            s, sa, se = np.zeros(n, L), np.zeros(n), np.zeros(n)
            for j in range(m):
                s += Pc[:, j].astype(L) * d[j]
                sa += np.abs(Pc[:, j]) * (float(abs(d[j])) + E[j])
                se += np.abs(Pc[:, j]) * E[j]
            y_ref, bound = xl - s, (m + 2) * U * (np.abs(x) + sa) + se
            if dev == "cpu":        # numpy's own double evaluation stays within the bounds
                c64 = Qc[:, :m].T @ x
                assert (np.abs(c64.astype(L) - c[:m]) <= (n + m + 1) * U * a[:m]).all(), (n, m)
                d64 = c64 if G is None else G @ c64
                assert (np.abs(d64.astype(L) - d) <= E).all(), (n, m)
                assert (np.abs((x - Pc[:, :m] @ d64).astype(L) - y_ref) <= bound).all(), (n, m)
            refs.append((G, y_ref, bound))
        for ld in (n, n + 5):
            Qt, Pt = torch.from_numpy(_flat(Qc, m, ld)).to(dev), torch.from_numpy(_flat(Pc, m, ld)).to(dev)
            for G, y_ref, bound in refs:
                outs = []
                for _ in range(2):
                    y = torch.full((n,), np.nan, dtype=torch.float64, device=dev)      # every row is written
                    oblique_project(P, n, m, Qt, ld, G, Pt, ld, xt, y)
                    outs.append(y.cpu().numpy())
                y = xt.clone()
                oblique_project(P, n, m, Qt, ld, G, Pt, ld, y, y)                      # in place
                outs.append(y.cpu().numpy())
                assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (n, m, ld)
                err = np.abs(outs[0].astype(L) - y_ref)
                assert (err <= bound).all(), (n, m, ld, G is None, float((err / bound).max()))
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                                  # x itself is never written


def check_oblique_project_refusals(lib, dev):
    _, P = small_prec(lib)
    n = 64
    V = torch.zeros(33 * n, dtype=torch.float64, device=dev)
    x, y = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    for args in ((n, 0, V, n, None, V, n, x, y), (n, 33, V, n, None, V, n, x, y), (n, 2, V, n - 1, None, V, n, x, y),
                 (n, 2, V, n, None, V, n - 1, x, y), (0, 2, V, n, None, V, n, x, y), (n, 2, None, n, None, V, n, x, y),
                 (n, 2, V, n, None, V, n, None, y)):
        with pytest.raises(hymls_amd.HymlsError) as e:
            oblique_project(P, *args)
        assert e.value.code == -2, args[:2]
    oblique_project(P, n, 2, V, n, None, V, n, x, y)       # and the valid call next to them passes


# ---------------------------------------------------------------- helpers of the projected systems
def _orthonormal(rng, N, m):
    return np.linalg.qr(rng.uniform(-1, 1, (N, m)))[0]


def _b_orthonormal(rng, N, m):
    """B = a positive diagonal on the first half of the rows and zero on the rest; V with V' B V = I, BV = B V"""
    B = np.zeros(N)
    B[:N // 2] = rng.uniform(0.5, 1.5, N // 2)
    V = rng.uniform(-1, 1, (N, m))
    R = np.linalg.cholesky(V.T @ (B[:, None] * V))          # V' B V = R R'
    V = np.linalg.solve(R, V.T).T                           # V R^-T
    return V, B[:, None] * V


def _project(V, BV, r):
    return r - BV @ (V.T @ r)


# ---------------------------------------------------------------- 2. the reference's unit tests as properties
def check_unit_properties(lib, dev, with_b):
    """testSuite/unit_tests/HYMLS_ProjectedOperator.cpp: Apply / ApplyWithB (V' y = 0 after the operator, to 1e-12) and
    ApplyInverse / ApplyInverseWithB (V' y = 0, with B: V' B y = 0, after the preconditioner, to 1e-10), on Laplace 8^3 with
    m = 10; X random in [-1, 1) as there.  Both forms of the preconditioner satisfy it and agree to 1e-10 |y|."""
    A, P = small_prec(lib)
    N, m = A.shape[0], 10
    rng = np.random.default_rng(51)
    V, BV = _b_orthonormal(rng, N, m) if with_b else (_orthonormal(rng, N, m),) * 2
    S = hymls_amd.NativeSolver(P, _prm())
    assert S.getNumProjection() == 0
    x = torch.from_numpy(rng.uniform(-1, 1, N)).to(dev)
    with pytest.raises(hymls_amd.HymlsError) as e:
        S.applyProjected(0, x)                               # no projection set
    assert e.value.code == -2
    S.setProjectionVectors(V, BV if with_b else None)
    assert S.getNumProjection() == m
    y = S.applyProjected(0, x).cpu().numpy()
    # the operator against its formula with numpy products
    t = x.cpu().numpy() - V @ (BV.T @ x.cpu().numpy())
    y_np = _project(V, BV, A @ t)
    print("operator: |V' y|_inf = %.3e, |y - numpy| / |y| = %.3e" % (np.abs(V.T @ y).max(), np.linalg.norm(y - y_np) / np.linalg.norm(y_np)))
    assert np.abs(V.T @ y).max() <= 1e-12
    assert np.linalg.norm(y - y_np) <= 1e-12 * np.linalg.norm(y_np)
    ys = {}
    for form in ("folded", "literal"):
        S.setParameterList(_prm(**{"MI Projection Form": form}))
        ys[form] = S.applyProjected(1, x).cpu().numpy()
        print("preconditioner, %s: |BV' y|_inf = %.3e" % (form, np.abs(BV.T @ ys[form]).max()))
        assert np.abs(BV.T @ ys[form]).max() <= 1e-10
    assert np.linalg.norm(ys["folded"] - ys["literal"]) <= 1e-10 * np.linalg.norm(ys["literal"])
    # and against the formula with the handle's own ApplyInverse
    Minv = lambda v: P.ApplyInverse(torch.from_numpy(np.ascontiguousarray(v)).to(dev)).cpu().numpy()
    Z = np.stack([Minv(BV[:, j]) for j in range(m)], axis=1)
    y0 = Minv(x.cpu().numpy())
    y_np = Minv(x.cpu().numpy() - BV @ np.linalg.solve(BV.T @ Z, BV.T @ y0))
    assert np.linalg.norm(ys["literal"] - y_np) <= 1e-10 * np.linalg.norm(y_np)
    # host pointers, and Y = X
    assert np.array_equal(S.applyProjected(1, x.cpu().numpy()), ys["literal"])
    xx = x.clone()
    assert S._lib.hymls_mi_solver_apply_projected(S._s, 1, xx.data_ptr(), xx.data_ptr(), 1) == 0
    assert np.array_equal(xx.cpu().numpy(), ys["literal"])


def check_set_projection_refusals(lib, dev):
    A, P = small_prec(lib)
    N = A.shape[0]
    rng = np.random.default_rng(52)
    S = hymls_amd.NativeSolver(P, _prm())
    lib = bind_projection(S._lib)
    V = _orthonormal(rng, N, 3)
    bad = V.copy()
    bad[:, 1] += 1e-6 * V[:, 0]                              # |V' V - I|_inf = 1e-6 > 1e-8
    with pytest.raises(hymls_amd.HymlsError) as e:
        S.setProjectionVectors(bad)
    assert e.value.code == -2 and "e-0" in str(e.value), str(e.value)    # the norm is in the message
    assert S.getNumProjection() == 0
    with pytest.raises(hymls_amd.HymlsError) as e:
        S.setProjectionVectors(V, 2.0 * V)                   # V' BV = 2 I
    assert e.value.code == -2
    with pytest.raises(hymls_amd.HymlsError) as e:
        S.setProjectionVectors(_orthonormal(rng, N, 33))
    assert e.value.code == -2
    with pytest.raises(hymls_amd.HymlsError) as e:
        S.setProjectionVectors(_orthonormal(rng, N - 1, 2))  # not the row count of the handle
    assert e.value.code == -2
    Vf = np.asfortranarray(V)
    assert lib.hymls_mi_solver_set_projection(S._s, N, 3, Vf.ctypes.data, N - 1, None, 0, 0) == -2
    assert lib.hymls_mi_solver_set_projection(S._s, N, 3, Vf.ctypes.data, N, Vf.ctypes.data, N - 1, 0) == -2
    assert lib.hymls_mi_solver_set_projection_form(S._s, 2) == -2 and lib.hymls_mi_solver_set_projection_form(S._s, -1) == -2
    with pytest.raises(ValueError):
        hymls_amd.NativeSolver(P, _prm(**{"MI Projection Form": "both"}))
    assert S.getNumProjection() == 0
    S.setProjectionVectors(torch.from_numpy(V).to(dev))     # a torch tensor, and the valid call passes
    assert S.getNumProjection() == 3


# ---------------------------------------------------------------- 3. exact preconditioner
def check_exact(lib, dev, with_b, lor):
    """"Number of Levels" 0: M = K, so A_p M_p^-1 is the identity on the range of I - BV V' and GMRES takes 1 iteration.
    A_p = (I - BV V') K (I - V BV') is singular with null space span(V), so its solutions differ by elements of span(V):
    pinv(A_p) b is the one with V' x = 0, the solver's the one with BV' x = 0 (its iterates are M_p^-1 of something).
    With BV = V they are the same vector; with B the solver's is (I - V BV') pinv(A_p) b, which is what x is compared with."""
    A, P = small_prec(lib, levels=0)
    N, m = A.shape[0], 3
    rng = np.random.default_rng(53)
    V, BV = _b_orthonormal(rng, N, m) if with_b else (_orthonormal(rng, N, m),) * 2
    b = _project(V, BV, rng.uniform(-1, 1, N))
    S = hymls_amd.NativeSolver(P, _prm(tol=1e-10, **{"Left or Right Preconditioning": lor}))
    S.setProjectionVectors(V, BV if with_b else None)
    x = S.ApplyInverse(torch.from_numpy(b).to(dev)).cpu().numpy()
    Ad = A.toarray()
    Pl, Pr = np.eye(N) - BV @ V.T, np.eye(N) - V @ BV.T
    x_np = Pr @ (np.linalg.pinv(Pl @ Ad @ Pr) @ b)
    print("exact, B %s, %s: %d iterations, |BV' x|_inf / |x| = %.3e, |x - pinv(A_p) b| / |x| = %.3e"
          % (with_b, lor, S.getNumIter(), np.abs(BV.T @ x).max() / np.linalg.norm(x), np.linalg.norm(x - x_np) / np.linalg.norm(x_np)))
    assert S.getNumIter() == 1
    assert np.abs(BV.T @ x).max() <= 1e-10 * np.linalg.norm(x)
    assert np.linalg.norm(x - x_np) <= 1e-8 * np.linalg.norm(x_np)


# ---------------------------------------------------------------- 4. inexact preconditioner
CASES = {"laplace": ("Laplace", 16, 4, 2, "Cartesian"), "stokes": ("Stokes-C", 16, 8, 1, "Skew Cartesian")}


@functools.lru_cache(maxsize=None)
def _system(name, m=3, seed=54):
    eq, n, sx, levels, part = CASES[name]
    A, tv = problem(eq, n)
    rng = np.random.default_rng(seed)
    V = _orthonormal(rng, A.shape[0], m)
    # b = A_p x_ex: a right-hand side in the range of the projected operator, as a correction equation has it.  (A random
    # projected vector is not: Stokes-C with its pinned pressure is close to singular, and on such a b the projected
    # solve stalls near 4e-2 for 300 iterations, in the native solver and in hymls_amd.Solver alike.)
    x_ex = rng.uniform(-1, 1, A.shape[0])
    b = _project(V, V, A @ (x_ex - V @ (V.T @ x_ex)))
    return A, tv, V, b


def _prec(lib, name):
    eq, n, sx, levels, part = CASES[name]
    A, tv, V, b = _system(name)
    P = hymls_amd.Preconditioner(A, xml_params(eq, n, sx, levels, -1, part), testVector=tv, lib=lib)
    P.Initialize()
    P.Compute()
    return A, V, b, P


def _proj_residual(A, V, BV, b, x):
    return np.linalg.norm(_project(V, BV, b - A @ x)) / np.linalg.norm(b)


def check_inexact(lib, dev, name):
    """Iterations to 1e-8 measured on the CPU simulator (native folded / native literal / hymls_amd.Solver):
        Laplace 16^3, sx 4, two levels:               20 / 20 / 20
        Stokes-C 16^3, Skew Cartesian, sx 8, 1 level: 95 / 95 / 95
    so the three are asserted to lie within one iteration of each other, on the simulator and on the GPU."""
    A, V, b, P = _prec(lib, name)
    bt = torch.from_numpy(b).to(dev)
    counts = {}
    for form in ("folded", "literal"):
        S = hymls_amd.NativeSolver(P, _prm(**{"MI Projection Form": form}))
        S.setProjectionVectors(V)
        x = S.ApplyInverse(bt).cpu().numpy()
        counts[form] = S.getNumIter()
        res = _proj_residual(A, V, V, b, x)
        print("%s %s: %d iterations, projected residual %.3e, |V' x|_inf / |x| = %.3e"
              % (name, form, counts[form], res, np.abs(V.T @ x).max() / np.linalg.norm(x)))
        assert res <= SLACK * 1e-8 and S.achievedTol() <= 1e-8
        x2 = S.ApplyInverse(bt).cpu().numpy()               # a second identical solve: the same bits
        assert np.array_equal(x, x2) and S.getNumIter() == counts[form]
    Sp = hymls_amd.Solver(P, P, _prm())
    Sp.setProjectionVectors(V)
    xp = Sp.ApplyInverse(bt).cpu().numpy()
    counts["python"] = Sp.getNumIter()
    assert _proj_residual(A, V, V, b, xp) <= SLACK * 1e-8
    print("%s iterations: %s" % (name, counts))
    assert max(counts.values()) - min(counts.values()) <= 1, counts


# ---------------------------------------------------------------- 5. variants on Laplace 16^3
def check_variants(lib, dev):
    A, V, b, P = _prec(lib, "laplace")
    bt = torch.from_numpy(b).to(dev)

    def solve(prm, rhs=bt):
        S = hymls_amd.NativeSolver(P, prm)
        S.setProjectionVectors(V)
        return S, S.ApplyInverse(rhs)

    S0, x0 = solve(_prm())
    base = S0.getNumIter()
    for label, prm in (("left", _prm(**{"Left or Right Preconditioning": "Left"})), ("restarts", _prm(blocks=10)),
                       ("random", _prm(**{"Initial Vector": "Random", "Random Seed": 7})),
                       ("single", _prm(**{"MI Basis Storage": "single"}))):
        S, x = solve(prm)
        xn = x.cpu().numpy()
        res = _proj_residual(A, V, V, b, xn)
        print("Laplace 16^3 %s: %d iterations (plain %d), %d restarts, projected residual %.3e" % (label, S.getNumIter(), base, S.getNumRestarts(), res))
        assert res <= SLACK * 1e-8 and S.getNumIter() > 0
        assert np.abs(V.T @ xn).max() <= 1e-10 * np.linalg.norm(xn)
        assert (S.getNumRestarts() > 0) == (label in ("restarts", "single"))
    # "Previous": the second solve starts from the projected solution of the first and has nothing left to do
    S, x = solve(_prm(**{"Initial Vector": "Previous"}))
    first = S.getNumIter()
    x2 = S.ApplyInverse(2.0 * bt)
    print("Previous start: %d iterations, then %d for twice the right-hand side" % (first, S.getNumIter()))
    assert first == base and 0 < S.getNumIter() <= first
    assert _proj_residual(A, V, V, 2.0 * b, x2.cpu().numpy()) <= SLACK * 1e-8
    # CG (BV = V, K and M symmetric: the projected pair is symmetric) against the GMRES solution
    Sc, xc = solve({"Krylov Method": "CG", "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 300}})
    print("CG: %d iterations" % Sc.getNumIter())
    assert torch.linalg.norm(xc - x0) <= 1e-6 * torch.linalg.norm(x0)
    # two columns with a lock-step width of 2: the width is ignored, bitwise two single solves
    B2 = torch.stack([bt, 0.5 * bt + torch.from_numpy(_project(V, V, np.cos(np.arange(b.size)))).to(dev)])
    S2, X2 = solve(_prm(**{"MI Lockstep Columns": 2}), B2)
    assert S2.getLockstep() == 2 and len(S2.getColumnResults()) == 2
    for c in range(2):
        Sc1, xc1 = solve(_prm(), B2[c].contiguous())
        assert torch.equal(X2[c], xc1) and S2.getColumnResults()[c]["iterations"] == Sc1.getNumIter()
    assert torch.equal(X2[0], x0)


# ---------------------------------------------------------------- 6. life cycle
def check_life_cycle(lib, dev):
    A, P = small_prec(lib, levels=0)
    N, m = A.shape[0], 3
    rng = np.random.default_rng(55)
    V, BV = _b_orthonormal(rng, N, m)
    b = _project(V, BV, rng.uniform(-1, 1, N))
    bt = torch.from_numpy(b).to(dev)
    raw = torch.from_numpy(rng.uniform(-1, 1, N)).to(dev)
    Sn = hymls_amd.NativeSolver(P, _prm(tol=1e-10))
    x_never = Sn.ApplyInverse(raw)
    for form in ("folded", "literal"):
        S = hymls_amd.NativeSolver(P, _prm(tol=1e-10, **{"MI Projection Form": form}))
        S.setProjectionVectors(V, BV)
        x = S.ApplyInverse(bt).cpu().numpy()
        assert S.getNumIter() == 1
        # the bordered entry refuses a solver with projection vectors
        xo = torch.empty_like(bt)
        assert bind_bordered(S._lib).hymls_mi_solver_solve_bordered(S._s, bt.data_ptr(), None, xo.data_ptr(), None, 1) == -99
        # a changed matrix: Z and H are formed again by the next solve
        P.SetMatrix(2.0 * A)
        P.Compute()
        x2 = S.ApplyInverse(bt).cpu().numpy()
        print("%s after Compute with 2 K: %d iterations, |BV' x|_inf / |x| = %.3e, |2 x2 - x| / |x| = %.3e"
              % (form, S.getNumIter(), np.abs(BV.T @ x2).max() / np.linalg.norm(x2), np.linalg.norm(2 * x2 - x) / np.linalg.norm(x)))
        assert S.getNumIter() == 1
        assert np.abs(BV.T @ x2).max() <= 1e-10 * np.linalg.norm(x2)
        assert _proj_residual(2.0 * A, V, BV, b, x2) <= 1e-9
        assert np.linalg.norm(2 * x2 - x) <= 1e-8 * np.linalg.norm(x)
        P.SetMatrix(A)
        P.Compute()
        # without the projection: the bits of a solver that never had one
        S.setProjectionVectors(None)
        assert S.getNumProjection() == 0
        assert torch.equal(S.ApplyInverse(raw), x_never) and S.getNumIter() == Sn.getNumIter()


def missing_symbols_return_m99(lib):
    """a library whose krylov.cpp was built without HYMLS_MI_PROJECTED_SOLVER has every new symbol, and each returns -99
    (hymls_mi_solver_num_projection: 0)"""
    bind_projection(lib)
    A, P = small_prec(lib)
    N = A.shape[0]
    S = hymls_amd.NativeSolver(P, _prm())
    V = np.asfortranarray(_orthonormal(np.random.default_rng(56), N, 2))
    x = torch.ones(N, dtype=torch.float64)
    y = torch.empty_like(x)
    assert lib.hymls_mi_solver_set_projection(S._s, N, 2, V.ctypes.data, N, None, 0, 0) == -99
    assert lib.hymls_mi_solver_set_projection(S._s, N, 0, None, 0, None, 0, 0) == -99
    assert lib.hymls_mi_solver_num_projection(S._s) == 0
    assert lib.hymls_mi_solver_set_projection_form(S._s, 1) == -99
    assert lib.hymls_mi_solver_apply_projected(S._s, 0, x.data_ptr(), y.data_ptr(), 1) == -99
    Vt = torch.from_numpy(V.T.copy())
    assert lib.hymls_mi_oblique_project(P._h, N, 2, Vt.data_ptr(), N, None, Vt.data_ptr(), N, x.data_ptr(), y.data_ptr()) == -99
    assert S._lib.hymls_mi_solver_solve(S._s, x.data_ptr(), N, y.data_ptr(), N, 1, 1) == 0      # the plain solve is untouched
