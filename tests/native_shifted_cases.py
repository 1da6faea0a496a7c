"""Checks of the mass matrix and the shifted operator a K + b B of the native Krylov solver (hymls_mi_solver_set_mass_matrix,
_apply_mass, _set_shift, _shift, hymls_mi_shifted_product; hymls_amd.NativeSolver.SetMassMatrix / ApplyMass / setShift),
shared by tests/test_native_shifted.py (the TEST-ONLY simulator of tests/krylov_shift_sim, CPU tensors) and
tests/test_native_shifted_gpu.py (the product library on the MI355X).  Every check takes (lib, dev).

    operator         y = a K x + b B x,   B the mass matrix, or the identity when none is set
    preconditioner   ApplyInverse of the handle: the preconditioner of K alone
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import hymls_amd
from hymls_amd.native_solver import bind_shifted, shifted_product
from oracle import krylov as okrylov
from common import problem, xml_params
from native_projected_cases import CASES, SLACK, _prm, small_prec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
EPS = 2.0 ** -52
SHIFTS = ((1.0, 0.0), (0.0, 1.0), (1.0, -0.3), (0.5, 2.0))
# a mean row length for which dev::spmv_lanes gives L lanes (avg < 2.5: 1, < 5: 2, < 20: 4, else 8)
MEAN_FOR_LANES = {1: 1.5, 2: 3.5, 4: 8.0, 8: 24.0}
NVEC = 5


def same_bits(x, y):
    """torch.equal on the bit patterns (NaN sentinels compare equal to themselves)"""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


def spmv_lanes(n, hint):
    avg = hint / n if hint >= 0 else 8.0
    return 1 if avg < 2.5 else (2 if avg < 5.0 else (4 if avg < 20.0 else 8))


# ---------------------------------------------------------------- 1. the building block on edge shapes
def _random_csr(rng, n, lengths):
    """CSR with the given row lengths, columns uniform in [0, n) (a row may name a column twice: duplicates add up), values
    uniform in [-1, 1)"""
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=rp[1:])
    nnz = int(rp[-1])
    return sp.csr_matrix((rng.uniform(-1, 1, nnz), rng.integers(0, n, nnz).astype(np.int32), rp.astype(np.int32)), shape=(n, n))


def _row_sums(M, x):
    """(sum_j M_ij x_j in extended precision, sum_j |M_ij x_j|, the row lengths) of a CSR matrix with unsorted, repeated columns"""
    n = M.shape[0]
    lens = np.diff(M.indptr)
    s, sa = np.zeros(n, LD), np.zeros(n)
    rows = np.flatnonzero(lens)
    if rows.size:
        xs = x[M.indices]
        starts = M.indptr[rows]
        s[rows] = np.add.reduceat(M.data.astype(LD) * xs.astype(LD), starts)
        sa[rows] = np.add.reduceat(np.abs(M.data * xs), starts)
    return s, sa, lens


@functools.lru_cache(maxsize=2)
def _product_problem(n):
    """A: row lengths cycling through 0 .. 17 (0 .. 2 L + 1 for the widest L = 8, so every lane of every L meets rows with
    none, one and several entries of its own; at 2^20 + 3 the middle rows cycle through 0 .. 3 only) plus one row of
    min(n, 1000) entries; B in three kinds: None (the identity), a
    diagonal with zero values and missing rows, and random CSR with longer rows than A that are never empty.  X: NVEC columns.
    The references (row sums in np.longdouble, sums of absolute values, row lengths) are computed once per n."""
    rng = np.random.default_rng(3000 + n % 9973)
    la = np.arange(n) % 18
    if n > 8192:      # keeps the host reference of the largest case near a second: the long cycle in the first and last 4096 rows
        la[4096:n - 4096] %= 4
    la[n // 2] = min(n, 1000)
    A = _random_csr(rng, n, la)
    d = rng.uniform(-1, 1, n)
    d[::3] = 0.0
    keep = np.arange(n) % 5 != 4
    Bd = sp.csr_matrix((d[keep], np.flatnonzero(keep).astype(np.int32), np.concatenate([[0], np.cumsum(keep)]).astype(np.int32)), shape=(n, n))
    Br = _random_csr(rng, n, la + 1 + np.arange(n) % 3)
    X = rng.uniform(-1, 1, (n, NVEC))
    refs = {}
    for kind, M in (("A", A), ("diag", Bd), ("random", Br)):
        refs[kind] = [_row_sums(M, X[:, v]) for v in range(NVEC)]
    refs["identity"] = [(X[:, v].astype(LD), np.abs(X[:, v]), np.ones(n, dtype=np.int64)) for v in range(NVEC)]
    return A, {"identity": None, "diag": Bd, "random": Br}, X, refs


def _dev_csr(M, dev):
    if M is None:
        return None
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev) for a, t in ((M.indptr, np.int32), (M.indices, np.int32), (M.data, np.float64)))


def _combos(n):
    """(lanes or None for hint -1, kind of B, (a, b)).  Up to n = 4099 the full cross product; at 2^20 + 3, where the host
    reference of one combination takes half a second, every L, every B and every (a, b) still occur, but not every triple"""
    if n <= 4099:
        return [(L, k, ab) for L in (None, 1, 2, 4, 8) for k in ("identity", "diag", "random") for ab in SHIFTS]
    return [(None, "identity", SHIFTS[2]), (None, "diag", SHIFTS[3]), (None, "random", SHIFTS[1]), (4, "random", SHIFTS[0]),
            (1, "random", SHIFTS[2]), (2, "diag", SHIFTS[2]), (8, "random", SHIFTS[3])]


def check_shifted_product(lib, dev, n):
    """Y = a A X + b B X against numpy in extended precision, per row
        |y - y_ref| <= (len_A + len_B + 4) 2^-52 (|a| sum_j |A_ij x_j| + |b| sum_j |B_ij x_j|),
    the bound of a sum of len_A + len_B products in any order, fused or not, with the two scalings and the final add
    (len_B = 1 and the sum |x_i| for B = identity).  The lanes per row follow from the hint alone, so one A serves every L:
    the hint is n times a mean row length that selects L, once the true nnz, once -1.  Bitwise: every column of an nvec > 1
    call equals its nvec = 1 call, a repeated call gives the same bits, and the rows of Y beyond n keep their NaN."""
    _, P = small_prec(lib)
    A, Bs, X, refs = _product_problem(n)
    ldx, ldy = n + 2, n + 3
    Ad = _dev_csr(A, dev)
    Bd = {k: _dev_csr(M, dev) for k, M in Bs.items()}
    # operands at the end of exactly sized allocations: a read or write past the last column is not absorbed by padding
    xf = np.zeros((NVEC - 1) * ldx + n)
    for v in range(NVEC):
        xf[v * ldx:v * ldx + n] = X[:, v]
    xt = torch.from_numpy(xf).to(dev)
    assert spmv_lanes(n, A.nnz) in (1, 2, 4, 8)
    seen = set()
    for L, kind, (a, b) in _combos(n):
        hint = -1 if L is None else (A.nnz if spmv_lanes(n, A.nnz) == L else int(n * MEAN_FOR_LANES[L]))
        assert L is None or spmv_lanes(n, hint) == L
        seen.add(spmv_lanes(n, hint))

        def call(nv, v0=0):
            y = torch.full(((nv - 1) * ldy + n,), np.nan, dtype=torch.float64, device=dev)
            shifted_product(P, n, a, Ad, b, Bd[kind], xt[v0 * ldx:], ldx, y, ldy, nv, hint)
            return y
        full = call(NVEC)
        assert same_bits(full, call(NVEC))                                       # repeated: the same bits
        for v in range(NVEC):                                                    # every column: the bits of its nvec = 1 call
            assert same_bits(full[v * ldy:v * ldy + n], call(1, v)), (n, L, kind, a, b, v)
        for nv in (2, 3, 4):
            assert same_bits(call(nv), full[:(nv - 1) * ldy + n]), (n, L, kind, a, b, nv)
        got = full.cpu().numpy()
        for v in range(NVEC):
            if v < NVEC - 1:
                assert np.isnan(got[v * ldy + n:(v + 1) * ldy]).all()            # rows beyond n are untouched
            sA, absA, lenA = refs["A"][v]
            sB, absB, lenB = refs[kind][v]
            y_ref = LD(a) * sA + LD(b) * sB
            bound = (lenA + lenB + 4) * EPS * (abs(a) * absA + abs(b) * absB)
            err = np.abs(got[v * ldy:v * ldy + n].astype(LD) - y_ref)
            assert (err <= bound).all(), (n, L, kind, a, b, v, float((err[bound > 0] / bound[bound > 0]).max()))
    assert seen == {1, 2, 4, 8}
    assert torch.equal(xt.cpu(), torch.from_numpy(xf))                           # X itself is never written


# ---------------------------------------------------------------- 2. refusals
def check_refusals(lib, dev):
    """every -2 of hymls_mi_shifted_product and hymls_mi_solver_set_mass_matrix (each is decided on the host: Y keeps its
    NaN, and a bad CSR never reaches a kernel), of set_shift and of apply_mass.  nnz >= 2^31 cannot be written in 32-bit
    row pointers: it shows as a decreasing entry, which is covered"""
    A, P = small_prec(lib)
    N = A.shape[0]
    lib = bind_shifted(P._lib)
    Ad = _dev_csr(A.tocsr(), dev)
    buf = torch.arange(4 * N, dtype=torch.float64, device=dev)
    x, y = buf[:N], torch.full((2 * N,), np.nan, dtype=torch.float64, device=dev)
    ok = dict(n=N, a=1.0, A=Ad, b=1.0, B=None, X=x, ldx=N, Y=y, ldy=N, nvec=1)
    bad = (dict(n=0), dict(n=2 ** 31), dict(nvec=-1), dict(ldx=N - 1), dict(ldy=N - 1), dict(A=None), dict(A=(Ad[0], None, Ad[2])),
           dict(X=buf, Y=buf[N - 1:]), dict(X=buf[N - 1:], Y=buf), dict(X=buf, Y=buf[2 * N - 1:], nvec=2), dict(X=x, Y=x), dict(X=None))
    for change in bad:
        with pytest.raises(hymls_amd.HymlsError) as e:
            shifted_product(P, **dict(ok, **change))
        assert e.value.code == -2, change.keys()
    assert torch.isnan(y).all()
    shifted_product(P, **dict(ok, nvec=0, X=None, Y=None))                       # nvec = 0: a no-op
    assert torch.isnan(y).all()
    shifted_product(P, **dict(ok, a=0.0, A=None))                                # a = 0: A may be null
    assert torch.equal(y[:N], x)
    shifted_product(P, **ok)                                                     # and the valid call next to them passes

    S = hymls_amd.NativeSolver(P, _prm())
    rp, ci, va = (np.ascontiguousarray(a) for a in (A.tocsr().indptr.astype(np.int32), A.tocsr().indices.astype(np.int32), A.tocsr().data))

    def set_mass(n, rp_, ci_, va_):
        if dev == "cpu":
            return lib.hymls_mi_solver_set_mass_matrix(S._s, n, rp_.ctypes.data, ci_.ctypes.data, va_.ctypes.data, 0)
        t = [torch.from_numpy(a).to(dev) for a in (rp_, ci_, va_)]                # device input: checked after one copy back
        return lib.hymls_mi_solver_set_mass_matrix(S._s, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 1)
    xs = torch.arange(N, dtype=torch.float64, device=dev)
    for what in ("n", "first", "decrease", "low", "high", "wrap"):
        r, c = rp.copy(), ci.copy()
        n = N
        if what == "n":
            n, r = N - 1, rp[:N].copy()
        elif what == "first":
            r[0] = 1
        elif what == "decrease":
            r[5] = r[4] - 1
        elif what == "low":
            c[7] = -1
        elif what == "high":
            c[-1] = N
        else:
            r[N] = -(2 ** 31)                                                    # what 2^31 entries look like in int32
        assert set_mass(n, r, c, va) == -2, what
        assert "set_mass_matrix" in lib.hymls_mi_solver_last_error(S._s).decode()
        assert torch.equal(S.ApplyMass(xs), xs)                                  # left without a mass matrix
    assert lib.hymls_mi_solver_set_mass_matrix(S._s, N, rp.ctypes.data, None, None, 0) == -2
    assert set_mass(N, rp, ci, va) == 0
    for a, b in ((0.0, 0.0), (np.nan, 1.0), (1.0, np.inf), (-np.inf, 0.0)):
        assert lib.hymls_mi_solver_set_shift(S._s, a, b) == -2
    assert S.getShift() == (1.0, 0.0)
    y2 = torch.empty(2 * N, dtype=torch.float64, device=dev)
    assert lib.hymls_mi_solver_apply_mass(S._s, buf.data_ptr(), N, y2.data_ptr(), N, -1, 1) == -2
    assert lib.hymls_mi_solver_apply_mass(S._s, buf.data_ptr(), N - 1, y2.data_ptr(), N, 2, 1) == -2
    assert lib.hymls_mi_solver_apply_mass(S._s, buf.data_ptr(), N, y2.data_ptr(), N - 1, 2, 1) == -2
    assert lib.hymls_mi_solver_apply_mass(S._s, buf.data_ptr(), N, buf.data_ptr(), N, 1, 1) == -2
    assert lib.hymls_mi_solver_apply_mass(S._s, None, N, y2.data_ptr(), N, 1, 1) == -2
    assert lib.hymls_mi_solver_apply_mass(S._s, None, N, None, N, 0, 1) == 0


def missing_symbols_return_m99(lib):
    """a library whose krylov.cpp was built without HYMLS_MI_SHIFTED_SOLVER has every new symbol, and each returns -99"""
    bind_shifted(lib)
    A, P = small_prec(lib)
    N = A.shape[0]
    S = hymls_amd.NativeSolver(P, _prm())
    Ac = A.tocsr()
    rp, ci, va = Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), np.ascontiguousarray(Ac.data)
    x = torch.ones(N, dtype=torch.float64)
    y = torch.empty_like(x)
    a, b = ctypes.c_double(), ctypes.c_double()
    assert lib.hymls_mi_solver_set_mass_matrix(S._s, N, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0) == -99
    assert lib.hymls_mi_solver_set_mass_matrix(S._s, N, None, None, None, 0) == -99
    assert lib.hymls_mi_solver_apply_mass(S._s, x.data_ptr(), N, y.data_ptr(), N, 1, 1) == -99
    assert lib.hymls_mi_solver_set_shift(S._s, 1.0, -0.5) == -99
    assert lib.hymls_mi_solver_shift(S._s, ctypes.byref(a), ctypes.byref(b)) == -99
    assert lib.hymls_mi_shifted_product(P._h, N, 1.0, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, -1, 0.0, None, None, None,
                                        x.data_ptr(), N, y.data_ptr(), N, 1) == -99
    assert S._lib.hymls_mi_solver_solve(S._s, x.data_ptr(), N, y.data_ptr(), N, 1, 1) == 0      # the plain solve is untouched


# ---------------------------------------------------------------- 3. solver properties on Laplace 8^3
def _diag_mass(N, seed=61):
    d = np.random.default_rng(seed).uniform(0.5, 1.5, N)
    d[::4] = 0.0
    return sp.diags(d).tocsr()


def check_solver_properties(lib, dev):
    A, P = small_prec(lib)
    N = A.shape[0]
    rng = np.random.default_rng(62)
    bt = torch.from_numpy(rng.uniform(-1, 1, N)).to(dev)
    Bm = _random_csr(rng, N, 1 + np.arange(N) % 6)
    S0 = hymls_amd.NativeSolver(P, _prm())
    x0 = S0.ApplyInverse(bt)
    S = hymls_amd.NativeSolver(P, _prm())
    assert S.getShift() == (1.0, 0.0)
    # setShift(1, 0), without and with a mass matrix: the bits and the count of a solver that never had either
    S.setShift(1.0, 0.0)
    assert torch.equal(S.ApplyInverse(bt), x0) and S.getNumIter() == S0.getNumIter()
    S.SetMassMatrix(Bm)
    assert torch.equal(S.ApplyInverse(bt), x0) and S.getNumIter() == S0.getNumIter()
    # ApplyMass = B X within the bound of check 1 (a = 0, b = 1), device and host, one and several columns; X without B
    X = rng.uniform(-1, 1, (N, 3))
    got_dev = S.ApplyMass(torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)).cpu().numpy().T
    got_host = S.ApplyMass(X)
    assert np.array_equal(got_dev, got_host)
    assert np.array_equal(S.ApplyMass(torch.from_numpy(X[:, 1].copy()).to(dev)).cpu().numpy(), got_dev[:, 1])
    for v in range(3):
        s, sa, lens = _row_sums(Bm, X[:, v])
        assert (np.abs(got_dev[:, v].astype(LD) - s) <= (lens + 4) * EPS * sa).all()
    assert np.array_equal(S0.ApplyMass(X), X)
    # the shift round-trips, and set_params keeps the shift and B
    S.setShift(0.5, -0.25)
    assert S.getShift() == (0.5, -0.25)
    S.setParameterList(_prm(tol=1e-9, **{"Left or Right Preconditioning": "Left"}))
    assert S.getShift() == (0.5, -0.25) and np.array_equal(S.ApplyMass(X), got_host)
    # removing B and resetting the shift restores the plain bits
    S.setParameterList(_prm())
    S.SetMassMatrix(None)
    assert np.array_equal(S.ApplyMass(X), X)
    S.setShift(1.0, 0.0)
    assert torch.equal(S.ApplyInverse(bt), x0) and S.getNumIter() == S0.getNumIter()


def check_exact_scaled(lib, dev):
    """"Number of Levels" 0: M = K, so with (a, b) = (2, 0) the preconditioned operator is 2 I: one GMRES iteration, and
    x = K^-1 b / 2"""
    A, P = small_prec(lib, levels=0)
    N = A.shape[0]
    b = np.random.default_rng(63).uniform(-1, 1, N)
    S = hymls_amd.NativeSolver(P, _prm(tol=1e-10))
    S.setShift(2.0, 0.0)
    x = S.ApplyInverse(torch.from_numpy(b).to(dev)).cpu().numpy()
    x_ref = spla.spsolve(A.tocsc(), b) / 2.0
    print("exact, (2, 0): %d iterations, |x - K^-1 b / 2| / |x| = %.3e" % (S.getNumIter(), np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)))
    assert S.getNumIter() == 1
    assert np.linalg.norm(x - x_ref) <= 1e-10 * np.linalg.norm(x_ref)


# ---------------------------------------------------------------- 4. shifted solves
@functools.lru_cache(maxsize=None)
def _shifted_system(name):
    eq, n, sx, levels, part = CASES[name]
    A, tv = problem(eq, n)
    A = A.tocsr()
    N = A.shape[0]
    vel = np.ones(N, dtype=bool) if eq == "Laplace" else np.arange(N) % 4 != 3
    sigma = 0.1 * A.diagonal()[vel].mean()
    Bm = None if eq == "Laplace" else sp.diags(vel.astype(np.float64)).tocsr()      # diag(1, 1, 1, 0) per node
    return A, tv, Bm, sigma


def _handle(lib, name):
    eq, n, sx, levels, part = CASES[name]
    A, tv, Bm, sigma = _shifted_system(name)
    P = hymls_amd.Preconditioner(A, xml_params(eq, n, sx, levels, -1, part), testVector=tv, lib=lib)
    P.Initialize()
    P.Compute()
    return A, Bm, sigma, P


def check_shifted_solve(lib, dev, name):
    """(a K + b B) x = rhs with the preconditioner of K, start vector "Zero", sigma = 0.1 times the mean diagonal entry of the
    velocity rows of K (no case needs more than 200 reference iterations, so 0.1 it is).  The generated matrices are the
    reference's, -1 times the discrete operator, so those diagonals and sigma are negative (-0.6 and -150): the shift makes K
    more definite, as a time stepper's does.  The right-hand side is (a K + b B) x_ex for a random x_ex: on a random
    right-hand side Stokes-C with its pinned pressure stalls near 0.2 for 250 iterations, with and without a shift, in the
    oracle as well (tests/native_projected_cases.py meets the same).  The reference iteration is oracle.krylov.gmres / pcg on
    the callable x -> a K x + b B x with the same handle's ApplyInverse.  Iterations to 1e-8 measured on the CPU simulator
    (native / oracle):
        Laplace 16^3, sx 4, two levels, B = I:   (1, sigma) GMRES 20 / 20, CG 20 / 20;  (0.5, sigma) GMRES 22 / 22, CG 22 / 22
        Stokes-C 16^3, Skew Cartesian, sx 8, one level, B = diag(1, 1, 1, 0):   (1, sigma) GMRES 80 / 80
    so the solver's count is asserted to lie within one iteration of the reference's, on the simulator and on the GPU."""
    A, Bm, sigma, P = _handle(lib, name)
    N = A.shape[0]
    x_ex = np.random.default_rng(64).uniform(-1, 1, N)
    Minv = lambda v: P.ApplyInverse(torch.from_numpy(np.ascontiguousarray(v)).to(dev)).cpu().numpy()
    runs = [((1.0, sigma), "GMRES"), ((1.0, sigma), "CG"), ((0.5, sigma), "GMRES"), ((0.5, sigma), "CG")] if name == "laplace" else [((1.0, sigma), "GMRES")]
    for (a, b), method in runs:
        op = (lambda v: a * (A @ v) + b * v) if Bm is None else (lambda v: a * (A @ v) + b * (Bm @ v))
        rhs = op(x_ex)
        bt = torch.from_numpy(rhs).to(dev)
        if method == "GMRES":
            _, its_ref, res_ref = okrylov.gmres(op, rhs, prec=Minv, tol=1e-8, maxit=250)
        else:
            _, its_ref, res_ref = okrylov.pcg(op, rhs, prec=Minv, tol=1e-8, maxit=250)
        assert its_ref <= 200 and res_ref <= SLACK * 1e-8, (its_ref, res_ref)
        S = hymls_amd.NativeSolver(P, _prm(**{"Krylov Method": method}))
        S.SetMassMatrix(Bm)
        S.setShift(a, b)
        x = S.ApplyInverse(bt)
        its = S.getNumIter()
        res = np.linalg.norm(rhs - op(x.cpu().numpy())) / np.linalg.norm(rhs)
        print("%s (%g, %g) %s: %d iterations (oracle %d), true residual %.3e" % (name, a, b, method, its, its_ref, res))
        assert res <= SLACK * 1e-8
        assert abs(its - its_ref) <= 1, (its, its_ref)
        assert torch.equal(S.ApplyInverse(bt), x) and S.getNumIter() == its         # a second identical solve: the same bits


# ---------------------------------------------------------------- 5. the correction equation of Jacobi-Davidson
def check_correction_equation(lib, dev):
    """Laplace 16^3: V the eigenvectors of the three lowest modes, BV = V, theta = 1.01 lambda_0, setShift(1, -theta) and
    setProjectionVectors(V), rhs = (I - V V') r.  The generated K is -1 times the discrete Laplacian, as in the reference, so
    the lowest modes are its eigenvalues of smallest magnitude, 0 > lambda_0 > theta > lambda_3: K - theta I is indefinite,
    but definite on the complement of V, with the sign of K and of its preconditioner, which is what CG needs.  The reference
    iteration is oracle.krylov on the projected callables: the operator (I - V V') (K - theta I) (I - V V') and the literal
    projected preconditioner.  Iterations to 1e-8 on the CPU simulator: GMRES folded 25, literal 25, oracle 25;  CG 25, oracle 25."""
    A, Bm, sigma, P = _handle(lib, "laplace")
    N = A.shape[0]
    # (a fixed start vector: the second and third mode belong to a threefold eigenvalue, of which ARPACK returns two vectors)
    lam, V = spla.eigsh(A.tocsc(), k=3, sigma=0.0, which="LM", v0=np.cos(np.arange(N)))
    order = np.argsort(np.abs(lam))
    lam, V = lam[order], np.linalg.qr(V[:, order])[0]
    theta = 1.01 * lam[0]
    assert lam[0] < 0.0 and theta > lam[1] >= lam[2] - 1e-9
    proj = lambda v: v - V @ (V.T @ v)
    rhs = proj(np.random.default_rng(65).uniform(-1, 1, N))
    bt = torch.from_numpy(rhs).to(dev)
    Minv = lambda v: P.ApplyInverse(torch.from_numpy(np.ascontiguousarray(v)).to(dev)).cpu().numpy()
    Z = np.stack([Minv(V[:, j]) for j in range(3)], axis=1)
    H = V.T @ Z
    op = lambda v: proj(A @ proj(v) - theta * proj(v))
    prec = lambda v: Minv(v - V @ np.linalg.solve(H, V.T @ Minv(v)))
    _, its_g, _ = okrylov.gmres(op, rhs, prec=prec, tol=1e-8, maxit=250)
    _, its_c, _ = okrylov.pcg(op, rhs, prec=prec, tol=1e-8, maxit=250)
    for method, form, its_ref in (("GMRES", "folded", its_g), ("GMRES", "literal", its_g), ("CG", "folded", its_c)):
        S = hymls_amd.NativeSolver(P, _prm(**{"Krylov Method": method, "MI Projection Form": form}))
        S.setShift(1.0, -theta)
        S.setProjectionVectors(V)
        x = S.ApplyInverse(bt).cpu().numpy()
        res = np.linalg.norm(proj(rhs - (A @ x - theta * x))) / np.linalg.norm(rhs)
        vx = np.abs(V.T @ x).max() / np.linalg.norm(x)
        print("correction equation, %s %s: %d iterations (oracle %d), projected residual %.3e, |V' x|_inf / |x| = %.3e"
              % (method, form, S.getNumIter(), its_ref, res, vx))
        assert res <= SLACK * 1e-8
        assert vx <= 1e-10
        assert abs(S.getNumIter() - its_ref) <= 1, (S.getNumIter(), its_ref)
        # apply_projected(which = 0) is the shifted projected operator
        y = S.applyProjected(0, bt).cpu().numpy()
        assert np.linalg.norm(y - op(rhs)) <= 1e-12 * np.linalg.norm(op(rhs))


# ---------------------------------------------------------------- 6. compositions
def check_lockstep(lib, dev):
    """widths 2 and 4 with a shift and a mass matrix on four right-hand sides: X and the per-column results are bitwise those
    of width 1, with "Zero" and "Random" start vectors, both basis storages and CG"""
    A, P = small_prec(lib)
    N = A.shape[0]
    Bm = _diag_mass(N)
    sigma = 0.1 * A.diagonal().mean()
    Bt = torch.from_numpy(np.random.default_rng(66).uniform(-1, 1, (4, N))).to(dev)
    for method, storage in (("GMRES", "double"), ("GMRES", "single"), ("CG", "double")):
        for start in ("Zero", "Random"):
            outs = {}
            for width in (1, 2, 4):
                S = hymls_amd.NativeSolver(P, _prm(**{"Krylov Method": method, "MI Basis Storage": storage, "Initial Vector": start,
                                                      "Random Seed": 9, "MI Lockstep Columns": width}))
                S.SetMassMatrix(Bm)
                S.setShift(1.0, sigma)
                outs[width] = (S.ApplyInverse(Bt), S.getColumnResults())
            X1 = outs[1][0].cpu().numpy()
            for c in range(4 if start == "Zero" else 0):          # ("Random": convergence is relative to the first residual)
                r = Bt[c].cpu().numpy() - (A @ X1[c] + sigma * (Bm @ X1[c]))
                assert np.linalg.norm(r) <= SLACK * 1e-8 * np.linalg.norm(Bt[c].cpu().numpy())
            for width in (2, 4):
                assert torch.equal(outs[width][0], outs[1][0]), (method, storage, start, width)
                assert outs[width][1] == outs[1][1], (method, storage, start, width)


def check_bordered(lib, dev):
    """Laplace 8^3 with a border of two columns and the shift (1, sigma), B = I: [x; s] against a dense numpy solve of
    [K + sigma I, V; W', C], to 1e-6 relative at tolerance 1e-10"""
    A, tv = problem("Laplace", 8)
    N, m = A.shape[0], 2
    rng = np.random.default_rng(67)
    V, W, Cm = rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (m, m))
    sigma = 0.1 * A.diagonal().mean()
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 1), testVector=tv, lib=lib)
    P.Initialize()
    S = hymls_amd.NativeBorderedSolver(P, _prm(tol=1e-10))
    assert S.SetBorder(V, W, Cm) == 0
    P.Compute()
    S.setShift(1.0, sigma)
    b, t = rng.uniform(-1, 1, N), rng.uniform(-1, 1, m)
    x, s = S.ApplyInverse(torch.from_numpy(b).to(dev), t)
    full = np.block([[A.toarray() + sigma * np.eye(N), V], [W.T, Cm]])
    ref = np.linalg.solve(full, np.concatenate([b, t]))
    got = np.concatenate([x.cpu().numpy(), s])
    print("bordered, shift (1, %g): %d iterations, |[x; s] - dense| / |dense| = %.3e" % (sigma, S.getNumIter(), np.linalg.norm(got - ref) / np.linalg.norm(ref)))
    assert np.linalg.norm(got - ref) <= 1e-6 * np.linalg.norm(ref)
