"""Checks of the lock-step columns of the native Krylov solver (hymls_mi_solver_set_lockstep, hymls_mi_matvec_mv,
hymls_mi_orthogonalize_mv[_f32], "MI Lockstep Columns"), shared by tests/test_lockstep.py (the TEST-ONLY simulator of
tests/krylov_lockstep_sim, CPU tensors) and tests/test_lockstep_gpu.py (the product library on the MI355X).
Every check takes (lib, dev) and is bitwise: a column of a lock-step solve does the arithmetic of its own single-column
solve, so nothing here has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hymls_amd
from hymls_amd.native_solver import (bind_lockstep, bind_bordered, matvec_mv, orthogonalize, orthogonalize_f32, orthogonalize_mv,
                                     orthogonalize_mv_f32)
from common import problem, xml_params
from oracle import galeri

K_SETS = ((5, 5, 5, 5), (1, 7, 100, 251), (251, 1))
_PREC = {}


def small_prec(lib):
    if ("small", id(lib)) not in _PREC:
        A, tv = problem("Laplace", 8)
        P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 1), testVector=tv, lib=lib)
        P.Initialize()
        P.Compute()
        _PREC[("small", id(lib))] = (A, P)
    return _PREC[("small", id(lib))]


def prec(lib, name):
    """computed preconditioners, one per library and problem (kept for the session: the checks only solve with them)"""
    key = (name, id(lib))
    if key not in _PREC:
        if name == "laplace8":
            return small_prec(lib)
        if name == "laplace16":
            A, tv = problem("Laplace", 16)
            prm = xml_params("Laplace", 16, 4, 1)
        elif name == "stokes16":
            A, tv = problem("Stokes-C", 16)
            prm = xml_params("Stokes-C", 16, 4, 1, -1, "Skew Cartesian")
        elif name == "oseen8":
            A = galeri.oseen3d(8, 8, 8, 100.0)
            tv = galeri.create_testvector(A)
            prm = xml_params("Stokes-C", 8, 4, 1, -1, "Skew Cartesian")
        elif name in ("stokes32", "stokes32_single"):
            A, tv = problem("Stokes-C", 32)
            extra = {"MI Factor Storage": "single"} if name.endswith("single") else None
            prm = xml_params("Stokes-C", 32, 4, 2, -1, "Skew Cartesian", extra=extra)
        P = hymls_amd.Preconditioner(A, prm, testVector=tv, lib=lib)
        P.Initialize()
        P.Compute()
        _PREC[key] = (A.tocsr(), P)
    return _PREC[key]


# ---------------------------------------------------------------- 1. orthogonalize_mv against nb single calls
def _exact(cols, ld, n, dtype):
    """the columns (n x m) with leading dimension ld in exactly (m - 1) * ld + n entries"""
    m = cols.shape[1]
    flat = np.zeros((m - 1) * ld + n, dtype=dtype)
    for j in range(m):
        flat[j * ld:j * ld + n] = cols[:, j]
    return flat


def _exact_t(rows, ld):
    """torch: the columns rows[j] (m x n, one column per row) with leading dimension ld in exactly (m - 1) * ld + n entries"""
    m, n = rows.shape
    flat = torch.zeros((m - 1) * ld + n, dtype=rows.dtype, device=rows.device)
    torch.as_strided(flat, (m, n), (ld, 1)).copy_(rows)
    return flat


@functools.lru_cache(maxsize=2)
def _orth_data(n, dev):
    """a basis of 251 columns and four vectors, generated once per size where the check runs (seeded)"""
    g = torch.Generator(device=dev)
    g.manual_seed(500 + n % 9973)
    V = (torch.rand((251, n), dtype=torch.float64, device=dev, generator=g) * 2 - 1) / n ** 0.5
    W = torch.rand((4, n), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    return V, W


def check_orthogonalize_mv(lib, dev, n, ks, f32):
    """every column of one batched call against hymls_mi_orthogonalize[_f32] with its own k: coefficients, norm, the
    orthogonalised vector and (FP32 basis) the rounded next column, bit for bit.  The columns of a batch have bases of
    their own (column v: the basis scaled by v + 1), the arrays are exactly sized, and every nb <= len(ks) is run."""
    A, P = small_prec(lib)
    Vn, Wn = _orth_data(n, dev)
    tt = torch.float32 if f32 else torch.float64
    ldw = n + 5
    for ldv in (n, n + 5):
        bases = [_exact_t((Vn[:k] * (v + 1)).to(tt), ldv) for v, k in enumerate(ks)]
        singles = []
        for v, k in enumerate(ks):
            w = Wn[v].clone()
            if f32:
                vn = torch.zeros(n, dtype=torch.float32, device=dev)
                h, nrm = orthogonalize_f32(P, n, k, bases[v], ldv, w, vn)
                singles.append((h, nrm, w, vn))
            else:
                h, nrm = orthogonalize(P, n, k, bases[v], ldv, w)
                singles.append((h, nrm, w, None))
        for nb in range(1, len(ks) + 1):
            kk = ks[:nb]
            vstride = (max(kk) - 1) * ldv + n           # the bases of the batch back to back, each exactly sized
            Vb = torch.zeros(nb * vstride, dtype=tt, device=dev)
            for v in range(nb):
                Vb[v * vstride:v * vstride + bases[v].numel()] = bases[v]
            for with_next in ((True, False) if f32 else (False,)):
                Wb = _exact_t(Wn[:nb], ldw)
                if f32:
                    nxt = torch.zeros((nb - 1) * (n + 3) + n, dtype=torch.float32, device=dev) if with_next else None
                    hs, nrms = orthogonalize_mv_f32(P, n, kk, Vb, ldv, vstride, Wb, ldw, nxt, n + 3)
                else:
                    hs, nrms = orthogonalize_mv(P, n, kk, Vb, ldv, vstride, Wb, ldw)
                for v in range(nb):
                    h, nrm, w, vn = singles[v]
                    assert np.array_equal(hs[v], h), (n, kk, v, ldv)
                    assert nrms[v] == nrm, (n, kk, v, ldv)
                    assert torch.equal(Wb[v * ldw:v * ldw + n], w), (n, kk, v, ldv)
                    if f32 and with_next:
                        assert torch.equal(nxt[v * (n + 3):v * (n + 3) + n], vn), (n, kk, v, ldv)
            del Vb


def check_orthogonalize_mv_refusals(lib, dev):
    A, P = small_prec(lib)
    n = 64
    V = torch.zeros(4 * 8 * n, dtype=torch.float64, device=dev)
    W = torch.zeros(5 * n, dtype=torch.float64, device=dev)
    for ks, ldv in (((), n), ((2, 2, 2, 2, 2), n), ((0, 2), n), ((2, 257), n), ((2, 2), n - 1)):
        with pytest.raises(hymls_amd.HymlsError) as e:
            orthogonalize_mv(P, n, ks, V, ldv, 8 * n, W, n)
        assert e.value.code == -2, (ks, ldv)
        with pytest.raises(hymls_amd.HymlsError) as e:
            orthogonalize_mv_f32(P, n, ks, V.float(), ldv, 8 * n, W, n)
        assert e.value.code == -2, (ks, ldv)
    orthogonalize_mv(P, n, (2, 2), V, n, 8 * n, W, n)      # and the valid call next to them passes


# ---------------------------------------------------------------- 2. matvec_mv against column-wise matvec
def check_matvec_mv(lib, dev, name):
    A, P = prec(lib, name)
    n = P._n
    rng = np.random.default_rng(77)
    Xn = rng.uniform(-1, 1, (n, 5))
    ref = [P.MatVec(torch.from_numpy(Xn[:, v].copy()).to(dev)) for v in range(5)]
    for v in range(5):                                     # the single-vector product itself against scipy, loosely
        assert np.abs(ref[v].cpu().numpy() - A @ Xn[:, v]).max() <= 1e-9 * np.abs(A).sum(axis=1).max()
    for nvec in range(1, 6):
        for ld in (n, n + 3):
            X = torch.from_numpy(_exact(Xn[:, :nvec], ld, n, np.float64)).to(dev)
            Y = torch.full(((nvec - 1) * ld + n,), np.nan, dtype=torch.float64, device=dev)
            matvec_mv(P, X, ld, Y, ld, nvec)
            Yh = np.full((nvec - 1) * ld + n, np.nan)
            matvec_mv(P, X.cpu().numpy(), ld, Yh, ld, nvec)      # host pointers
            for v in range(nvec):
                assert torch.equal(Y[v * ld:v * ld + n], ref[v]), (name, nvec, ld, v)
                assert np.array_equal(Yh[v * ld:v * ld + n], ref[v].cpu().numpy()), (name, nvec, ld, v)


# ---------------------------------------------------------------- helpers of the solves
def _prm(method="GMRES", tol=1e-8, maxit=300, blocks=30, restarts=20, width=1, **sol):
    d = {"Krylov Method": method, "MI Lockstep Columns": width,
         "Iterative Solver": {"Convergence Tolerance": tol, "Maximum Iterations": maxit, "Num Blocks": blocks, "Maximum Restarts": restarts}}
    d.update(sol)
    return d


def _solve(S, B, dev):
    """(return code, X, per-column results) of one hymls_mi_solver_solve on the columns of B (n x nvec numpy)"""
    n, nvec = B.shape
    Bt = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)          # (nvec, n): column-major n x nvec
    X = torch.full_like(Bt, np.nan)
    code = S._lib.hymls_mi_solver_solve(S._s, Bt.data_ptr(), n, X.data_ptr(), n, nvec, 1)
    cols = S.getColumnResults()
    assert len(cols) == nvec
    assert (S.getNumIter(), S.achievedTol(), S.getNumRestarts()) == (cols[-1]["iterations"], cols[-1]["achieved_tol"], cols[-1]["restarts"]) \
        or np.isnan(S.achievedTol())
    return code, X, cols


def _same(a, b):
    """two (code, X, cols) results are the same bits"""
    return a[0] == b[0] and torch.equal(a[1], b[1]) and a[2] == b[2]


def stokes_columns(A, nvec):
    """columns that end at different iterations: K*ones, a random vector, K*ones + 1e-6 random, zero, K*e_1"""
    n = A.shape[0]
    rng = np.random.default_rng(91)
    e1 = np.zeros(n); e1[0] = 1.0
    cols = [A @ np.ones(n), rng.uniform(-1, 1, n), A @ np.ones(n) + 1e-6 * rng.uniform(-1, 1, n), np.zeros(n), A @ e1]
    return np.stack(cols[:nvec], axis=1)


# ---------------------------------------------------------------- 3. GMRES in lock-step against width 1
def check_gmres(lib, dev, storage, right, start, nvec, width, variant="converge"):
    A, P = prec(lib, "stokes16")
    B = stokes_columns(A, nvec)
    # tolerance 1e-6 and at most 150 iterations keep the simulator run short: the columns still restart and end apart
    kw = {"Left or Right Preconditioning": "Right" if right else "Left", "Initial Vector": start, "MI Basis Storage": storage,
          "tol": 1e-6, "maxit": 150}
    if variant == "maxit":
        kw.update(maxit=20)
    elif variant == "norestart":
        kw.update(restarts=0)
    S = hymls_amd.NativeSolver(P, _prm(width=1, **kw))
    one = _solve(S, B, dev)
    S.setParameterList(_prm(width=width, **kw))
    assert S.getLockstep() == width
    lock = _solve(S, B, dev)
    its = [c["iterations"] for c in lock[2]]
    print("GMRES(30) %s basis %s %s nvec %d width %d %s: code %d iterations %s restarts %s" % (
        storage, "right" if right else "left", start, nvec, width, variant, lock[0], its, [c["restarts"] for c in lock[2]]))
    assert _same(one, lock), (one[0], lock[0], one[2], lock[2])
    if variant == "maxit":
        assert lock[0] == -1 and max(its) == 20 and torch.isfinite(lock[1]).all()
    if variant == "converge":
        # (the random right-hand side may stagnate under GMRES(30) until the iterations run out: the status says so)
        assert lock[0] == (0 if all(c["converged"] for c in lock[2]) else -1) and lock[2][0]["converged"]
        if start == "Zero" and right:
            assert max(c["restarts"] for c in lock[2]) >= 1        # GMRES(30) restarts on this problem
            for g0 in range(0, nvec, width):                        # the drop-out path: a group whose columns end apart
                if len(its[g0:g0 + width]) > 1:
                    assert len(set(its[g0:g0 + width])) > 1, its
        if nvec >= 4 and start == "Zero":
            assert its[3] == 0 and lock[2][3]["achieved_tol"] == 0.0 and not lock[1][3].any()   # the zero column
    S.close()


def check_gmres_large(lib, dev, storage, name="stokes32"):
    """GPU only: Stokes-C 32^3 three-level, GMRES(100), 4 columns, widths 1, 2 and 4"""
    A, P = prec(lib, name)
    n = A.shape[0]
    rng = np.random.default_rng(92)
    B = np.stack([A @ np.ones(n), A @ rng.uniform(-1, 1, n), 1e-3 * (A @ rng.uniform(-1, 1, n)), A @ np.sin(np.arange(n))], axis=1)
    kw = {"MI Basis Storage": storage}
    S = hymls_amd.NativeSolver(P, _prm(blocks=100, maxit=600, width=1, **kw))
    one = _solve(S, B, dev)
    assert one[0] == 0, one[2]
    for width in (2, 4):
        S.setParameterList(_prm(blocks=100, maxit=600, width=width, **kw))
        lock = _solve(S, B, dev)
        print("Stokes-C 32^3 %s %s width %d: code %d iterations %s" % (name, storage, width, lock[0], [c["iterations"] for c in lock[2]]))
        assert _same(one, lock), (width, one[2], lock[2])
    S.close()


# ---------------------------------------------------------------- 4. CG
def check_cg(lib, dev, width):
    A, P = prec(lib, "laplace16")
    n = A.shape[0]
    rng = np.random.default_rng(93)
    B = np.stack([A @ np.ones(n), rng.uniform(-1, 1, n), np.zeros(n), A @ rng.uniform(-1, 1, n) * 1e-3], axis=1)
    for start, maxit in (("Zero", 100), ("Random", 100), ("Zero", 3)):
        S = hymls_amd.NativeSolver(P, _prm("CG", tol=1e-10, maxit=maxit, width=1, **{"Initial Vector": start}))
        one = _solve(S, B, dev)
        S.setParameterList(_prm("CG", tol=1e-10, maxit=maxit, width=width, **{"Initial Vector": start}))
        lock = _solve(S, B, dev)
        print("CG %s maxit %d width %d: code %d iterations %s" % (start, maxit, width, lock[0], [c["iterations"] for c in lock[2]]))
        assert _same(one, lock), (one[2], lock[2])
        assert lock[0] == (0 if maxit == 100 else -1)
        if start == "Zero":
            assert lock[2][2]["iterations"] == 0 and not lock[1][2].any()
            assert len({c["iterations"] for c in lock[2]}) > 1
        S.close()


# ---------------------------------------------------------------- 5. "Previous"
def check_previous(lib, dev):
    """width 2, nvec 4, two calls: every column of a group starts from the solution stored before the group (the last
    column of the preceding group or call).  A width-1 solver is given that start vector through a preceding solve: a
    "Previous" solve of one column after a solve whose last column is the wanted vector."""
    A, P = prec(lib, "laplace16")
    n = A.shape[0]
    rng = np.random.default_rng(94)
    B1, B2 = rng.uniform(-1, 1, (n, 4)), rng.uniform(-1, 1, (n, 4))
    prm = dict(tol=1e-6, maxit=100, blocks=30, **{"Initial Vector": "Previous"})
    S = hymls_amd.NativeSolver(P, _prm(width=2, **prm))
    r1 = _solve(S, B1, dev)
    r2 = _solve(S, B2, dev)
    assert r1[0] == 0 and r2[0] == 0

    # the start vectors are reproduced with the width-1 solver's own mechanism: it solves the right-hand sides whose
    # solutions lead to the wanted start vector, one after the other, then the wanted column
    def chain(seed_b, b, seed_start):
        """result of solving b at width 1 from the stored solution of a preceding width-1 solve of seed_b (itself started
        from seed_start: a list of right-hand sides solved before it, oldest first)"""
        T = hymls_amd.NativeSolver(P, _prm(width=1, **prm))
        for sb in seed_start + [seed_b]:
            _solve(T, sb.reshape(n, 1), dev)
        out = _solve(T, b.reshape(n, 1), dev)
        T.close()
        return out

    # call 1: group (0, 1) starts from nothing stored (zero), group (2, 3) from the solution of column 1
    fresh = [_solve(hymls_amd.NativeSolver(P, _prm(width=1, **prm)), B1[:, c:c + 1], dev) for c in (0, 1)]
    for c in (0, 1):
        assert torch.equal(r1[1][c], fresh[c][1][0]) and r1[2][c] == fresh[c][2][0], c
    for c in (2, 3):
        want = chain(B1[:, 1], B1[:, c], [])
        assert torch.equal(r1[1][c], want[1][0]) and r1[2][c] == want[2][0], c
    # call 2: group (0, 1) starts from the solution of column 3 of call 1 (which started from column 1 of call 1),
    # group (2, 3) from the solution of column 1 of call 2
    for c in (0, 1):
        want = chain(B1[:, 3], B2[:, c], [B1[:, 1]])
        assert torch.equal(r2[1][c], want[1][0]) and r2[2][c] == want[2][0], c
    for c in (2, 3):
        want = chain(B2[:, 1], B2[:, c], [B1[:, 1], B1[:, 3]])
        assert torch.equal(r2[1][c], want[1][0]) and r2[2][c] == want[2][0], c
    # width back to 1: column after column again, each from the one before; the stored solution is column 3 of call 2
    S.setParameterList(_prm(width=1, **prm))
    r3 = _solve(S, B1[:, :2], dev)
    T = hymls_amd.NativeSolver(P, _prm(width=1, **prm))
    for sb in (B1[:, 1], B1[:, 3], B2[:, 1], B2[:, 3]):
        _solve(T, sb.reshape(n, 1), dev)
    want = _solve(T, B1[:, :2], dev)
    assert _same(r3, want)
    S.close()
    T.close()


# ---------------------------------------------------------------- 6. life cycle and refusals
def check_life_cycle(lib, dev):
    bind_lockstep(lib)
    A, P = prec(lib, "laplace16")
    n = A.shape[0]
    B = np.random.default_rng(95).uniform(-1, 1, (n, 4))
    S = hymls_amd.NativeSolver(P, _prm(blocks=10, tol=1e-9))
    for bad in (0, 5, -1):
        assert lib.hymls_mi_solver_set_lockstep(S._s, bad) == -2
        assert S.getLockstep() == 1
    with pytest.raises(ValueError):
        hymls_amd.NativeSolver(P, _prm(width=5))
    one = {blocks: None for blocks in (10, 25)}
    for blocks in (10, 25):
        S.setParameterList(_prm(blocks=blocks, tol=1e-9))
        one[blocks] = _solve(S, B, dev)
    for width, blocks in ((4, 10), (1, 25), (4, 25), (2, 10), (4, 10)):     # the basis grows with the width set and with it changed
        S.setParameterList(_prm(blocks=blocks, tol=1e-9, width=width))
        assert S.getLockstep() == width
        assert _same(_solve(S, B, dev), one[blocks]), (width, blocks)
    # FP32 basis after FP64 at the same width: the per-column bases are reallocated
    S.setParameterList(_prm(blocks=10, tol=1e-9, width=1, **{"MI Basis Storage": "single"}))
    f1 = _solve(S, B, dev)
    S.setParameterList(_prm(blocks=10, tol=1e-9, width=4, **{"MI Basis Storage": "single"}))
    assert _same(_solve(S, B, dev), f1)
    # column results: out of range
    its = C.c_int()
    assert lib.hymls_mi_solver_column_result(S._s, 4, C.byref(its), None, None, None) == -2
    assert lib.hymls_mi_solver_column_result(S._s, -1, C.byref(its), None, None, None) == -2
    assert lib.hymls_mi_solver_column_result(S._s, 3, C.byref(its), None, None, None) == 0 and its.value == f1[2][3]["iterations"]
    S.close()


def check_bordered_ignores_width(lib, dev):
    bind_bordered(lib)
    A, tv = problem("Laplace", 8)
    N, m = A.shape[0], 2
    rng = np.random.default_rng(96)
    V, W, Cm = rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (N, m)), rng.uniform(-1, 1, (m, m))
    P = hymls_amd.Preconditioner(A, xml_params("Laplace", 8, 4, 1), testVector=tv, lib=lib)
    P.Initialize()
    P.SetBorder(V, W, Cm)
    P.Compute()
    b, t = torch.from_numpy(rng.uniform(-1, 1, N)).to(dev), rng.uniform(-1, 1, m)
    outs = []
    for width in (1, 4):
        S = hymls_amd.NativeBorderedSolver(P, _prm(blocks=250, width=width))
        x, s = S.ApplyInverse(b, t)
        outs.append((x, s, S.getNumIter(), S.getColumnResults()))
        S.close()
    assert torch.equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2:] == outs[1][2:]
    assert len(outs[1][3]) == 1


def missing_launchers_return_m99(lib):
    """a library whose krylov.cpp was built without HYMLS_MI_LOCKSTEP_SOLVER has every symbol; a width above 1 and the three
    building blocks return -99, and the plain solve is untouched"""
    bind_lockstep(lib)
    A, P = small_prec(lib)
    n = P._n
    S = hymls_amd.NativeSolver(P, _prm())
    assert lib.hymls_mi_solver_set_lockstep(S._s, 2) == -99 and S.getLockstep() == 1
    assert lib.hymls_mi_solver_set_lockstep(S._s, 1) == 0
    x = torch.zeros(2 * n, dtype=torch.float64)
    y = torch.zeros(2 * n, dtype=torch.float64)
    assert lib.hymls_mi_matvec_mv(P._h, x.data_ptr(), n, y.data_ptr(), n, 2, 1) == -99
    k = np.array([1, 1], dtype=np.int32)
    h, nrm = np.zeros(2), np.zeros(2)
    assert lib.hymls_mi_orthogonalize_mv(P._h, n, 2, k.ctypes.data, x.data_ptr(), n, n, y.data_ptr(), n, h.ctypes.data, 1, nrm.ctypes.data) == -99
    assert lib.hymls_mi_orthogonalize_mv_f32(P._h, n, 2, k.ctypes.data, x.float().data_ptr(), n, n, y.data_ptr(), n, None, 0, h.ctypes.data, 1,
                                             nrm.ctypes.data) == -99
    code, X, cols = _solve(S, (A @ np.ones((n, 2))), "cpu")
    assert code == 0 and len(cols) == 2
    S.close()
