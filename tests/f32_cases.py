"""Checks of the FP32 storage of the interior factor panels ("MI Factor Storage" = "single"),
shared by tests/test_f32_panels.py (TEST-ONLY simulator tests/f32_sim, CPU) and tests/test_f32_panels_gpu.py (the
product library on the MI355X, through tests/f32_child.py).  Every check takes the library and the torch device of
the vectors, prints the figures it is about to judge and raises AssertionError.

The sharp check is bitwise: FP32 storage against a second handle in FP64 storage whose panels were rounded through
float in place (test-only switch HYMLS_MI_ROUND_PANELS=1).  Both read the same values and add them in the same order."""
import math
import os

import numpy as np
import torch

import hymls_amd
from common import problem, xml_params

# eq, n, sx, "Number of Levels" (k-level method = k - 1), cx, partitioner
CASES = [
    ("Laplace", 16, 4, 1, -1, "Cartesian"),             # two-level
    ("Laplace", 32, 4, 1, -1, "Cartesian"),             # two-level
    ("Stokes-C", 16, 8, 0, -1, "Skew Cartesian"),       # one-level
    ("Stokes-C", 32, 8, 2, 2, "Skew Cartesian"),        # three-level
]
CASE_IDS = ["laplace16_2level", "laplace32_2level", "stokes16_1level", "stokes32_3level"]
NVECS = (1, 2, 3, 5)
# coarse cap on |x32 - x64| / |x64|: sqrt(2^-24); a wrong or misplaced panel gives errors of order 1 (the bitwise
# check is the precise one)
CAP = math.sqrt(2.0 ** -24)


def case_params(case):
    eq, n, sx, levels, cx, part = case
    return xml_params(eq, n, sx, levels, cx=cx, partitioner=part)


def make(A, tv, prm, lib, storage=None, rounded=False):
    """a computed handle; storage None: the setter is never called; rounded: FP64 storage of float-rounded panels"""
    P = hymls_amd.Preconditioner(A, prm, testVector=tv, lib=lib)
    if storage is not None:
        P.SetFactorStorage(storage)
    assert "HYMLS_MI_ROUND_PANELS" not in os.environ
    if rounded:
        os.environ["HYMLS_MI_ROUND_PANELS"] = "1"
    try:
        P.Compute()
    finally:
        os.environ.pop("HYMLS_MI_ROUND_PANELS", None)
    return P


def apply(P, B, dev):
    """ApplyInverse of an (n, nv) host array: host pointers on the simulator, device pointers on the GPU"""
    if dev == "cpu":
        return P.ApplyInverse(B)
    Bt = torch.from_numpy(np.ascontiguousarray(B.T if B.ndim == 2 else B)).to(dev)
    X = P.ApplyInverse(Bt).cpu().numpy()
    return X.T if B.ndim == 2 else X


def rhs(n, nv, seed=7):
    rng = np.random.default_rng(seed + nv)
    return rng.uniform(-1, 1, (n, nv)) if nv > 1 else rng.uniform(-1, 1, n)


def fused_share(P64, P32):
    """(FP64 bytes of the panels stored in FP32 on the finest level, the same on the coarser levels): apply_bytes counts
    both sweeps of both solves, 2 x 8 B against 2 x 4 B per entry, so the difference of the figures of the two storages is
    the FP64 size of the demoted slabs; which = 1 is the finest level, 4 the coarser ones"""
    return P64.apply_bytes(1) - P32.apply_bytes(1), P64.apply_bytes(4) - P32.apply_bytes(4)


def check_case(lib, dev, case):
    """cases 1, 2 and 5 of the issue on one problem: bitwise against rounded FP64 panels, really FP32, byte figures"""
    eq, n = case[0], case[1]
    A, tv = problem(eq, n)
    prm = case_params(case)
    P64, P32, PR = make(A, tv, prm, lib), make(A, tv, prm, lib, "single"), make(A, tv, prm, lib, rounded=True)
    assert P64.FactorStorage() == "double" and P32.FactorStorage() == "single" and PR.FactorStorage() == "double"
    figures = {}
    for nv in NVECS:
        B = rhs(A.shape[0], nv)
        x64, x32, xr = apply(P64, B, dev), apply(P32, B, dev), apply(PR, B, dev)
        rel = float(np.linalg.norm(x32 - x64) / np.linalg.norm(x64))
        nbad = int(np.count_nonzero(x32 != xr))
        print("f32 panels %s %d^3 levels %d nvec %d: entries that differ from rounded FP64 panels %d, |x32 - x64| / |x64| = %.3e"
              % (eq, n, case[3], nv, nbad, rel), flush=True)
        figures["nvec%d" % nv] = rel
        assert np.isfinite(x32).all()
        assert nbad == 0 and np.array_equal(x32, xr), (case, nv, nbad)
        assert 0.0 < rel < CAP, (case, nv, rel)
    # bytes: every class of every level of these cases is solved by the fused kernel, so the panel figure halves exactly
    b64, b32 = P64.apply_bytes(1), P32.apply_bytes(1)
    fine, coarse = fused_share(P64, P32)
    r64, r32 = P64.apply_bytes(9), P32.apply_bytes(9)
    print("  bytes: which=1 %.0f -> %.0f, which=9 %.0f -> %.0f, sparse-equivalent %.0f / %.0f"
          % (b64, b32, r64, r32, P64.apply_bytes(6), P32.apply_bytes(6)), flush=True)
    assert b64 > 0 and b32 == b64 / 2
    assert P32.apply_bytes(6) == P64.apply_bytes(6) and P32.apply_bytes(7) == P64.apply_bytes(7)
    assert P64.apply_bytes(0) - P32.apply_bytes(0) == fine + coarse
    assert fine > 0 and coarse >= 0 and r32 == r64 - (fine + coarse) / 2
    assert PR.apply_bytes(9) == r64 and PR.apply_bytes(1) == b64
    return figures


def check_defaults(lib, dev):
    """case 3: never calling the setter and calling it with 64 give the same bits"""
    case = CASES[0]
    A, tv = problem(case[0], case[1])
    prm = case_params(case)
    Pa, Pb = make(A, tv, prm, lib), make(A, tv, prm, lib, "double")
    assert lib.hymls_mi_factor_storage(Pa._h) == 64 and lib.hymls_mi_factor_storage(Pb._h) == 64
    for nv in (1, 3):
        B = rhs(A.shape[0], nv)
        assert np.array_equal(apply(Pa, B, dev), apply(Pb, B, dev))


def check_lifecycle(lib, dev):
    """case 4 (the return value of the unchanged tests/hostsim library is checked by the simulator test itself)"""
    case = CASES[0]
    A, tv = problem(case[0], case[1])
    prm = case_params(case)
    n = A.shape[0]
    B = rhs(n, 1)
    fresh = {s: apply(make(A, tv, prm, lib, s), B, dev) for s in ("double", "single")}
    assert not np.array_equal(fresh["double"], fresh["single"])
    P = make(A, tv, prm, lib)
    K = (A.indptr, A.indices, A.data)
    # a changed value: not computed until the next Compute; the same value again changes nothing
    assert P.SetFactorStorage("double") == 0 and P.IsComputed()
    assert P.SetFactorStorage("single") == 0 and not P.IsComputed() and P.IsInitialized()
    out = np.empty(n)
    assert lib.hymls_mi_apply_inverse(P._h, B.ctypes.data, n, out.ctypes.data, n, 1, 0) == -1
    # 32 -> 64 -> 32 with SetMatrix in between: each time the bits of a fresh handle in that storage
    for storage in ("single", "double", "single"):
        P.SetFactorStorage(storage)
        P.SetMatrix(K)
        assert not P.IsComputed()
        P.Compute()
        assert P.FactorStorage() == storage
        assert np.array_equal(apply(P, B, dev), fresh[storage]), storage
    # Compute twice in FP32: bitwise repeatable (the FP64 slab is obtained again, filled and released)
    r9 = P.apply_bytes(9)
    P.Compute()
    assert np.array_equal(apply(P, B, dev), fresh["single"]) and P.apply_bytes(9) == r9
    # any other width
    assert lib.hymls_mi_set_factor_storage(P._h, 16) == -2 and lib.hymls_mi_factor_storage(P._h) == 32 and P.IsComputed()
    assert lib.hymls_mi_set_factor_storage(P._h, 0) == -2
    # border and FP32 storage, in both orders
    V = np.random.default_rng(3).uniform(-1, 1, (n, 1))
    try:
        P.SetBorder(V)
        raise AssertionError("SetBorder on a handle with FP32 storage was accepted")
    except hymls_amd.HymlsError as e:
        assert e.code == -99 and "FP32" in str(e), e
    assert P.IsComputed() and np.array_equal(apply(P, B, dev), fresh["single"])
    Pb = make(A, tv, prm, lib)
    Pb.SetBorder(V)
    assert lib.hymls_mi_set_factor_storage(Pb._h, 32) == -99 and "border" in lib.hymls_mi_last_error(Pb._h).decode()
    assert lib.hymls_mi_factor_storage(Pb._h) == 64
    Pb.SetBorder(None)
    assert lib.hymls_mi_set_factor_storage(Pb._h, 32) == 0
    Pb.Compute()
    assert np.array_equal(apply(Pb, B, dev), fresh["single"])


def check_python_and_xml(lib, dev, tmp_dir):
    """case 9: the parameter-list key, the method and the XML driver's reader give the same thing"""
    from hymls_amd.driver import read_parameters
    case = CASES[0]
    A, tv = problem(case[0], case[1])
    B = rhs(A.shape[0], 2)
    prm = case_params(case)
    x_method = apply(make(A, tv, prm, lib, "single"), B, dev)
    keyed = case_params(case)
    keyed["Preconditioner"]["MI Factor Storage"] = "single"
    Pk = hymls_amd.Preconditioner(A, keyed, testVector=tv, lib=lib)
    assert Pk.FactorStorage() == "single"
    Pk.Compute()
    assert np.array_equal(apply(Pk, B, dev), x_method)
    xml = os.path.join(str(tmp_dir), "f32.xml")
    with open(xml, "w") as f:
        f.write('<ParameterList name="HYMLS"><ParameterList name="Problem">'
                '<Parameter name="Equations" type="string" value="Laplace"/><Parameter name="Dimension" type="int" value="3"/>'
                '<Parameter name="nx" type="int" value="16"/><Parameter name="ny" type="int" value="16"/>'
                '<Parameter name="nz" type="int" value="16"/></ParameterList><ParameterList name="Preconditioner">'
                '<Parameter name="Separator Length" type="int" value="4"/><Parameter name="Number of Levels" type="int" value="1"/>'
                '<Parameter name="Partitioner" type="string" value="Cartesian"/>'
                '<Parameter name="MI Factor Storage" type="string" value="single"/></ParameterList></ParameterList>')
    from_xml = read_parameters(xml)
    assert from_xml["Preconditioner"]["MI Factor Storage"] == "single"
    Px = hymls_amd.Preconditioner(A, from_xml, testVector=tv, lib=lib)
    Px.Compute()
    assert Px.FactorStorage() == "single" and np.array_equal(apply(Px, B, dev), x_method)
    for bad in ("half", 32, ""):
        wrong = case_params(case)
        wrong["Preconditioner"]["MI Factor Storage"] = bad
        try:
            hymls_amd.Preconditioner(A, wrong, testVector=tv, lib=lib)
            raise AssertionError("unknown storage %r accepted" % (bad,))
        except hymls_amd.HymlsError as e:
            assert e.code == -2, e


GMRES = {"Krylov Method": "GMRES", "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 1000,
                                                        "Num Blocks": 100, "Maximum Restarts": 40}}


def check_solver(lib, dev, n):
    """case 7: Stokes-C n^3 three-level Skew, right-preconditioned GMRES(100) to 1e-8 through hymls_amd.Solver and the native
    solver, in both storages.  True residual ||b - K x|| / ||b|| in FP64 on the host: below 1e-7, the bound the existing
    solver tests put on their FP64 runs at this tolerance (tests/test_native_solver.py).  Iterations with FP32 storage:
    at most max(2, 5 %) more than with FP64 storage in this same run."""
    A, tv = problem("Stokes-C", n)
    prm = xml_params("Stokes-C", n, 8, 2, cx=2 if n == 32 else -1, partitioner="Skew Cartesian")
    b = A @ np.random.default_rng(11).uniform(-1, 1, A.shape[0])
    res = {}
    for storage in ("double", "single"):
        P = make(A, tv, prm, lib, storage)
        for name, S in (("python", hymls_amd.Solver(P, P, {"Solver": GMRES})), ("native", hymls_amd.NativeSolver(P, {"Solver": GMRES}))):
            x = S.ApplyInverse(torch.from_numpy(b).to(dev)).cpu().numpy()
            rr = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
            res[(name, storage)] = (S.getNumIter(), rr)
            print("f32 panels solver Stokes-C %d^3 %s storage, %s solver: %d iterations, true residual %.3e"
                  % (n, storage, name, S.getNumIter(), rr), flush=True)
    for name in ("python", "native"):
        (i64, r64), (i32, r32) = res[(name, "double")], res[(name, "single")]
        assert r64 < 1e-7 and r32 < 1e-7, res
        assert i32 - i64 <= max(2, math.ceil(0.05 * i64)), res
    return {"%s_%s" % k: v for k, v in res.items()}


def check_overflow(lib, dev):
    """case 6: three interior unknowns of a Laplace 8^3 matrix scaled by 1e-20 (rows and columns): the inverted pivot block
    holds entries of order 1e39.  FP64 storage computes and applies it; FP32 storage refuses in Compute."""
    import scipy.sparse as sp
    A, tv = problem("Laplace", 8)
    prm = xml_params("Laplace", 8, 4, 1)
    P0 = hymls_amd.Preconditioner(A, prm, testVector=tv, lib=lib)
    P0.Initialize()
    d = np.ones(A.shape[0])
    d[P0.interior(0, 0)[:3]] = 1e-20
    As = (sp.diags(d) @ A @ sp.diags(d)).tocsr()
    P64 = make(As, tv, prm, lib, "double")
    x = apply(P64, np.ones(A.shape[0]), dev)
    assert np.isfinite(x).all() and np.abs(x).max() > 3.5e38        # (beyond FLT_MAX: the entries that do not fit)
    P32 = hymls_amd.Preconditioner(As, prm, testVector=tv, lib=lib)
    P32.SetFactorStorage("single")
    try:
        P32.Compute()
        raise AssertionError("Compute with FP32 storage accepted panel entries beyond FLT_MAX")
    except hymls_amd.HymlsError as e:
        assert e.code == -4 and "FP32" in str(e), e
    assert not P32.IsComputed()
    P32.SetFactorStorage("double")        # the handle recovers in FP64 storage
    P32.Compute()
    assert np.array_equal(apply(P32, np.ones(A.shape[0]), dev), x)
