"""Checks of the FP32 storage of the merged level-solve panels ("MI Merged Factor Storage" = "single", DESIGN.md
section 16), shared by tests/test_merged_f32.py (TEST-ONLY simulator tests/lvllab, CPU) and
tests/test_merged_f32_gpu.py (the product library on the MI355X, through tests/merged_f32_child.py).  Every check takes
the library and the torch device of the vectors, prints the figures it is about to judge and raises AssertionError.

The sharp check is bitwise, as in tests/f32_cases.py: FP32 storage against a second handle in FP64 storage whose
panels were rounded through float in place (test-only switch HYMLS_MI_ROUND_PANELS, a bit mask: 1 the classes of the
fused solve, 2 those of the merged level solve).  Both read the same values and add them in the same order.

A run is (problem, no_fused).  no_fused sets HYMLS_MI_NO_FUSED_SOLVE=1 while the handle is built, which puts the
classes of the finest level on the merged route too: the situation of separator length 16 at a test-sized grid.
Laplace 16^3 two-level has one LevelSolver level whose subdomains fit the fused kernel at every separator length (8^3
interiors at most), so it has a merged class only with no_fused; the as-it-is run of Stokes-C 32^3 three-level uses
separator length 4 and coarsening factor 4, with which the second level is solved on the merged route (every check
asserts apply_bytes(10) > 0 first).  Two more as-it-is runs cover the default dispatch between the two routes: Laplace
32^3 two-level with separator length 16, whose eight 15^3 interiors do not fit the fused kernel, so the whole finest level
is on the merged route without any switch, and Stokes-C 24^3 three-level (separator length 4, coarsening factor 3),
where some classes of the second level are fused and the others merged."""
import contextlib
import math
import os

import numpy as np

import hymls_amd
from common import problem, xml_params
from f32_cases import CAP, GMRES, NVECS, apply, rhs

# eq, n, sx, "Number of Levels" (k-level method = k - 1), cx, partitioner
LAPLACE = ("Laplace", 16, 4, 1, -1, "Cartesian")            # two-level
STOKES = ("Stokes-C", 32, 4, 2, 4, "Skew Cartesian")        # three-level
LAPLACE_SX16 = ("Laplace", 32, 16, 1, -1, "Cartesian")      # two-level, the finest level on the merged route as it is
STOKES24 = ("Stokes-C", 24, 4, 2, 3, "Skew Cartesian")      # three-level, fused and merged classes on the second level
# (problem, no_fused)
RUNS = [(LAPLACE, True), (STOKES, False), (STOKES, True), (LAPLACE_SX16, False), (STOKES24, False)]
RUN_IDS = ["laplace16_2level_nofused", "stokes32_3level", "stokes32_3level_nofused", "laplace32_sx16_2level", "stokes24_3level"]
# GMRES(100) to 1e-8 on STOKES: iterations of (solver, merged storage), measured on the simulator
ITERATIONS = {("python", "double"): 145, ("python", "single"): 145, ("native", "double"): 145, ("native", "single"): 145}
TOL = 1e-8


def params(case):
    eq, n, sx, levels, cx, part = case
    return xml_params(eq, n, sx, levels, cx=cx, partitioner=part)


@contextlib.contextmanager
def env(**kw):
    """environment switches of the library for the duration of a call; they must not be set outside"""
    kw = {k: v for k, v in kw.items() if v is not None}
    for k in kw:
        assert k not in os.environ, k
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in kw:
            os.environ.pop(k, None)


def all_no_fused(check):
    """the whole check with HYMLS_MI_NO_FUSED_SOLVE=1 (a later Initialize of a handle reads it again)"""
    def wrapped(*args):
        with env(HYMLS_MI_NO_FUSED_SOLVE="1"):
            return check(*args)
    wrapped.__doc__ = check.__doc__
    return wrapped


def make(A, tv, prm, lib, merged=None, fused=None, round_mask=0, no_fused=False):
    """a computed handle; merged / fused None: that setter is never called; round_mask: FP64 storage of float-rounded panels"""
    no_fused = no_fused and "HYMLS_MI_NO_FUSED_SOLVE" not in os.environ
    with env(HYMLS_MI_NO_FUSED_SOLVE="1" if no_fused else None, HYMLS_MI_ROUND_PANELS=str(round_mask) if round_mask else None):
        P = hymls_amd.Preconditioner(A, prm, testVector=tv, lib=lib)
        if merged is not None:
            P.SetMergedFactorStorage(merged)
        if fused is not None:
            P.SetFactorStorage(fused)
        P.Compute()
    return P


def check_run(lib, dev, run):
    """bitwise against rounded FP64 panels (merged alone and together with the fused switch), really FP32, byte figures"""
    case, no_fused = run
    A, tv = problem(case[0], case[1])
    prm = params(case)
    P64 = make(A, tv, prm, lib, no_fused=no_fused)
    m64 = P64.apply_bytes(10)
    print("merged f32 %s no_fused=%s: apply_bytes(10) = %.0f of %.0f" % (case, no_fused, m64, P64.apply_bytes(0)), flush=True)
    assert m64 > 0, "no class on the merged route: the case checks nothing"
    P32 = make(A, tv, prm, lib, merged="single", no_fused=no_fused)
    PR = make(A, tv, prm, lib, round_mask=2, no_fused=no_fused)
    Pboth = make(A, tv, prm, lib, merged="single", fused="single", no_fused=no_fused)
    PR3 = make(A, tv, prm, lib, round_mask=3, no_fused=no_fused)
    assert P64.MergedFactorStorage() == "double" and P32.MergedFactorStorage() == "single" and PR.MergedFactorStorage() == "double"
    assert P32.FactorStorage() == "double" and Pboth.FactorStorage() == "single" and Pboth.MergedFactorStorage() == "single"
    figures = {}
    for nv in NVECS:
        B = rhs(A.shape[0], nv)
        x64, x32, xr = apply(P64, B, dev), apply(P32, B, dev), apply(PR, B, dev)
        xb, xr3 = apply(Pboth, B, dev), apply(PR3, B, dev)
        rel = float(np.linalg.norm(x32 - x64) / np.linalg.norm(x64))
        relb = float(np.linalg.norm(xb - x64) / np.linalg.norm(x64))
        nbad, nbad3 = int(np.count_nonzero(x32 != xr)), int(np.count_nonzero(xb != xr3))
        print("  nvec %d: entries that differ from rounded FP64 panels %d (merged), %d (merged + fused); |x32 - x64| / |x64| = "
              "%.3e (merged), %.3e (merged + fused)" % (nv, nbad, nbad3, rel, relb), flush=True)
        figures["nvec%d" % nv] = [rel, relb]
        assert np.isfinite(x32).all() and np.isfinite(xb).all()
        assert nbad == 0 and np.array_equal(x32, xr), (run, nv, nbad)
        assert nbad3 == 0 and np.array_equal(xb, xr3), (run, nv, nbad3)
        assert 0.0 < rel < CAP and 0.0 < relb < CAP, (run, nv, rel, relb)
    # bytes: which = 10 halves exactly; 0, 4 (and 1 where the finest level is on the route) fall by the same amount;
    # the resident panels fall by half the FP64 size of the demoted slabs
    m32 = P32.apply_bytes(10)
    r64, r32 = P64.apply_bytes(9), P32.apply_bytes(9)
    print("  bytes: which=10 %.0f -> %.0f, which=9 %.0f -> %.0f, which=1 %.0f -> %.0f, which=4 %.0f -> %.0f"
          % (m64, m32, r64, r32, P64.apply_bytes(1), P32.apply_bytes(1), P64.apply_bytes(4), P32.apply_bytes(4)), flush=True)
    assert m32 == m64 / 2
    assert P64.apply_bytes(0) - P32.apply_bytes(0) == m64 - m32
    assert P32.apply_bytes(8) <= P64.apply_bytes(8)     # (8 takes the smaller of the stored and the sparse-equivalent figure)
    assert (P64.apply_bytes(1) - P32.apply_bytes(1)) + (P64.apply_bytes(4) - P32.apply_bytes(4)) == m64 - m32
    if no_fused:
        assert P64.apply_bytes(1) - P32.apply_bytes(1) > 0
    assert P32.apply_bytes(6) == P64.apply_bytes(6) and P32.apply_bytes(7) == P64.apply_bytes(7)
    assert r32 == r64 - (m64 - m32) / 2          # m64 - m32 = 8 B per entry = the FP64 size of the demoted slabs
    assert PR.apply_bytes(9) == r64 and PR.apply_bytes(10) == m64
    return figures


@all_no_fused
def check_defaults(lib, dev):
    """never calling the setter and calling it with 64 give the same bits; the fused switch does not move the merged one"""
    A, tv = problem(LAPLACE[0], LAPLACE[1])
    prm = params(LAPLACE)
    Pa, Pb = make(A, tv, prm, lib, no_fused=True), make(A, tv, prm, lib, merged="double", no_fused=True)
    assert lib.hymls_mi_merged_factor_storage(Pa._h) == 64 and lib.hymls_mi_merged_factor_storage(Pb._h) == 64
    assert Pa.apply_bytes(10) > 0
    for nv in (1, 3):
        B = rhs(A.shape[0], nv)
        assert np.array_equal(apply(Pa, B, dev), apply(Pb, B, dev))
    # HYMLS_MI_ROUND_PANELS = 1 keeps its meaning: the merged classes are not rounded
    Pc = make(A, tv, prm, lib, round_mask=1, no_fused=True)
    B = rhs(A.shape[0], 1)
    assert np.array_equal(apply(Pa, B, dev), apply(Pc, B, dev))
    Pd = make(A, tv, prm, lib, fused="single", no_fused=True)      # (no fused class in this run: nothing to demote)
    assert Pd.MergedFactorStorage() == "double" and Pd.apply_bytes(10) == Pa.apply_bytes(10)
    assert np.array_equal(apply(Pa, B, dev), apply(Pd, B, dev))


@all_no_fused
def check_lifecycle(lib, dev):
    """64 -> 32 -> 64 with SetMatrix in between, other widths, the border in both orders"""
    A, tv = problem(LAPLACE[0], LAPLACE[1])
    prm = params(LAPLACE)
    n = A.shape[0]
    B = rhs(n, 1)
    fresh = {s: apply(make(A, tv, prm, lib, merged=s, no_fused=True), B, dev) for s in ("double", "single")}
    assert not np.array_equal(fresh["double"], fresh["single"])
    P = make(A, tv, prm, lib, no_fused=True)
    K = (A.indptr, A.indices, A.data)
    # a changed value: not computed until the next Compute; the same value again changes nothing
    assert P.SetMergedFactorStorage("double") == 0 and P.IsComputed()
    assert P.SetMergedFactorStorage("single") == 0 and not P.IsComputed() and P.IsInitialized()
    out = np.empty(n)
    assert lib.hymls_mi_apply_inverse(P._h, B.ctypes.data, n, out.ctypes.data, n, 1, 0) == -1
    r9 = {}
    for storage in ("single", "double", "single", "double"):
        P.SetMergedFactorStorage(storage)
        P.SetMatrix(K)
        assert not P.IsComputed()
        P.Compute()
        assert P.MergedFactorStorage() == storage and P.FactorStorage() == "double"
        assert np.array_equal(apply(P, B, dev), fresh[storage]), storage
        assert r9.setdefault(storage, P.apply_bytes(9)) == P.apply_bytes(9)
    assert r9["single"] == r9["double"] - P.apply_bytes(10) / 4
    # Compute twice in FP32: bitwise repeatable (the FP64 slab is obtained again, filled and released)
    P.SetMergedFactorStorage("single")
    P.Compute()
    P.Compute()
    assert np.array_equal(apply(P, B, dev), fresh["single"]) and P.apply_bytes(9) == r9["single"]
    # any other width
    assert lib.hymls_mi_set_merged_factor_storage(P._h, 16) == -2 and lib.hymls_mi_merged_factor_storage(P._h) == 32 and P.IsComputed()
    assert lib.hymls_mi_set_merged_factor_storage(P._h, 0) == -2
    # border and FP32 storage, in both orders
    V = np.random.default_rng(3).uniform(-1, 1, (n, 1))
    try:
        P.SetBorder(V)
        raise AssertionError("SetBorder on a handle with FP32 merged storage was accepted")
    except hymls_amd.HymlsError as e:
        assert e.code == -99 and "FP32 merged" in str(e), e
    assert P.IsComputed() and np.array_equal(apply(P, B, dev), fresh["single"])
    Pb = make(A, tv, prm, lib, no_fused=True)
    Pb.SetBorder(V)
    assert lib.hymls_mi_set_merged_factor_storage(Pb._h, 32) == -99 and "border" in lib.hymls_mi_last_error(Pb._h).decode()
    assert lib.hymls_mi_merged_factor_storage(Pb._h) == 64
    Pb.SetBorder(None)
    assert lib.hymls_mi_set_merged_factor_storage(Pb._h, 32) == 0
    Pb.Compute()
    assert np.array_equal(apply(Pb, B, dev), fresh["single"])


@all_no_fused
def check_python_and_xml(lib, dev, tmp_dir):
    """the parameter-list key, the method and the XML driver's reader give the same thing"""
    from hymls_amd.driver import read_parameters
    A, tv = problem(LAPLACE[0], LAPLACE[1])
    B = rhs(A.shape[0], 2)
    prm = params(LAPLACE)
    x_method = apply(make(A, tv, prm, lib, merged="single", no_fused=True), B, dev)
    keyed = params(LAPLACE)
    keyed["Preconditioner"]["MI Merged Factor Storage"] = "single"
    Pk = hymls_amd.Preconditioner(A, keyed, testVector=tv, lib=lib)
    assert Pk.MergedFactorStorage() == "single" and Pk.FactorStorage() == "double"
    Pk.Compute()
    assert np.array_equal(apply(Pk, B, dev), x_method)
    xml = os.path.join(str(tmp_dir), "merged_f32.xml")
    with open(xml, "w") as f:
        f.write('<ParameterList name="HYMLS"><ParameterList name="Problem">'
                '<Parameter name="Equations" type="string" value="Laplace"/><Parameter name="Dimension" type="int" value="3"/>'
                '<Parameter name="nx" type="int" value="16"/><Parameter name="ny" type="int" value="16"/>'
                '<Parameter name="nz" type="int" value="16"/></ParameterList><ParameterList name="Preconditioner">'
                '<Parameter name="Separator Length" type="int" value="4"/><Parameter name="Number of Levels" type="int" value="1"/>'
                '<Parameter name="Partitioner" type="string" value="Cartesian"/>'
                '<Parameter name="MI Merged Factor Storage" type="string" value="single"/></ParameterList></ParameterList>')
    from_xml = read_parameters(xml)
    assert from_xml["Preconditioner"]["MI Merged Factor Storage"] == "single"
    Px = hymls_amd.Preconditioner(A, from_xml, testVector=tv, lib=lib)
    Px.Compute()
    assert Px.MergedFactorStorage() == "single" and np.array_equal(apply(Px, B, dev), x_method)
    for bad in ("half", 32, ""):
        wrong = params(LAPLACE)
        wrong["Preconditioner"]["MI Merged Factor Storage"] = bad
        try:
            hymls_amd.Preconditioner(A, wrong, testVector=tv, lib=lib)
            raise AssertionError("unknown storage %r accepted" % (bad,))
        except hymls_amd.HymlsError as e:
            assert e.code == -2, e


def check_solver(lib, dev):
    """Stokes-C 32^3 three-level, right-preconditioned GMRES(100) to 1e-8 through hymls_amd.Solver and the native solver,
    merged storage double and single.  The true residual ||b - K x|| / ||b||, formed in FP64 on the host, is below the
    tolerance in both storages, and the iteration counts are the ones measured on the simulator (ITERATIONS)."""
    import torch
    A, tv = problem(STOKES[0], STOKES[1])
    prm = params(STOKES)
    b = A @ np.random.default_rng(11).uniform(-1, 1, A.shape[0])
    res = {}
    for storage in ("double", "single"):
        P = make(A, tv, prm, lib, merged=storage)
        assert P.apply_bytes(10) > 0
        for name, S in (("python", hymls_amd.Solver(P, P, {"Solver": GMRES})), ("native", hymls_amd.NativeSolver(P, {"Solver": GMRES}))):
            x = S.ApplyInverse(torch.from_numpy(b).to(dev)).cpu().numpy()
            rr = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
            res[(name, storage)] = (S.getNumIter(), rr)
            print("merged f32 solver Stokes-C 32^3 merged storage %s, %s solver: %d iterations, true residual %.3e"
                  % (storage, name, S.getNumIter(), rr), flush=True)
    for key, (it, rr) in res.items():
        assert rr < TOL, res
        assert it == ITERATIONS[key], res
    return {"%s_%s" % k: v for k, v in res.items()}


@all_no_fused
def check_overflow(lib, dev):
    """the overflow case of f32_cases.check_overflow forced onto the merged route: three interior unknowns of a Laplace 8^3
    matrix scaled by 1e-20, the inverted pivot block holds entries of order 1e39.  FP64 storage computes and applies it;
    FP32 merged storage refuses in Compute with -4 and a message that names it, and the handle recovers in FP64 storage."""
    import scipy.sparse as sp
    A, tv = problem("Laplace", 8)
    prm = xml_params("Laplace", 8, 4, 1)
    P0 = hymls_amd.Preconditioner(A, prm, testVector=tv, lib=lib)
    P0.Initialize()
    d = np.ones(A.shape[0])
    d[P0.interior(0, 0)[:3]] = 1e-20
    As = (sp.diags(d) @ A @ sp.diags(d)).tocsr()
    P64 = make(As, tv, prm, lib, merged="double", no_fused=True)
    assert P64.apply_bytes(10) > 0
    x = apply(P64, np.ones(A.shape[0]), dev)
    assert np.isfinite(x).all() and np.abs(x).max() > 3.5e38        # (beyond FLT_MAX: the entries that do not fit)
    P32 = hymls_amd.Preconditioner(As, prm, testVector=tv, lib=lib)
    P32.SetMergedFactorStorage("single")
    try:
        P32.Compute()
        raise AssertionError("Compute with FP32 merged storage accepted panel entries beyond FLT_MAX")
    except hymls_amd.HymlsError as e:
        assert e.code == -4 and "FP32 merged factor storage" in str(e), e
    assert not P32.IsComputed()
    P32.SetMergedFactorStorage("double")        # the handle recovers in FP64 storage
    P32.Compute()
    assert np.array_equal(apply(P32, np.ones(A.shape[0]), dev), x)
    assert P32.apply_bytes(9) == P64.apply_bytes(9)


def worst(figures):
    return max(max(v) for v in figures.values()) if figures else math.nan
