"""Cases, ctypes driver and checks of the level-solve lab (tests/lvllab/lvl_harness.cpp): the merged level solve
(k_lvl_fwd / k_lvl_bwd, MergedSolve) of one pattern class on FP64 panels, on float-rounded FP64 panels and on the FP32
slab.  Shared by tests/test_lvllab.py (simulator) and tests/test_lvllab_gpu.py (product library, through
tests/lvllab/child.py).

Cases: LVL_CASES of tests/solve_tails_cases.py (imported, not copied: whole-front arrows a1..a9, dense_w8, the 64-row tile
tasks dense_w257..263, arrow_21_top241|243|247 with ri % 4 != 0), nrhs = 7 so that one solve runs the <4>, <2> and <1>
instantiations, plus dense_w2100: one front whose forward tile tasks need 2420 doubles of LDS per column, 77 KiB at
NV = 4, which is above the 64 KiB a kernel gets without hipFuncSetAttribute.

Checks.
  bitwise      the _f32 launchers on the demoted slab equal the FP64 launchers on the round_panels slab for nv in
               {1, 2, 3, 4, 7} and with ld = n + 5; demote_panels / round_panels equal astype(float32)
  column groups  a column of an _mv solve equals the single-vector solve of that column, also with
               HYMLS_MI_MV_GROUP_LVL = 1 and 2
  bound        |x - ref| <= c eps M per entry, ref the per-front sweeps in np.longdouble from the float32-rounded slab:
               panel_solve / panel_bound of tests/fusedlab/cases.py, imported (c = 2 x the longest chain of summands, M the
               same recurrence on absolute values)
  sharpness    1e-9 max|x| added to one entry fails the bound"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import solve_tails_cases as st  # noqa: E402

fc, fl = st.fc, st.fl
NRHS = st.LVL_NRHS
NV_LIST = (1, 2, 3, 4, 7)
PAD = 5
BIG = fl.Case("dense_w2100", "dense", (2100, 2), leaf=2100, merged=True, nrhs=NRHS)
CASES = list(st.LVL_CASES) + [BIG]
BY_NAME = {c.name: c for c in CASES}
CANARY = fc.CANARY


def build(which, out=None):
    """path of the harness library; sim: built (with its simulator library) in `out`"""
    if which == "gpu":
        subprocess.check_call(["make", "-s", "-C", HERE, "gpu"])
        return os.path.join(HERE, "liblvllab_gpu.so")
    out = out or os.path.join(HERE, "build")
    subprocess.check_call(["make", "-s", "-j8", "-C", HERE, "sim", "OUT=%s" % out])
    return os.path.join(out, "liblvllab_sim.so")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class HarnessError(RuntimeError):
    pass


class Lab:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        P, i32 = ctypes.c_void_p, ctypes.c_int32
        self.lib.lvllab_error.restype = ctypes.c_char_p
        self.lib.lvllab_plan_factor.argtypes = [i32, i32, P, P, P, P, i32, P, i32, i32, P, P, i32, P, i32, P, P]
        self.lib.lvllab_storage.argtypes = [P, P, P]
        self.lib.lvllab_solve.argtypes = [i32, i32, i32, P, P, P]

    def _check(self, rc):
        if rc != 0:
            raise HarnessError("lvllab: %d %s" % (rc, self.lib.lvllab_error().decode()))

    def plan_factor(self, case):
        """tables of the class (the layout of fusedlab's tables_of), the unpacked FP64 slab [nb][fs], flag bits"""
        pat = case.pattern()
        nb, nI, nS = case.nb, pat.nI, pat.nS
        vals = [case.values(pat, b) for b in range(nb)]
        kval = np.ascontiguousarray(np.concatenate([V[pat.rows, pat.cols] for V in vals]))
        info = np.zeros(8, dtype=np.int64)
        args = (nI, nS, _p(pat.rowptr), _p(pat.col), _p(pat.zero_diag), _p(pat.coord), nb, _p(kval), case.leaf, case.max_width)
        self._check(self.lib.lvllab_plan_factor(*args, None, None, 0, None, 0, None, _p(info)))
        nf, fs, nidx = int(info[0]), int(info[1]), int(info[3])
        assert info[7] == 1, "%s: merged_solve_fits is false" % case.name
        slab = np.zeros((nb, fs))
        fronts = np.zeros((nf, 10), dtype=np.int64)
        fidx = np.zeros(max(nidx, 1), dtype=np.int32)
        perm = np.zeros(nI, dtype=np.int32)
        self._check(self.lib.lvllab_plan_factor(*args, _p(slab), _p(fronts), nf, _p(fidx), len(fidx), _p(perm), _p(info)))
        T = {"nI": nI, "nb": nb, "fs": fs, "fronts": fronts, "fidx": fidx[:nidx], "perm": perm,
             "tasks": (int(info[4]), int(info[5])), "lds": int(info[6])}
        return T, slab, int(info[2])

    def storage(self, T):
        slab32 = np.zeros((T["nb"], T["fs"]), dtype=np.float32)
        rounded = np.zeros((T["nb"], T["fs"]))
        info = np.zeros(2, dtype=np.int64)
        self._check(self.lib.lvllab_storage(_p(slab32), _p(rounded), _p(info)))
        return slab32, rounded, info.tolist()

    def solve(self, T, storage, rhs, pad=0):
        """rhs [nv][nb * nI] in elimination order; the vectors as they come back [nv][ld] and the two guard marks"""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        nv, n = rhs.shape
        assert n == T["nb"] * T["nI"]
        x = np.zeros((nv, n + pad))
        info = np.zeros(2, dtype=np.int64)
        self._check(self.lib.lvllab_solve(storage, nv, pad, _p(rhs), _p(x), _p(info)))
        return x, info.tolist()


_labs = {}


def load(which, out=None):
    if which not in _labs:
        _labs[which] = Lab(build(which, out))
    return _labs[which]


FP64, FP32, ROUNDED = 0, 1, 2


def run_case(lab, case, groups=(None,)):
    """Every solve of a case.  groups: values of HYMLS_MI_MV_GROUP_LVL for the _mv solves (None: unset)."""
    assert "HYMLS_MI_MV_GROUP_LVL" not in os.environ
    T, slab, flag = lab.plan_factor(case)
    slab32, rounded, sflags = lab.storage(T)
    n = T["nb"] * T["nI"]
    pat = case.pattern()
    # [nrhs][nb * nI] in elimination order
    rhs = np.concatenate([case.rhs(pat, b)[:, T["perm"]] for b in range(case.nb)], axis=1)
    R = {"T": T, "slab": slab, "slab32": slab32, "rounded": rounded, "flag": flag, "storage_flags": sflags, "rhs": rhs,
         "guards": [], "n": n}

    def solve(key, storage, cols, pad=0):
        x, g = lab.solve(T, storage, rhs[cols], pad)
        R[key] = x
        R["guards"].append((key, g))

    for v in range(NRHS):                                   # single-vector solves: the NV = 1 launch of every column
        solve("x32_col%d" % v, FP32, [v])
        solve("xr_col%d" % v, ROUNDED, [v])
    solve("x64", FP64, list(range(NRHS)))
    for grp in groups:
        tag = "" if grp is None else "_g%d" % grp
        if grp is not None:
            os.environ["HYMLS_MI_MV_GROUP_LVL"] = str(grp)
        try:
            for nv in NV_LIST:
                solve("x32_nv%d%s" % (nv, tag), FP32, list(range(nv)))
                solve("xr_nv%d%s" % (nv, tag), ROUNDED, list(range(nv)))
            solve("x32_ld%s" % tag, FP32, list(range(NRHS)), PAD)
            solve("xr_ld%s" % tag, ROUNDED, list(range(NRHS)), PAD)
        finally:
            os.environ.pop("HYMLS_MI_MV_GROUP_LVL", None)
    R["groups"] = list(groups)
    return R


def exact_failures(case, R):
    """Everything that must hold bit for bit, the canaries and the flags (messages; empty: all hold)."""
    bad = []
    n = R["n"]

    def same(what, a, b):
        if not fc.same_bits(a, b):
            bad.append("%s: %s" % (case.name, what))

    if R["flag"] or any(R["storage_flags"]):
        bad.append("%s: flag bits %d after the factorisation, %s after demote / round" % (case.name, R["flag"], R["storage_flags"]))
    for key, g in R["guards"]:
        if g != [1, 1]:
            bad.append("%s: %s: guard tail or pad of x / y written %s" % (case.name, key, g))
    if not np.isfinite(R["slab"]).all():
        bad.append("%s: non-finite panel entry" % case.name)
    same("demote_panels differs from astype(float32)", R["slab32"], fc.round_f32(R["slab"]))
    same("round_panels differs from astype(float32)", R["rounded"], fc.round_f32(R["slab"]).astype(np.float64))
    singles32 = np.concatenate([R["x32_col%d" % v] for v in range(NRHS)])
    singlesr = np.concatenate([R["xr_col%d" % v] for v in range(NRHS)])
    if not np.isfinite(singles32).all():
        bad.append("%s: non-finite or unwritten solution entry" % case.name)
    same("single-vector _f32 solves differ from the FP64 launchers on the rounded slab", singles32, singlesr)
    if fc.same_bits(singles32, R["x64"]):
        bad.append("%s: the FP32 solve equals the FP64 solve bit for bit: the float slab was not read" % case.name)
    for grp in R["groups"]:
        tag = "" if grp is None else "_g%d" % grp
        for nv in NV_LIST:
            x32, xr = R["x32_nv%d%s" % (nv, tag)], R["xr_nv%d%s" % (nv, tag)]
            same("_mv_f32 nv = %d%s differs from the FP64 launchers on the rounded slab" % (nv, tag), x32, xr)
            same("_mv_f32 nv = %d%s: a column differs from its single-vector solve" % (nv, tag), x32, singles32[:nv])
        x32, xr = R["x32_ld%s" % tag], R["xr_ld%s" % tag]
        same("_mv_f32 with ld = n + %d%s differs from the rounded slab" % (PAD, tag), x32, xr)
        same("_mv_f32 with ld = n + %d%s differs from single solves" % (PAD, tag), x32[:, :n], singles32)
        if not fc.is_canary(x32[:, n:]).all() or not fc.is_canary(xr[:, n:]).all():
            bad.append("%s: pad behind a column written (ld = n + %d%s)" % (case.name, PAD, tag))
    return bad


_ref_cache = {}


def reference(case, R, b, v):
    """(longdouble sweeps from the float32-rounded slab, bound) of member b, column v; computed once and left unchanged"""
    key = (case.name, b, v)
    slab = fc.round_f32(R["slab"][b]).astype(np.float64)
    nI = R["T"]["nI"]
    rhs = R["rhs"][v, b * nI: (b + 1) * nI]
    hit = _ref_cache.get(key)
    if hit is None or not (fc.same_bits(hit[0], slab) and fc.same_bits(hit[1], rhs)):
        hit = (slab, rhs.copy(), fc.panel_solve(R["T"], slab, rhs, np.longdouble), fc.panel_bound(R["T"], slab, rhs))
        _ref_cache[key] = hit
    return hit[2], hit[3]


def bound_ratio(case, R, x_of=None, columns=(0, NRHS - 1)):
    """largest |x - ref| / bound over the entries of every member for the FP32 single-vector solves of `columns`"""
    worst, nI = 0.0, R["T"]["nI"]
    for v in columns:
        for b in range(case.nb):
            ref, bound = reference(case, R, b, v)
            x = R["x32_col%d" % v][0, b * nI: (b + 1) * nI]
            if x_of is not None:
                x = x_of(x)
            err = np.abs((x.astype(np.longdouble) - ref).astype(np.float64))
            worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))))
    return worst


def perturbed(x):
    """the mutant of the sharpness check: 1e-9 max|x| on the entry of largest magnitude's neighbour"""
    y = x.copy()
    y[len(y) // 2] += 1e-9 * np.abs(x).max()
    return y


def bound_failures(case, R):
    bad = []
    r = bound_ratio(case, R)
    rm = bound_ratio(case, R, perturbed, columns=(0,))
    print("lvllab %-24s |x32 - ref| / bound = %.3f, with 1e-9 max|x| on one entry %.3g" % (case.name, r, rm), flush=True)
    if not r <= 1.0:
        bad.append("%s: FP32 level solve outside the bound of the longdouble sweeps: ratio %.3f" % (case.name, r))
    if not rm > 1.0:
        bad.append("%s: the bound does not see a perturbation of 1e-9 max|x|: ratio %.3g" % (case.name, rm))
    return bad


def task_kinds(R):
    """{'whole', 'tile'} as MergedSolve::build cuts the fronts of the class"""
    return {"whole" if w + ri <= fl.LVL_SMALL_ROWS else "tile" for w, ri in R["T"]["fronts"][:, :2]}
