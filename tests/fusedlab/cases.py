"""Kernel lab of the fused interior solve and its panel layouts (tests/fusedlab/fused_harness.cpp).

Patterns and member values come from tests/frontlab/cases.py (dense block, arrowhead, grid box, saddle point).  This file
holds the ctypes driver of the harness, the case list, the numpy references written for the lab (nothing of them is taken
from the simulator or a kernel), the error bound of the panel sweeps and the coverage tags.  Shared by
tests/test_fusedlab.py (host simulator) and tests/test_fusedlab_gpu.py (product library, through child.py).

The reference of a solve is built from the panels the device produced (the unpacked FP64 slab, which tests/frontlab checks
against LAPACK): the multifrontal sweeps restated per front in np.longdouble from the front table and the index lists alone
-- a child's contribution goes to the row of the parent that has the same elimination position, so the assembly lists, the
contribution offsets and the level tables of the plan are not used and are thereby checked.  The bound per entry is
c eps M_i: M is the same recurrence on absolute values with every subtraction turned into an addition, c is twice the longest
chain of summands that feeds one entry (counted per case by the same recurrence on integers).  Every summand of a sum of n
terms passes through at most n roundings whatever the order, so an entry fed by a chain of L summands carries at most
((1 + u)^L - 1) M_i, u = eps / 2: to first order L u M_i, a quarter of the bound.  No constant is tuned."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"sim": os.path.join(HERE, "libfusedlab_sim.so"), "gpu": os.path.join(HERE, "libfusedlab_gpu.so")}


def _frontlab():
    key = "frontlab_cases"
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(HERE, "..", "frontlab", "cases.py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


fl = _frontlab()

EPS = 2.0 ** -52
CANARY = np.uint64(0x7ff4dead5eed5eed)
CANARY32 = np.uint32(0x7fa5eed5)
FLT_MAX = float(np.finfo(np.float32).max)
ERRORS = {"arg": -10, "perm": -11, "a_col": -12, "a_row": -13, "xoff": -14, "fits": -15}
GAP = 3                       # canary entries between the members' blocks of the level vector
NV_LIST = (2, 3, 4, 5, 7)
# limits of the launchers the GPU-only tags mirror (device_hip.hip: LDS_LIMIT_BYTES; device.hpp: NV_MAX)
LDS_LIMIT_BYTES = 160 * 1024
NV_MAX = 4


# ------------------------------------------------------------------ the harness
def build(which):
    subprocess.check_call(["make", "-s", "-C", HERE, which])
    return LIBS[which]


class HarnessError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "fusedlab: error %d: %s" % (code, msg))
        self.code = code


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Lab:
    """The exported entries of the harness."""

    def __init__(self, which):
        self.which = which
        self.lib = ctypes.CDLL(build(which))
        self.lib.fusedlab_error.restype = ctypes.c_char_p
        P, I, L = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        sig = {"fusedlab_reset": [],
               "fusedlab_plan": [I, I, P, P, P, P, I, P, I, I, I, P],
               "fusedlab_tables": [I, P, P, P, P, P, P],
               "fusedlab_factor": [I, P, P, P],
               "fusedlab_repack": [I, I, I, P, P],
               "fusedlab_set_slab": [I, P, I],
               "fusedlab_storage": [I, I, P, P],
               "fusedlab_solve": [I, I, P, P, P, I, L, I, L, P, P],
               "fusedlab_solve_io": [I, P, P, P, I, I, P, P, P, P, L, I, P, P, P, I, L, P, P, P, P, P, P],
               "fusedlab_demote": [I, L, I, I, P, P, P, P],
               "fusedlab_transposed": [I, L, P, P]}
        for name, args in sig.items():
            f = getattr(self.lib, name)
            f.argtypes, f.restype = args, ctypes.c_int

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc < 0:
            raise HarnessError(rc, self.lib.fusedlab_error().decode())
        return rc

    def reset(self):
        self._call("fusedlab_reset")

    def plan(self, pat, xoff, leaf, max_width, packed):
        """analyse_class + BatchedLU::upload; returns the tables of the class."""
        info = np.zeros(12, dtype=np.int64)
        xoff = _i32(xoff)
        cid = self._call("fusedlab_plan", pat.nI, pat.nS, _p(pat.rowptr), _p(pat.col), _p(pat.zero_diag), _p(pat.coord),
                         len(xoff), _p(xoff), leaf, max_width, int(packed), _p(info))
        nf, nlev, fs, cs, mlr, need, need_fronts, fits, nfw, nbw, nfidx, scratch = (int(v) for v in info)
        T = {"id": cid, "nI": pat.nI, "nb": len(xoff), "xoff": xoff, "nf": nf, "nlev": nlev, "fs": fs, "contrib_size": cs,
             "max_level_rows": mlr, "need": need, "need_fronts": need_fronts, "fits": bool(fits), "packed": bool(packed)}
        fronts = np.zeros((nf, 10), dtype=np.int64)
        T["fidx"] = np.zeros(nfidx, dtype=np.int32)
        T["fw_ptr"], T["bw_ptr"] = np.zeros(nlev + 1, dtype=np.int32), np.zeros(nlev + 1, dtype=np.int32)
        T["rec_n"] = np.zeros(nfw, dtype=np.int32)
        T["perm"] = np.zeros(pat.nI, dtype=np.int32)
        self._call("fusedlab_tables", cid, _p(fronts), _p(T["fidx"]), _p(T["fw_ptr"]), _p(T["bw_ptr"]), _p(T["rec_n"]), _p(T["perm"]))
        T["fronts"] = fronts
        return T

    def factor(self, T, kval):
        slab = np.zeros((T["nb"], T["fs"]))
        info = np.zeros(2, dtype=np.int64)
        self._call("fusedlab_factor", T["id"], _p(_f64(kval)), _p(slab), _p(info))
        return slab, int(info[0]), bool(info[1])

    def repack(self, T, b0, nbc):
        slab = np.zeros((T["nb"], T["fs"]))
        info = np.zeros(1, dtype=np.int64)
        self._call("fusedlab_repack", T["id"], b0, nbc, _p(slab), _p(info))
        return slab, bool(info[0])

    def set_slab(self, T, slab, packed):
        self._call("fusedlab_set_slab", T["id"], _p(_f64(slab)), int(packed))

    def storage(self, T, what):
        out = np.zeros((T["nb"], T["fs"]), dtype=np.float32 if what == 1 else np.float64)
        info = np.zeros(2, dtype=np.int64)
        self._call("fusedlab_storage", T["id"], what, _p(out), _p(info))
        return out, int(info[0]), bool(info[1])

    def solve(self, kind, subs, x, n, storage=0):
        """subs: [(class id, member, xoff)]; x [nv][ldx] (a copy is solved in place).  Returns (x, guard intact, LDS)."""
        x = _f64(np.atleast_2d(x)).copy()
        nv, ldx = x.shape
        sc, sm, so = (_i32([s[k] for s in subs]) for k in range(3))
        info = np.zeros(4, dtype=np.int64)
        self._call("fusedlab_solve", kind, len(subs), _p(sc), _p(sm), _p(so), storage, n, nv, ldx, _p(x), _p(info))
        return x, bool(info[0]), tuple(int(v) for v in info[1:])

    def solve_io(self, subs, n, nuser, perm, a_row, a_col, a_val, x2, z, b, a_lanes, nnz_hint):
        sc, sm, so = (_i32([s[k] for s in subs]) for k in range(3))
        perm, a_row, a_col = _i32(perm), _i32(a_row), _i32(a_col)
        a_val, x2, z, b = _f64(a_val), _f64(x2), _f64(z), _f64(b)
        out = {"x10_fused": np.zeros(n), "x10_sep": np.zeros(n), "user_fused": np.zeros(nuser), "user_sep": np.zeros(nuser),
               "t1_after": np.zeros(n)}
        info = np.zeros(3, dtype=np.int64)
        self._call("fusedlab_solve_io", len(subs), _p(sc), _p(sm), _p(so), n, nuser, _p(perm), _p(a_row), _p(a_col), _p(a_val),
                   len(a_col), len(x2), _p(x2), _p(z), _p(b), a_lanes, nnz_hint, _p(out["x10_fused"]), _p(out["x10_sep"]),
                   _p(out["user_fused"]), _p(out["user_sep"]), _p(out["t1_after"]), _p(info))
        out["guards"] = info.copy()
        return out

    def demote(self, what, src, src_off, dst_off):
        """Returns (whole output buffer from the 16-byte boundary on: offset + n + 64 entries, flag)."""
        src = _f64(src)
        n = len(src)
        dst = np.zeros(dst_off + n + 64, dtype=np.float32)
        rnd = np.zeros(src_off + n + 64)
        info = np.zeros(1, dtype=np.int64)
        self._call("fusedlab_demote", what, n, src_off, dst_off, _p(src), _p(dst), _p(rnd), _p(info))
        return (dst if what == 1 else rnd), int(info[0])

    def transposed(self, T, x):
        x = _f64(x).copy()
        info = np.zeros(1, dtype=np.int64)
        self._call("fusedlab_transposed", T["id"], len(x), _p(x), _p(info))
        return x, bool(info[0])


_loaded = {}


def load(which):
    if which not in _loaded:
        _loaded[which] = Lab(which)
    return _loaded[which]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(u), b.view(u)))


def canary_vector(shape):
    return np.full(shape, CANARY, dtype=np.uint64).view(np.float64)


def is_canary(a):
    return np.ascontiguousarray(a).view(np.uint64) == CANARY


# ------------------------------------------------------------------ references (numpy, written for the lab)
def packed_index(w, ri):
    """Where entry t = i + (w + ri) k of the column-major (w + ri) x w panel goes (device.hpp: packed_lower / packed_l21 /
    packed_upper, restated): [strictly lower triangle by columns | L21 rows, ld = ri | upper triangle by columns]."""
    ld = w + ri
    i, k = np.meshgrid(np.arange(ld, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    lower = k * (2 * w - k - 1) // 2 + (i - k - 1)
    l21 = w * (w - 1) // 2 + (i - w) + ri * k
    upper = w * (w - 1) // 2 + ri * w + k * (k + 1) // 2 + i
    dst = np.where(i >= w, l21, np.where(i > k, lower, upper))
    return dst.T.reshape(-1)      # indexed by t = i + ld k


def repack_reference(T, slab, members, swap=None):
    """The slab with the L-side panels of `members` repacked; swap = (front, t0, t1): exchange two targets of that front's
    permutation (the mutant of the sharpness test)."""
    out = slab.copy()
    for s, (w, ri, rs, parent, level, c0, idx_off, lp_off, q_off, big) in enumerate(T["fronts"]):
        dst = packed_index(int(w), int(ri))
        if swap is not None and swap[0] == s:
            dst[swap[1]], dst[swap[2]] = dst[swap[2]], dst[swap[1]]
        n = (w + ri) * w
        for b in members:
            out[b, lp_off + dst] = slab[b, lp_off: lp_off + n]
    return out


def _tree(T):
    F = T["fronts"]
    kids = [[] for _ in range(len(F))]
    for s in range(len(F)):
        if F[s, 3] >= 0:
            kids[int(F[s, 3])].append(s)
    return F, kids


def _panels(T, slab, s, dtype):
    w, ri, rs, parent, level, c0, idx_off, lp_off, q_off, big = (int(v) for v in T["fronts"][s])
    L = slab[lp_off: lp_off + (w + ri) * w].reshape(w, w + ri).T.astype(dtype)
    Q = slab[q_off: q_off + w * ri].reshape(ri, w).T.astype(dtype)
    return w, ri, c0, T["fidx"][idx_off: idx_off + w + ri].astype(np.int64), np.tril(L[:w], -1), np.triu(L[:w]), L[w:], Q


def panel_solve(T, slab, b, dtype=np.longdouble, absolute=False, transposed=False, drop=None):
    """The sweeps of one member with the panels of its unpacked slab, b and the result in elimination order.
    Forward per front: assembly, x = f + L11inv_strict f, c = u - L21 f; backward: x = Uinv x - Q x[idx]
    (transposed: U^T then L^T).  absolute: the recurrence of the bound.  drop = (child front, row): that one assembly
    source is left out (the mutant of the sharpness test)."""
    F, kids = _tree(T)
    sgn = dtype(1) if absolute else dtype(-1)
    x = np.abs(b).astype(dtype) if absolute else b.astype(dtype)
    slab = np.abs(slab) if absolute else slab
    contrib = {}
    for s in range(len(F)):
        w, ri, c0, idx, Ls, U, PL, Q = _panels(T, slab, s, dtype)
        a = np.zeros(w + ri, dtype=dtype)
        a[:w] = x[c0: c0 + w]
        for c in kids[s]:
            pos, val = contrib.pop(c)
            loc = np.searchsorted(idx, pos)
            assert np.array_equal(idx[loc], pos), "a child's update row is missing in its parent"
            if drop is not None and drop[0] == c:
                val = val.copy()
                val[drop[1]] = 0
            a[loc] += val
        f = a[:w]
        if not transposed:
            x[c0: c0 + w] = f + Ls @ f
            contrib[s] = (idx[w:], a[w:] + sgn * (PL @ f))
        else:
            x[c0: c0 + w] = U.T @ f
            contrib[s] = (idx[w:], a[w:] + sgn * (Q.T @ f))
    assert not contrib or all(len(v[0]) == 0 for v in contrib.values())
    for s in range(len(F) - 1, -1, -1):
        w, ri, c0, idx, Ls, U, PL, Q = _panels(T, slab, s, dtype)
        xs = x[c0: c0 + w]
        if not transposed:
            x[c0: c0 + w] = U @ xs + sgn * (Q @ x[idx[w:]])
        else:
            x[c0: c0 + w] = xs + Ls.T @ xs + sgn * (PL.T @ x[idx[w:]])
    return x


def chain_length(T, transposed=False):
    """Longest chain of summands that feeds one entry of the result (see the module docstring): per sum, its number of
    terms plus the longest chain among its inputs."""
    F, kids = _tree(T)
    D = np.zeros(T["nI"], dtype=np.int64)
    contrib = {}
    for s in range(len(F)):
        w, ri, rs, parent, level, c0, idx_off = (int(v) for v in F[s, :7])
        idx = T["fidx"][idx_off: idx_off + w + ri].astype(np.int64)
        Da = np.zeros(w + ri, dtype=np.int64)
        Da[:w] = D[c0: c0 + w]
        nterm = np.zeros(w + ri, dtype=np.int64)
        nterm[:w] = 1
        for c in kids[s]:
            pos, Dc = contrib.pop(c)
            loc = np.searchsorted(idx, pos)
            Da[loc] = np.maximum(Da[loc], Dc)
            nterm[loc] += 1
        Da += nterm
        f = Da[:w]
        fmax = int(f.max())
        if not transposed:
            D[c0: c0 + w] = np.maximum.accumulate(f) + np.arange(1, w + 1)
        else:
            D[c0: c0 + w] = np.maximum.accumulate(f) + np.arange(1, w + 1)    # column i of U: i + 1 terms
        contrib[s] = (idx[w:], np.maximum(Da[w:], fmax) + w + 1)
    for s in range(len(F) - 1, -1, -1):
        w, ri, rs, parent, level, c0, idx_off = (int(v) for v in F[s, :7])
        idx = T["fidx"][idx_off: idx_off + w + ri].astype(np.int64)
        up = int(D[idx[w:]].max()) if ri else 0
        xs = D[c0: c0 + w]
        suffix = np.maximum.accumulate(xs[::-1])[::-1]
        D[c0: c0 + w] = np.maximum(suffix, up) + (w - np.arange(w)) + ri
    return int(D.max())


def panel_bound(T, slab, b, transposed=False):
    """c eps M per entry (elimination order) for one member."""
    M = panel_solve(T, slab, b, np.longdouble, absolute=True, transposed=transposed)
    return (2 * chain_length(T, transposed) * EPS * M).astype(np.float64)


def round_f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(np.float32)


# ------------------------------------------------------------------ the case list
class ClassSpec:
    """sep: separator rows kept of the frontlab pattern (None: all).  The whole shell of a grid box makes the Schur update
    of its root front heavy enough for the multi-workgroup path (Front::big), which fused_solve_fits excludes; the solve
    itself never reads the separator rows."""

    def __init__(self, kind, args, nb=1, leaf=24, max_width=256, packed=True, sep=None):
        self.kind, self.args, self.nb, self.leaf, self.max_width, self.packed, self.sep = kind, args, nb, leaf, max_width, packed, sep

    def pattern(self):
        pat = fl.PATTERNS[self.kind](*self.args)
        if self.sep is None or self.sep >= pat.nS:
            return pat
        n = pat.nI + self.sep
        cut = fl.Pattern(pat.nI, self.sep, pat.mask[:n, :n].copy(), pat.zero_diag, pat.coord.reshape(-1, 3))
        if hasattr(pat, "vp_sign"):
            cut.vp_sign = pat.vp_sign[:n, :n]
        return cut


class Case:
    """classes: the pattern classes of the launch.  steps (all on by default): 'mv' multi-vector solves, 'f32' FP32 panels,
    'io' FusedIO with a_lanes lanes, 'transposed'.  sim = False: product library only (too slow for the simulator suite)."""

    def __init__(self, name, classes, a_lanes=4, steps=("mv", "f32", "io", "transposed"), sim=True):
        self.name, self.classes, self.a_lanes, self.steps, self.sim = name, classes, a_lanes, steps, sim

    def __repr__(self):
        return self.name


def _one(name, kind, args, **kw):
    ckw = {k: kw.pop(k) for k in ("nb", "leaf", "max_width", "packed", "sep") if k in kw}
    return Case(name, [ClassSpec(kind, args, **ckw)], **kw)


CASES = [
    # one dense front: the three level widths of both sweeps at their edges, every k tail, w = 1, nlev = 1
    _one("dense_w1", "dense", (1, 2), leaf=1, nb=2, a_lanes=1),
    _one("dense_w7", "dense", (7, 3), leaf=7, nb=3, a_lanes=2, packed=False),
    _one("dense_w64", "dense", (64, 4), leaf=64, nb=2, a_lanes=8),
    _one("dense_w65", "dense", (65, 0), leaf=65, nb=2),
    _one("dense_w128", "dense", (128, 3), leaf=128, a_lanes=1),
    _one("dense_w129", "dense", (129, 5), leaf=129, nb=2, packed=False),
    _one("dense_w203", "dense", (203, 2), leaf=203, a_lanes=2),
    # trees: assembly rows with 1 .. 5 inline sources and with the list route, ri % 4 != 0, update rows
    _one("arrow_2x5_top3", "arrow", (2, 5, 3, 2), leaf=5, nb=3, a_lanes=1),
    _one("arrow_3x9_top6", "arrow", (3, 9, 6, 3), leaf=9, nb=2, a_lanes=2),
    _one("arrow_4x16_top21", "arrow", (4, 16, 21, 4), leaf=16, nb=2, a_lanes=8),
    _one("arrow_5x24_top30", "arrow", (5, 24, 30, 4), leaf=24, nb=2),
    _one("arrow_7x24_top37", "arrow", (7, 24, 37, 6), leaf=24, nb=3, packed=False),
    _one("grid7_8", "grid", (8, 8, 8, 7), nb=3, a_lanes=2),
    _one("grid27_6", "grid", (6, 6, 6, 27), leaf=32, nb=2, a_lanes=8),
    _one("saddle_4", "saddle", (4, 16), nb=2),
    # many small fronts: more than 256 fronts, a first level of more than 384 pivot rows (the descriptor table moves)
    _one("grid7_12_leaf4", "grid", (12, 12, 12, 7), leaf=4, nb=2, sep=48, steps=("mv", "io")),
    # LDS above 64 KiB for one vector; four columns no longer fit 160 KiB (groups of 2), then two do not either (1)
    _one("grid7_14", "grid", (14, 14, 14, 7), leaf=32, nb=2, sep=48, steps=("mv", "f32")),
    _one("grid7_15", "grid", (15, 15, 15, 7), leaf=32, nb=1, sep=48, steps=("mv",)),
    # two classes of very different size in one launch: the small one runs with the LDS of the large one
    Case("two_dense40_grid12", [ClassSpec("dense", (40, 3), nb=2, leaf=40),
                                ClassSpec("grid", (12, 12, 12, 7), nb=1, leaf=24, sep=48)], steps=("mv", "io")),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def class_values(case, ci, pat, b):
    return fl.member_values(pat, fl.seed_of("%s/%d" % (case.name, ci), b))


def rng_of(case, what):
    return np.random.default_rng(fl.seed_of(case.name + "/" + what, 0))


# ------------------------------------------------------------------ running a case
def run_case(lab, case):
    """Every step of the case through the harness.  Returns a flat dict of arrays (child.py stores it as .npz)."""
    lab.reset()
    R = {}
    pats = [c.pattern() for c in case.classes]
    # layout of the level vector: the members' blocks one after the other, GAP canary entries between and behind them
    xoffs, off = [], 0
    for c, pat in zip(case.classes, pats):
        xoffs.append([off + b * (pat.nI + GAP) for b in range(c.nb)])
        off += c.nb * (pat.nI + GAP)
    n = off
    tabs = [lab.plan(pat, xo, c.leaf, c.max_width, c.packed) for c, pat, xo in zip(case.classes, pats, xoffs)]
    subs, inside = [], np.zeros(n, dtype=bool)
    for ci, T in enumerate(tabs):
        for key in ("fronts", "fidx", "fw_ptr", "bw_ptr", "rec_n", "perm"):
            R["c%d_%s" % (ci, key)] = T[key]
        R["c%d_scalars" % ci] = np.array([T[k] for k in ("nI", "nb", "nf", "nlev", "fs", "contrib_size", "max_level_rows", "need",
                                                         "need_fronts", "fits", "packed")], dtype=np.int64)
        R["c%d_xoff" % ci] = T["xoff"]
        for b, o in enumerate(T["xoff"]):
            subs.append((T["id"], b, int(o)))
            inside[o: o + T["nI"]] = True
    R["n"] = np.array(n)
    # ---- factor (unpacked panels), then repack_fronts alone
    flags = []
    for ci, (c, pat, T) in enumerate(zip(case.classes, pats, tabs)):
        kval = np.concatenate([class_values(case, ci, pat, b)[pat.rows, pat.cols] for b in range(c.nb)])
        U, flag, guard = lab.factor(T, kval)
        flags += [flag, int(not guard)]
        R["c%d_slab" % ci] = U
        # member 1 alone first (the others must not change), then the rest; every call returns the whole slab
        todo = [(1, 1), (0, 1)] + ([(2, c.nb - 2)] if c.nb > 2 else []) if c.nb > 1 else [(0, 1)]
        for q, (b0, nbc) in enumerate(todo):
            P, guard = lab.repack(T, b0, nbc)
            flags.append(int(not guard))
            if q == 0:
                R["c%d_repack_first" % ci] = P
        R["c%d_repacked" % ci] = P
    R["flags"] = np.array(flags, dtype=np.int64)     # [factor flag, guards written ...]: all zero when all is well
    _run_solves(lab, case, pats, tabs, subs, inside, n, R)
    lab.reset()
    return R


def _layout(lab, tabs, R, packed):
    """Slab and layout flag of every class: its repacked slab, or the unpacked one."""
    for ci, T in enumerate(tabs):
        lab.set_slab(T, R["c%d_repacked" % ci] if packed[ci] else R["c%d_slab" % ci], packed[ci])


def _run_solves(lab, case, pats, tabs, subs, inside, n, R):
    nvmax = max(NV_LIST)
    rng = rng_of(case, "rhs")
    B = canary_vector((nvmax, n))
    B[:, inside] = rng.uniform(-1.0, 1.0, (nvmax, int(inside.sum())))
    R["rhs"] = B
    guards = []

    def solve(kind, sub, x, storage=0):
        y, guard, lds = lab.solve(kind, sub, x, n, storage)
        guards.append(int(not guard))
        R["lds"] = np.array(lds, dtype=np.int64)
        return y

    def singles(kind, storage=0):
        return np.stack([solve(kind, subs, B[v], storage)[0] for v in range(nvmax)])

    # ---- packed against unpacked panels (only the addresses differ), then the layout the case asks for
    _layout(lab, tabs, R, [False] * len(tabs))
    R["x_unpacked"] = solve(0, subs, B[0])[0]
    _layout(lab, tabs, R, [True] * len(tabs))
    R["x_packed"] = solve(0, subs, B[0])[0]
    _layout(lab, tabs, R, [c.packed for c in case.classes])
    R["x_single"] = singles(0)
    # ---- a member alone, a class alone (the launch then has the LDS of that class only)
    R["x_member_alone"] = solve(0, [subs[-1]], B[0])[0]
    R["x_class_alone"] = solve(0, [s for s in subs if s[0] == tabs[0]["id"]], B[0])[0]
    if "mv" in case.steps:
        for nv in NV_LIST:
            R["x_mv%d" % nv] = solve(2, subs, B[:nv])
        for nv in (4, 7):     # ldx = n + 5: the 5 entries behind every column hold the canary
            Bl = canary_vector((nv, n + 5))
            Bl[:, :n] = B[:nv]
            R["x_mv%d_ld" % nv] = lab.solve(2, subs, Bl, n)[0]
    if "f32" in case.steps:
        f32_flags = []
        for ci, T in enumerate(tabs):
            R["c%d_slab32" % ci], fl32, g = lab.storage(T, 1)
            f32_flags += [fl32, int(not g)]
            R["c%d_rounded" % ci], fl32, g = lab.storage(T, 2)
            f32_flags += [fl32, int(not g)]
        R["f32_flags"] = np.array(f32_flags, dtype=np.int64)
        R["x_f32"] = singles(1)
        R["x_rounded"] = singles(0, storage=2)
        if "mv" in case.steps:
            R["x_mv3_f32"] = solve(3, subs, B[:3])
            R["x_mv3_rounded"] = solve(2, subs, B[:3], storage=2)
    if "io" in case.steps:
        for k, v in io_run(lab, case, subs, tabs).items():
            R["io_" + k] = v
    if "transposed" in case.steps:
        xt = B[0].copy()
        for T in tabs:
            xt, guard = lab.transposed(T, xt)
            guards.append(int(not guard))
        R["x_transposed"] = xt
    R["guards"] = np.array(guards, dtype=np.int64)


def io_inputs(case, n):
    """perm: a random injection into a user vector of n + 7 entries; A: rows of 0 .. 2 a_lanes + 1 entries, every fifth
    row empty; nnz_hint: an entry count for which spmv() shares a row among a_lanes lanes (device.hpp: spmv_lanes)."""
    rng = rng_of(case, "io")
    nuser, nx2 = n + 7, 37
    perm = rng.permutation(nuser)[:n].astype(np.int32)
    length = rng.integers(0, 2 * case.a_lanes + 2, n)
    length[::5] = 0
    a_row = np.concatenate([[0], np.cumsum(length)]).astype(np.int32)
    nnz = int(a_row[-1])
    return {"nuser": nuser, "perm": perm, "a_row": a_row, "a_col": rng.integers(0, nx2, nnz).astype(np.int32),
            "a_val": rng.uniform(-1.0, 1.0, nnz), "x2": rng.uniform(-1.0, 1.0, nx2), "z": rng.uniform(-1.0, 1.0, n),
            "b": rng.uniform(-1.0, 1.0, nuser), "hint": n * {1: 1, 2: 3, 4: 10, 8: 30}[case.a_lanes]}


def io_subs(subs, tabs):
    """The same members laid end to end: FusedIO needs every row of the level vector solved by the launch."""
    nI = {T["id"]: T["nI"] for T in tabs}
    out, off = [], 0
    for cid, b, _ in subs:
        out.append((cid, b, off))
        off += nI[cid]
    return out, off


def io_run(lab, case, subs, tabs):
    dense, nd = io_subs(subs, tabs)
    I = io_inputs(case, nd)
    out = lab.solve_io(dense, nd, I["nuser"], I["perm"], I["a_row"], I["a_col"], I["a_val"], I["x2"], I["z"], I["b"],
                       case.a_lanes, I["hint"])
    out["x10_plain"] = lab.solve(0, dense, I["b"][I["perm"]], nd)[0][0]     # the plain solve of the gathered vector
    return out


# ------------------------------------------------------------------ checks on the results of a case
def tables_of(R):
    """The class tables stored by run_case."""
    tabs, ci = [], 0
    while "c%d_fronts" % ci in R:
        sc = [int(v) for v in R["c%d_scalars" % ci]]
        T = dict(zip(("nI", "nb", "nf", "nlev", "fs", "contrib_size", "max_level_rows", "need", "need_fronts", "fits", "packed"), sc))
        for key in ("fronts", "fidx", "fw_ptr", "bw_ptr", "rec_n", "perm", "xoff"):
            T[key] = R["c%d_%s" % (ci, key)]
        T["id"] = ci
        tabs.append(T)
        ci += 1
    return tabs


def members_of(R):
    """[(class index, member, offset in the level vector)] in launch order."""
    return [(ci, b, int(o)) for ci, T in enumerate(tables_of(R)) for b, o in enumerate(T["xoff"])]


def exact_failures(case, R):
    """Everything that must hold bit for bit, the canaries and the flags (messages; empty: all hold)."""
    bad = []
    tabs = tables_of(R)
    n = int(R["n"])
    inside = np.zeros(n, dtype=bool)
    for ci, b, o in members_of(R):
        inside[o: o + tabs[ci]["nI"]] = True

    def same(what, a, b):
        if not same_bits(a, b):
            bad.append(what)

    def gaps(what, x):
        x = np.atleast_2d(x)
        if not is_canary(x[:, :n][:, ~inside]).all() or not is_canary(x[:, n:]).all():
            bad.append(what + ": an entry outside the members' blocks was written")
        if not np.isfinite(x[:, :n][:, inside]).all():
            bad.append(what + ": non-finite or unwritten solution entry")

    if R["flags"].any():
        bad.append("factorisation flag or a written guard tail: %s" % R["flags"].tolist())
    if R["guards"].any():
        bad.append("guard tail behind a solution vector written")
    for ci, T in enumerate(tabs):
        U = R["c%d_slab" % ci]
        if not np.isfinite(U).all():
            bad.append("class %d: non-finite or unwritten panel entry" % ci)
        first = [1] if T["nb"] > 1 else [0]
        same("class %d: repack of member %d alone differs from the permuted slab (or touches another member, a Q panel)" % (ci, first[0]),
             R["c%d_repack_first" % ci], repack_reference(T, U, first))
        same("class %d: repacked slab differs from the permuted slab" % ci, R["c%d_repacked" % ci], repack_reference(T, U, range(T["nb"])))
        if "c%d_slab32" % ci in R:
            cur = R["c%d_repacked" % ci] if T["packed"] else U
            same("class %d: demote_panels differs from astype(float32)" % ci, R["c%d_slab32" % ci], round_f32(cur))
            same("class %d: round_panels differs from astype(float32)" % ci, R["c%d_rounded" % ci], round_f32(cur).astype(np.float64))
    if "f32_flags" in R and R["f32_flags"].any():
        bad.append("FP32 range flag on finite panels or a written guard tail: %s" % R["f32_flags"].tolist())
    same("packed and unpacked panels give different solves", R["x_packed"], R["x_unpacked"])
    same("the class's own layout differs from the packed solve", R["x_single"][0], R["x_packed"])
    for key in ("x_unpacked", "x_packed", "x_single"):
        gaps(key, R[key])
    # a member alone / the first class alone: the same bits in its block, canary everywhere else
    for key, keep in (("x_member_alone", [members_of(R)[-1]]), ("x_class_alone", [m for m in members_of(R) if m[0] == 0])):
        want = canary_vector(n)
        for ci, b, o in keep:
            want[o: o + tabs[ci]["nI"]] = R["x_single"][0, o: o + tabs[ci]["nI"]]
        rest = R["rhs"][0].copy()     # the other members' right-hand sides stay as they were
        for ci, b, o in keep:
            rest[o: o + tabs[ci]["nI"]] = want[o: o + tabs[ci]["nI"]]
        same(key + ": differs from the same members inside the whole launch", R[key], rest)
    if "mv" in case.steps:
        for nv in NV_LIST:
            same("_mv with nv = %d differs from single solves" % nv, R["x_mv%d" % nv], R["x_single"][:nv])
        for nv in (4, 7):
            x = R["x_mv%d_ld" % nv]
            same("_mv with nv = %d, ldx = n + 5 differs from single solves" % nv, x[:, :n], R["x_single"][:nv])
            gaps("x_mv%d_ld" % nv, x)
    if "f32" in case.steps:
        same("_f32 on the demoted slab differs from the FP64 kernel on the rounded slab", R["x_f32"], R["x_rounded"])
        gaps("x_f32", R["x_f32"])
        if "mv" in case.steps:
            same("_mv_f32 differs from single _f32 solves", R["x_mv3_f32"], R["x_f32"][:3])
            same("_mv on the rounded slab differs from single solves", R["x_mv3_rounded"], R["x_rounded"][:3])
    if "io" in case.steps:
        if R["io_guards"].min() != 1:
            bad.append("FusedIO: guard tail written")
        same("FusedIO (1, 0) differs from gather + solve", R["io_x10_fused"], R["io_x10_sep"])
        same("gather + solve differs from the solve of the gathered vector", R["io_x10_sep"], R["io_x10_plain"])
        same("FusedIO (2, 1) differs from spmv + solve + axpby + scatter", R["io_user_fused"], R["io_user_sep"])
        if not is_canary(R["io_t1_after"]).all():
            bad.append("FusedIO (2, 1) wrote its x argument")
        nd = len(R["io_t1_after"])
        hit = np.zeros(len(R["io_user_fused"]), dtype=bool)
        hit[io_inputs(case, nd)["perm"]] = True
        if not is_canary(R["io_user_fused"][~hit]).all() or not np.isfinite(R["io_user_fused"][hit]).all():
            bad.append("FusedIO (2, 1): user entries outside perm written, or entries of perm not written")
    return bad


def member_problem(case, R, ci, b, transposed=False, f32=False):
    """(tables, unpacked slab of the member, right-hand side and device result in elimination order)."""
    T = tables_of(R)[ci]
    o = int(T["xoff"][b])
    slab = R["c%d_slab" % ci][b]
    if f32:
        slab = round_f32(slab).astype(np.float64)
    key = "x_transposed" if transposed else ("x_f32" if f32 else "x_single")
    x = R[key] if transposed else R[key][0]
    return T, slab, R["rhs"][0, o: o + T["nI"]], x[o: o + T["nI"]]


def panel_ratios(case, R, x_of=None, drop=None):
    """Largest |x - x_ref| / bound over the entries of every member, per kind of solve: {kind: ratio}.  x_of(kind, ci, b,
    x): the vector to judge instead of the device's (the float64 restatement, the mutants)."""
    out = {}
    kinds = [("fp64", False, False)] + ([("f32", False, True)] if "f32" in case.steps else []) + \
            ([("transposed", True, False)] if "transposed" in case.steps else [])
    for kind, tr, f32 in kinds:
        worst = 0.0
        for ci, b, o in members_of(R):
            T, slab, rhs, x = member_problem(case, R, ci, b, tr, f32)
            ref, bound = _reference(case, ci, b, kind, T, slab, rhs, tr, drop)
            if x_of is not None:
                x = x_of(kind, T, slab, rhs, x)
            err = np.abs((x.astype(np.longdouble) - ref).astype(np.float64))
            worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))))
        out[kind] = worst
    return out


_ref_cache = {}


def _reference(case, ci, b, kind, T, slab, rhs, tr, drop):
    """(reference, bound) of one member; computed once per slab (the variants of the GPU test share their panels bit for
    bit, and then share the reference, which is left unchanged)."""
    key = (case.name, ci, b, kind)
    hit = _ref_cache.get(key) if drop is None else None
    if hit is not None and same_bits(hit[0], slab) and same_bits(hit[1], rhs):
        return hit[2], hit[3]
    ref = panel_solve(T, slab, rhs, np.longdouble, transposed=tr, drop=drop)
    bound = panel_bound(T, slab, rhs, tr)
    if drop is None:
        _ref_cache[key] = (slab.copy(), rhs.copy(), ref, bound)
    return ref, bound


def float64_restatement(kind, T, slab, rhs, x):
    return panel_solve(T, slab, rhs, np.float64, transposed=(kind == "transposed"))


def end_to_end_failures(case, R):
    """A11 x = b (and A11^T x = b) against float64 LAPACK with frontlab's bound 8 nI eps cond(A11): shows that the panels
    mean what the reference assumes."""
    bad = []
    for ci, T in enumerate(tables_of(R)):
        pat = case.classes[ci].pattern()
        nI, perm = T["nI"], T["perm"]
        for b, o in list(enumerate(T["xoff"]))[: 1 if nI > 2000 else None]:     # (a condition number of order 3000 takes seconds)
            A11 = class_values(case, ci, pat, b)[:nI, :nI]
            kappa = np.linalg.cond(A11, 1)
            rhs = np.zeros(nI)
            rhs[perm] = R["rhs"][0, o: o + nI]
            for key, A in (("x_single", A11), ("x_transposed", A11.T)):
                if key not in R:
                    continue
                x = np.zeros(nI)
                x[perm] = (R[key][0] if key == "x_single" else R[key])[o: o + nI]
                xr = np.linalg.solve(A, rhs)
                fe = np.linalg.norm(x - xr) / np.linalg.norm(xr)
                if not fe <= fl.C_TOL * nI * EPS * kappa:
                    bad.append("class %d member %d %s: forward error %.3e > %.3e" % (ci, b, key, fe, fl.C_TOL * nI * EPS * kappa))
    return bad


# ------------------------------------------------------------------ coverage tags (from the tables of the plan entry)
def _width_tags(prefix, ni):
    t = set()
    if ni <= 64:
        t.add(prefix + "<=64")
    if ni in (64, 65, 128, 129):
        t.add(prefix + "=%d" % ni)
    if ni > 256:
        t.add(prefix + ">256")
    return t


def mv_groups(per, fixed, nv, cap=NV_MAX):
    """The column groups dev::interior_solve_fused_mv launches (device_hip.hip: fused_mv_groups), as (group, halved from)."""
    out, v = [], 0
    while v < nv:
        g0 = 4 if nv - v >= 4 else (2 if nv - v >= 2 else 1)
        g = g0
        while g > 1 and g > cap:
            g >>= 1
        fit = g
        while fit > 1 and (per * fit + fixed) * 8 > LDS_LIMIT_BYTES:
            fit >>= 1
        out.append((fit, g if fit < g else 0))
        v += fit
    return out


def coverage(results, gpu=False, mv_cap=NV_MAX):
    """Branches of the fused kernels reached by a set of runs: results = [(case, R)]."""
    got = set()
    for case, R in results:
        tabs = tables_of(R)
        if len(tabs) > 1:
            got.add("two_classes")
        need, fronts = max(T["need"] for T in tabs), max(T["need_fronts"] for T in tabs)
        per = max(T["need"] - T["need_fronts"] for T in tabs)
        if gpu:
            if need * 8 > 64 * 1024:
                got.add("lds>64KiB")
            if "mv" in case.steps:
                for nv in NV_LIST:
                    for g, halved in mv_groups(per, fronts, nv, mv_cap):
                        got.add("mv_group=%d" % g)
                        if halved:
                            got.add("mv_halved_to_%d" % g)
        for T in tabs:
            F = T["fronts"]
            got.add("packed" if T["packed"] else "unpacked")
            got.add("level_rows>384" if T["max_level_rows"] > 384 else "level_rows<384")
            if T["nI"] % 256:
                got.add("nI%256!=0")
            if T["nlev"] == 1:
                got.add("nlev=1")
            if T["nf"] > 256:
                got.add("nfronts>256")
            for n_src in set(T["rec_n"].tolist()):
                got.add("rec_list" if n_src == 0xffff else "rec_n=%d" % n_src)
            for w, ri in F[:, :2]:
                if w == 1:
                    got.add("w=1")
                got.add("ri=0" if ri == 0 else ("ri%4!=0" if ri % 4 else "ri%4=0"))
            lev = F[:, 4]
            for l in range(T["nlev"]):
                fw_ni = int(T["fw_ptr"][l + 1] - T["fw_ptr"][l])
                bw_ni = int(T["bw_ptr"][l + 1] - T["bw_ptr"][l])
                got |= _width_tags("fw_ni", fw_ni) | _width_tags("bw_ni", bw_ni)
                for w, ri in F[lev == l][:, :2]:
                    w, ri = int(w), int(ri)
                    # lengths of the k loops: forward kmax = min(r, w) per row r, backward w - i per pivot row i and ri
                    fw_len = set(min(r, w) for r in range(w + ri))
                    bw_len = set(range(1, w + 1)) | {ri}
                    for ni, lens in ((fw_ni, fw_len), (bw_ni, bw_len)):
                        for k in lens:
                            if ni <= 64:
                                got.add("ksplit4_tail" + ("=0" if k % 16 == 0 else "!=0"))
                            elif ni <= 128:
                                got.add("ksplit2_tail" + ("=0" if k % 8 == 0 else "!=0"))
                            else:
                                got.add("wide_tail%%4=%d" % (k % 4))
    return got


REQUIRED_SIM = ({"fw_ni<=64", "fw_ni=64", "fw_ni=65", "fw_ni=128", "fw_ni=129", "fw_ni>256",
                 "bw_ni<=64", "bw_ni=64", "bw_ni=65", "bw_ni=128", "bw_ni=129", "bw_ni>256",
                 "ksplit4_tail=0", "ksplit4_tail!=0", "ksplit2_tail=0", "ksplit2_tail!=0",
                 "wide_tail%4=0", "wide_tail%4=1", "wide_tail%4=2", "wide_tail%4=3",
                 "rec_n=0", "rec_n=1", "rec_n=2", "rec_n=3", "rec_n=4", "rec_n=5", "rec_list",
                 "w=1", "ri=0", "ri%4!=0", "nlev=1", "nfronts>256", "level_rows<384", "level_rows>384",
                 "packed", "unpacked", "two_classes", "nI%256!=0"})
GPU_ONLY = {"lds>64KiB", "mv_group=4", "mv_group=2", "mv_group=1", "mv_halved_to_2", "mv_halved_to_1"}
REQUIRED_GPU = REQUIRED_SIM | GPU_ONLY


# ------------------------------------------------------------------ demote_panels / round_panels on their own
DEMOTE_SIZES = (1, 3, 4, 5, 1023, 1024, 1025)


def demote_values(n):
    """Edge values first (FLT_MAX, the doubles next to it, the largest double that still rounds to FLT_MAX and the first
    that does not, subnormals of float, ties to even, signed zeros), then random ones; none of them NaN or infinite."""
    fmax = np.float64(np.finfo(np.float32).max)
    half_ulp = np.float64(2.0 ** 103)                   # half an ulp of float at FLT_MAX
    edge = [fmax, -fmax, np.nextafter(fmax, np.inf), np.nextafter(fmax + half_ulp, 0.0), fmax + half_ulp, 1e300, -1e300,
            2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 3 * 2.0 ** -150, 2.0 ** -140 + 2.0 ** -151, 1e-320,
            1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, -(1.0 + 2.0 ** -24), 0.0, -0.0, 1.0 / 3.0]
    v = np.random.default_rng(n).uniform(-4.0, 4.0, n)
    k = min(n, len(edge))
    start = (n * 7) % len(edge)
    v[:k] = [edge[(start + t) % len(edge)] for t in range(k)]
    return v


def demote_failures(lab):
    """Every size, every misalignment (dst 0 .. 3 floats, src 0 or 1 double behind a 16-byte boundary; src and dst
    misaligned differently is the one-by-one route of the launcher), finite inputs in and out of float's range, and one
    NaN / one infinity.  The flag must be raised exactly when an entry is NaN, infinite or above FLT_MAX."""
    bad = []
    for n in DEMOTE_SIZES:
        for special in (None, np.nan, -np.inf):
            v = demote_values(n)
            if special is not None:
                v[n // 2] = special
            elif n in (4, 1024):
                v = np.clip(v, -fmax_f64(), fmax_f64())     # all in range: the flag must stay down
            want32 = round_f32(v)
            want_flag = bool((~(np.abs(v) <= FLT_MAX)).any())
            for so in (0, 1):
                for do in (0, 1, 2, 3) if special is None else (1,):
                    out, flag = lab.demote(1, v, so, do)
                    if not same_bits(out[do: do + n], want32):
                        bad.append("demote n=%d src+%d dst+%d: differs from astype(float32)" % (n, so, do))
                    if not ((out[:do].view(np.uint32) == CANARY32).all() and (out[do + n:].view(np.uint32) == CANARY32).all()):
                        bad.append("demote n=%d src+%d dst+%d: wrote outside its n entries" % (n, so, do))
                    if bool(flag & 4) != want_flag or flag & ~4:
                        bad.append("demote n=%d src+%d dst+%d: flag %d, expected %s" % (n, so, do, flag, want_flag))
                out, flag = lab.demote(2, v, so, 0)
                if not same_bits(out[so: so + n], want32.astype(np.float64)):
                    bad.append("round n=%d src+%d: differs from astype(float32)" % (n, so))
                if not (is_canary(out[:so]).all() and is_canary(out[so + n:]).all()):
                    bad.append("round n=%d src+%d: wrote outside its n entries" % (n, so))
                if bool(flag & 4) != want_flag or flag & ~4:
                    bad.append("round n=%d src+%d: flag %d, expected %s" % (n, so, flag, want_flag))
    return bad


def fmax_f64():
    return np.float64(np.finfo(np.float32).max)
