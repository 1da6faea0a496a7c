"""Kernel lab of the separator-side, vector and table kernels of the device layer: the case list, the numpy references, the
bounds, the ctypes driver of the harness (sep_harness.cpp) and the coverage bookkeeping.

Every case calls one launcher of device.hpp on a shape chosen to reach a branch that whole-preconditioner runs do not
reach (or reach without telling a wrong result from rounding).  The references are restatements of the OPERATION in numpy,
written for this lab; none is derived from the host simulator or from a kernel.

Bounds
  tables and sums   integer-valued doubles below 2^20: every order of summation is exact, the result must EQUAL the
                    numpy restatement
  dot products      (spmv, dot, blocks_apply*)  reference in np.longdouble; per output 2 * n * eps * sum_j |a_j x_j| (times
                    |alpha|, plus 2 * eps * |beta y| for spmv), n = number of summands, eps = 2^-53.  The factor 2 is the only
                    margin: the bound is the textbook proof for any order of the sum, not a measurement
  ot_apply          2 w (w.x) - x per group in np.longdouble, same form with n = group size + 2
  Householder       (sblock_transform + sblock_extract, sblock_kept)  T = H S H with every H_g dense in np.longdouble
                    (Householder::Apply semantics: sg = sign of the leading entry, u = [sg v0 + nrm, sg v1, ...],
                    H = u u' / (nrm u0) - I, identity when |u0| or nrm is below 1e-14).  No a-priori tolerance: per case
                    the error of the SAME dense H S H in float64 against the longdouble one is measured, the bound is 16
                    times that, at least 16 * eps * max|T|.  Both routes are compared with the reference, never with
                    each other alone.
  dense_invert*     np.linalg.inv; |X - inv| <= 1e-13 cond max|inv| and |X A - I| <= 1e-13 cond (the bounds of
                    test_separator_block_inversion_gpu)

Measured float64 reference errors of the Householder cases (max over T and the slots, the bound is 16 times the larger of
the two columns):

  case              f64 error    eps * max|T|
  hh_5x1_nbc1       3.1e-16      1.3e-16
  hh_5x1_nbc3       0            1.1e-16      (every slice is an identity case: T = S)
  hh_40x6_nbc1      3.5e-16      1.8e-16
  hh_40x6_nbc3      8.8e-16      2.0e-16
  hh_64x8_nbc1      7.4e-16      1.9e-16
  hh_64x8_nbc3      7.4e-16      2.3e-16
  hh_300x40_nbc1    8.8e-16      2.3e-16
  hh_300x40_nbc3    1.0e-15      2.3e-16
  hh_300x260_nbc1   7.2e-16      2.2e-16
  hh_300x260_nbc3   5.4e-16      2.1e-16

Test-vector rule of the Householder cases: every slice is clearly on one side of the 1e-14 threshold (leading entry exactly
0, norm below 1e-20, or norm above 1e-3), so that the identity decision does not depend on rounding; tv_rule_failures().
"""
import ctypes
import os
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"sim": os.path.join(HERE, "libseplab_sim.so"), "gpu": os.path.join(HERE, "libseplab_gpu.so")}

EPS = 2.0 ** -53
LD = np.longdouble
CANARY = 0x7ff4dead5eed5eed
GJ_LDS_NB = 88              # largest order dense_invert_all inverts inside LDS

# environment variants of the GPU run (the switches are read once per process)
VARIANTS = [
    ("default", {}),
    ("blocked_min", {"HYMLS_MI_INVERT_BLOCKED_MIN": "100000"}),
    ("mv_group_1", {"HYMLS_MI_MV_GROUP_BLK": "1"}),
    ("mv_group_2", {"HYMLS_MI_MV_GROUP_BLK": "2"}),
]


class Case:
    def __init__(self, name, family, variants=("default",), sim=True, **params):
        self.name, self.family, self.variants, self.sim, self.p = name, family, tuple(variants), sim, params

    def rng(self, salt=0):
        return np.random.default_rng(zlib.crc32(self.name.encode()) + salt)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------ the harness
def build(which):
    subprocess.check_call(["make", "-s", "-C", HERE, which])
    return LIBS[which]


_SIGS = {
    "gather": "qppqpq", "scatter": "qpppqqi", "spmv": "ippppqpqqddq", "dot": "qppp", "pull_sum": "qpppqpq",
    "pull_sum_blocks": "qipppqpq", "build_pull_tables": "qppppqpq", "member_sources": "iiipppipppqp",
    "offdiag": "qpippippppqpqpqq", "ot_apply": "ippqpqq", "transform_extract": "iipppqiqppqq",
    "sblock_kept": "iipppippppipqq", "dense_invert": "iipqp", "dense_invert_all": "ipppqqip", "blocks_apply": "iipppqpq",
    "blocks_apply_all": "ipppppqpqipqpq", "blocks_apply_all_mv": "ipppppqpqipqpqiq", "blocks_apply_tile": "iiippqpqiq",
}
_CT = {"q": ctypes.c_int64, "i": ctypes.c_int32, "p": ctypes.c_void_p, "d": ctypes.c_double}
_loaded = {}


class Lib:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name, sig in _SIGS.items():
            f = getattr(self.lib, "seplab_" + name)
            f.argtypes = [_CT[c] for c in sig] + [ctypes.c_char_p, ctypes.c_int32]
            f.restype = ctypes.c_int
        for name, args in (("spmv_lanes", [ctypes.c_int32, ctypes.c_int64]), ("invert_blocked_order", [ctypes.c_int32]),
                           ("kept_fits", [ctypes.c_int32, ctypes.c_int32])):
            f = getattr(self.lib, "seplab_" + name)
            f.argtypes, f.restype = args, ctypes.c_int32
        self.lib.seplab_guard_words.restype = ctypes.c_int64
        self.guard = int(self.lib.seplab_guard_words())

    def call(self, name, *args):
        """Returns (code, message); arrays are passed by pointer and must be contiguous."""
        conv, keep = [], []
        for c, a in zip(_SIGS[name], args):
            if c == "p":
                if a is None:
                    conv.append(None)
                else:
                    assert isinstance(a, np.ndarray) and a.flags.c_contiguous, name
                    keep.append(a)
                    conv.append(a.ctypes.data_as(ctypes.c_void_p))
            else:
                conv.append(a)
        assert len(conv) == len(_SIGS[name]), name
        err = ctypes.create_string_buffer(512)
        code = getattr(self.lib, "seplab_" + name)(*conv, err, 512)
        return code, err.value.decode(errors="replace")

    def run(self, name, *args):
        code, msg = self.call(name, *args)
        if code != 0:
            raise RuntimeError("seplab_%s: error %d: %s" % (name, code, msg))

    def spmv_lanes(self, nrows, hint):
        return int(self.lib.seplab_spmv_lanes(nrows, hint))

    def blocked_order(self, nb):
        return bool(self.lib.seplab_invert_blocked_order(nb))

    def kept_fits(self, nS, ngl):
        return bool(self.lib.seplab_kept_fits(nS, ngl))

    def out(self, n, dtype=np.float64, init=None):
        """Host side of an output buffer: n payload elements and the guard tail; the harness fills everything behind the
        initial content with the canary."""
        item = np.dtype(dtype).itemsize
        words = (n * item + 7) // 8 + self.guard
        a = np.zeros(words * 8 // item, dtype=dtype)
        if init is not None:
            a[:len(init)] = init
        return a


def load(which):
    if which not in _loaded:
        _loaded[which] = Lib(build(which))
    return _loaded[which]


def words(a):
    return a.nbytes // 8


def untouched(buf, defined):
    """True where an element outside `defined` (boolean mask over the payload; the guard tail is never defined) still holds
    the canary bits."""
    raw = np.uint64 if buf.dtype.itemsize == 8 else np.uint32
    want = np.full(buf.nbytes // 8, CANARY, dtype=np.uint64).view(raw)
    same = buf.view(raw) == want
    mask = np.zeros(buf.size, dtype=bool)
    mask[:len(defined)] = defined
    return bool(np.all(same[~mask]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ints(rng, n, lim=1 << 19):
    """Integer-valued doubles: sums of any thousand of them are exact in any order."""
    return rng.integers(-lim, lim, n).astype(np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


# ------------------------------------------------------------------ families
# Every family has inputs(case) -> dict (deterministic), run(lib, case, inp) -> dict of arrays (whole buffers) and
# check(case, inp, out) -> (list of failures, largest error / bound).
_inputs = {}


def inputs(case):
    if case.name not in _inputs:
        _inputs[case.name] = FAMILIES[case.family][0](case)
    return _inputs[case.name]


def run_case(lib, case):
    return FAMILIES[case.family][1](lib, case, inputs(case))


def check_case(case, out):
    return FAMILIES[case.family][2](case, inputs(case), out)


def _exact(name, got, want, fails):
    if not same_bits(np.asarray(got), np.asarray(want, dtype=got.dtype)):
        bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
        fails.append("%s differs from the restatement at %d positions (first %s)" % (name, bad.size, bad[:3]))


def _bounded(name, got, ref, bound, fails):
    """|got - ref| <= bound elementwise (ref longdouble); returns the largest error / bound."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        fails.append("%s: not finite" % name)
        return np.inf
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        k = int(np.argmax(ratio))
        fails.append("%s: error %.3g above the bound %.3g at %d" % (name, err.ravel()[k], bound.ravel()[k], k))
    return worst


# ---- gather / scatter / scatter_add
def gs_inputs(case):
    rng, op = case.rng(), case.p["op"]
    if op == "gather":
        src = ints(rng, 1500)
        return {"idx": i32(rng.integers(0, 1500, 1000)), "src": src}
    if op == "scatter":
        return {"idx": i32(rng.permutation(1500)[:1000]), "src": ints(rng, 1000), "dst": ints(rng, 1500)}
    return {"idx": i32(rng.integers(0, 7, 1000) * 3), "src": ints(rng, 1000), "dst": ints(rng, 25)}   # 1000 sources, 7 targets


def gs_run(lib, case, inp):
    op = case.p["op"]
    if op == "gather":
        dst = lib.out(1000)
        lib.run("gather", 1000, inp["idx"], inp["src"], 1500, dst, words(dst))
    else:
        dst = lib.out(len(inp["dst"]), init=inp["dst"])
        lib.run("scatter", 1000, inp["idx"], inp["src"], dst, len(inp["dst"]), words(dst), int(op == "scatter_add"))
    return {"dst": dst}


def gs_check(case, inp, out):
    fails, op = [], case.p["op"]
    if op == "gather":
        want = inp["src"][inp["idx"]]
    elif op == "scatter":
        want = inp["dst"].copy()
        want[inp["idx"]] = inp["src"]
    else:
        want = inp["dst"].copy()
        np.add.at(want, inp["idx"], inp["src"])
    _exact("dst", out["dst"][:len(want)], want, fails)
    if not untouched(out["dst"], np.ones(len(want), bool)):
        fails.append("written behind the output")
    return fails, 0.0


# ---- pull_sum
def ps_inputs(case):
    rng = case.rng()
    lens = rng.choice([0, 1], 1200)
    lens = np.concatenate([[0], lens, [1000, 0, 1000, 1, 1000]])       # empty first range; three long ones
    ptr = i64(np.concatenate([[0], np.cumsum(lens)]))
    return {"ptr": ptr, "idx": i64(rng.integers(0, 5000, ptr[-1])), "in": ints(rng, 5000)}


def ps_run(lib, case, inp):
    n = len(inp["ptr"]) - 1
    o = lib.out(n)
    lib.run("pull_sum", n, inp["ptr"], inp["idx"], inp["in"], 5000, o, words(o))
    return {"out": o}


def ps_check(case, inp, out):
    fails, ptr = [], inp["ptr"]
    want = np.array([inp["in"][inp["idx"][ptr[e]:ptr[e + 1]]].sum() for e in range(len(ptr) - 1)])
    _exact("out", out["out"][:len(want)], want, fails)
    if not untouched(out["out"], np.ones(len(want), bool)):
        fails.append("written behind the output")
    return fails, 0.0


# ---- pull_sum_blocks
def psb_inputs(case):
    rng, blen = case.rng(), case.p["blen"]
    ptr = i64([0, 2, 2, 5])                                             # the middle block has an empty range
    base = i64(rng.integers(0, 3 * blen, 5))
    return {"ptr": ptr, "base": base, "in": ints(rng, 4 * blen)}


def psb_run(lib, case, inp):
    blen = case.p["blen"]
    o = lib.out(3 * blen)
    lib.run("pull_sum_blocks", blen, 3, inp["ptr"], inp["base"], inp["in"], len(inp["in"]), o, words(o))
    return {"out": o}


def psb_check(case, inp, out):
    fails, blen, ptr = [], case.p["blen"], inp["ptr"]
    want = np.zeros((3, blen))
    for B in range(3):
        for t in range(ptr[B], ptr[B + 1]):
            want[B] += inp["in"][inp["base"][t]:inp["base"][t] + blen]
    _exact("out", out["out"][:3 * blen], want.ravel(), fails)
    if not untouched(out["out"], np.ones(3 * blen, bool)):
        fails.append("written behind the output")
    return fails, 0.0


# ---- build_pull_tables
def bpt_inputs(case):
    rng = case.rng()
    rows = case.p["rows"]            # per row: run lengths of equal column gids
    keys, rcount, rowptr, pos = [], [0], [0], 0
    for r, runs in enumerate(rows):
        gids = np.sort(rng.choice(1 << 20, len(runs), replace=False))
        for g, n in zip(gids, runs):
            srcs = np.sort(rng.choice(1 << 30, n, replace=False)).astype(np.uint64)
            if case.p.get("big") == (r, pos):
                srcs[-1] = (1 << 32) + 5                                # a source position that needs bit 32 of the key
            keys += [(int(g) << 33) | int(s) for s in srcs]
            pos += 1
        rcount.append(len(keys))
        rowptr.append(rowptr[-1] + len(runs))
    return {"keys": np.array(keys, dtype=np.uint64), "rcount": i64(rcount), "rowptr": i32(rowptr)}


def bpt_run(lib, case, inp):
    nr, ne, nk = len(inp["rcount"]) - 1, int(inp["rowptr"][-1]), len(inp["keys"])
    ptr, idx = lib.out(ne + 1, np.int64), lib.out(nk, np.int64)
    lib.run("build_pull_tables", nr, inp["rcount"], inp["rowptr"], inp["keys"], ptr, words(ptr), idx, words(idx))
    return {"ptr": ptr, "idx": idx}


def bpt_check(case, inp, out):
    fails, keys = [], inp["keys"]
    gid = (keys >> np.uint64(33)).astype(np.int64)
    want_idx = (keys & np.uint64((1 << 33) - 1)).astype(np.int64)
    want_ptr = [0]
    for r in range(len(inp["rcount"]) - 1):
        k0, k1 = int(inp["rcount"][r]), int(inp["rcount"][r + 1])
        ends = [k + 1 for k in range(k0, k1) if k + 1 == k1 or gid[k + 1] != gid[k]]
        want_ptr += ends
    want_ptr = i64(want_ptr)
    assert len(want_ptr) == inp["rowptr"][-1] + 1
    _exact("ptr", out["ptr"][:len(want_ptr)], want_ptr, fails)
    _exact("idx", out["idx"][:len(want_idx)], want_idx, fails)
    if not (untouched(out["ptr"], np.ones(len(want_ptr), bool)) and untouched(out["idx"], np.ones(len(want_idx), bool))):
        fails.append("written behind the output")
    return fails, 0.0


# ---- member_sources
MS = dict(nk=60, nb=2, next=12, nent=16389)


def ms_inputs(case):
    rng = case.rng()
    nk, nb, nx, nent = MS["nk"], MS["nb"], MS["next"], MS["nent"]
    ext = np.stack([rng.permutation(nk)[:nx] for _ in range(nb)])
    er, ec = rng.integers(0, nx, nent), rng.integers(0, nx, nent)
    need = {(int(ext[b, a]), int(ext[b, c])) for b in range(nb) for a, c in zip(er, ec)}
    need.discard((int(ext[1, er[77]]), int(ext[1, ec[77]])))           # one entry of member 1 does not exist
    rows = [sorted(c for (r, c) in need if r == i) for i in range(nk)]
    krow = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    kcol = np.array([c for r in rows for c in r])
    return {"ext": i32(ext), "er": i32(er), "ec": i32(ec), "krow": i32(krow), "kcol": i32(kcol)}


def ms_run(lib, case, inp):
    src, flag = lib.out(MS["nb"] * MS["nent"], np.int32), np.zeros(1, np.int32)
    lib.run("member_sources", MS["nb"], MS["next"], MS["nent"], inp["ext"], inp["er"], inp["ec"], MS["nk"], inp["krow"], inp["kcol"],
            src, words(src), flag)
    return {"src": src, "flag": flag}


def ms_reference(inp):
    krow, kcol = inp["krow"], inp["kcol"]
    want = np.zeros((MS["nb"], MS["nent"]), np.int32)
    missing = 0
    for b in range(MS["nb"]):
        r, c = inp["ext"][b][inp["er"]], inp["ext"][b][inp["ec"]]
        for q in range(MS["nent"]):
            hit = np.flatnonzero(kcol[krow[r[q]]:krow[r[q] + 1]] == c[q])
            if hit.size:
                want[b, q] = krow[r[q]] + hit[0]
            else:
                missing += 1
    return want, missing


def ms_check(case, inp, out):
    fails = []
    want, missing = ms_reference(inp)
    n = want.size
    _exact("src", out["src"][:n], want.ravel(), fails)
    if missing == 0 or int(out["flag"][0]) & 1 != 1:
        fails.append("flag %d with %d missing entries" % (out["flag"][0], missing))
    if not untouched(out["src"], np.ones(n, bool)):
        fails.append("written behind the output")
    return fails, 0.0


# ---- offdiag_count + offdiag_fill
def od_inputs(case):
    rng, nk = case.rng(), 30
    rows_cols = [np.sort(rng.choice(nk, rng.integers(1, 9), replace=False)) for _ in range(nk)]
    ta = np.where(rng.random(nk) < 0.4, rng.integers(0, 100, nk), -1)
    tb = np.where(rng.random(nk) < 0.7, rng.integers(100, 200, nk), -1)
    excl = np.where(rng.random(nk) < 0.3, 1, -1)
    dead = rows_cols[5]                                                 # row 5 keeps nothing
    ta[dead], excl[dead] = -1, 1
    krow = np.concatenate([[0], np.cumsum([len(r) for r in rows_cols])])
    rows = rng.permutation(nk)[:20]
    rows[3] = 5
    return {"rows": i32(rows), "krow": i32(krow), "kcol": i32(np.concatenate(rows_cols)), "ta": i32(ta), "tb": i32(tb), "excl": i32(excl)}


def od_reference(case, inp):
    ta, tb, excl = inp["ta"], (inp["tb"] if case.p["tb"] else None), inp["excl"]
    count, col, src = [], [], []
    for r in inp["rows"]:
        n = 0
        for e in range(inp["krow"][r], inp["krow"][r + 1]):
            c = inp["kcol"][e]
            tg = ta[c] if ta[c] >= 0 else (tb[c] if tb is not None and excl[c] < 0 else -1)
            if tg >= 0:
                col.append(tg); src.append(e); n += 1
        count.append(n)
    return i32(count), i32(col), i32(src)


def od_run(lib, case, inp):
    count_w, col_w, _ = od_reference(case, inp)
    nrows, cap = len(inp["rows"]), len(col_w)
    count, col, src = lib.out(nrows + 1, np.int32), lib.out(cap, np.int32), lib.out(cap, np.int32)
    lib.run("offdiag", nrows, inp["rows"], 30, inp["krow"], inp["kcol"], 30, inp["ta"], inp["tb"] if case.p["tb"] else None, inp["excl"],
            count, words(count), col, words(col), src, words(src), cap)
    return {"count": count, "col": col, "src": src}


def od_check(case, inp, out):
    fails = []
    count_w, col_w, src_w = od_reference(case, inp)
    if 0 not in count_w:
        fails.append("no row without a kept entry")
    nrows = len(count_w)
    _exact("count", out["count"][1:nrows + 1], count_w, fails)
    _exact("col", out["col"][:len(col_w)], col_w, fails)
    _exact("src", out["src"][:len(src_w)], src_w, fails)
    defined = np.ones(nrows + 1, bool)
    defined[0] = False                                                  # count[0] belongs to the caller
    if not (untouched(out["count"], defined) and untouched(out["col"], np.ones(len(col_w), bool)) and
            untouched(out["src"], np.ones(len(src_w), bool))):
        fails.append("written outside the output set")
    return fails, 0.0


# ---- spmv
SPMV_AB = [(1.0, 0.0), (-1.0, 1.0), (2.5, -0.5)]
SPMV_LENS = [0, 1, 2, 33, 100]


def spmv_inputs(case):
    rng, nrows = case.rng(), case.p["nrows"]
    lens = np.array([SPMV_LENS[(i * 7 + i // 5) % 5] for i in range(nrows)])
    if nrows == 1:
        lens[:] = 33
    rp = np.concatenate([[0], np.cumsum(lens)])
    nx = 400
    col = np.concatenate([rng.choice(nx, n, replace=False) for n in lens] + [np.zeros(0, np.int64)])
    return {"rp": i32(rp), "col": i32(col), "val": rng.uniform(-1, 1, rp[-1]), "x": rng.uniform(-1, 1, nx), "y": rng.uniform(-1, 1, nrows)}


def spmv_hint(case, inp):
    # chosen so that the launcher takes case.p["lanes"] lanes per row (-1: the call without a hint)
    return {1: case.p["nrows"], 2: 3 * case.p["nrows"], 4: 10 * case.p["nrows"], 8: 40 * case.p["nrows"], 0: -1}[case.p["lanes"]]


def spmv_run(lib, case, inp):
    nrows, res = case.p["nrows"], {}
    for k, (alpha, beta) in enumerate(SPMV_AB):
        y0 = np.full(nrows, np.nan) if beta == 0.0 else inp["y"]
        y = lib.out(nrows, init=y0)
        lib.run("spmv", nrows, inp["rp"], inp["col"], inp["val"], inp["x"], len(inp["x"]), y, nrows, words(y), alpha, beta, spmv_hint(case, inp))
        res["y%d" % k] = y
    return res


def spmv_check(case, inp, out):
    fails, worst, nrows, rp = [], 0.0, case.p["nrows"], inp["rp"]
    prod = inp["val"].astype(LD) * inp["x"][inp["col"]].astype(LD)
    s = np.array([prod[rp[i]:rp[i + 1]].sum() for i in range(nrows)], dtype=LD)
    sa = np.array([np.abs(prod[rp[i]:rp[i + 1]]).sum() for i in range(nrows)], dtype=LD)
    n = np.diff(rp)
    for k, (alpha, beta) in enumerate(SPMV_AB):
        by = LD(beta) * inp["y"].astype(LD) if beta != 0.0 else np.zeros(nrows, LD)
        ref = LD(alpha) * s + by
        bound = 2 * (n * EPS * abs(alpha) * sa + EPS * np.abs(by))
        worst = max(worst, _bounded("y (alpha %g, beta %g)" % (alpha, beta), out["y%d" % k][:nrows], ref, bound, fails))
        if not untouched(out["y%d" % k], np.ones(nrows, bool)):
            fails.append("written behind y")
    return fails, worst


# ---- dot
def dot_inputs(case):
    rng, n = case.rng(), case.p["n"]
    return {"x": rng.uniform(-1, 1, n), "y": rng.uniform(-1, 1, n)}


def dot_run(lib, case, inp):
    o = np.zeros(1)
    lib.run("dot", case.p["n"], inp["x"], inp["y"], o)
    return {"dot": o}


def dot_check(case, inp, out):
    fails = []
    prod = inp["x"].astype(LD) * inp["y"].astype(LD)
    worst = _bounded("dot", out["dot"], np.array([prod.sum()]), [2 * case.p["n"] * EPS * float(np.abs(prod).sum())], fails)
    return fails, worst


# ---- ot_apply
OT_SIZES = [1, 2, 7, 8, 9, 16, 17, 40]
OT_TAIL = 5


def ot_inputs(case):
    rng, ng = case.rng(), case.p["ng"]
    sizes = [9] if ng == 1 else [OT_SIZES[(3 * g + g // 8) % 8] for g in range(ng)]
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(gptr[-1])
    w = rng.uniform(-1, 1, n)
    if ng > 1:
        z = ng // 2
        w[gptr[z]:gptr[z + 1]] = 0.0                                    # "x <- -x"
    return {"gptr": i32(gptr), "w": w, "x": rng.uniform(-1, 1, n + OT_TAIL)}


def ot_run(lib, case, inp):
    x = lib.out(len(inp["x"]), init=inp["x"])
    lib.run("ot_apply", case.p["ng"], inp["gptr"], inp["w"], len(inp["w"]), x, len(inp["x"]), words(x))
    return {"x": x}


def ot_check(case, inp, out):
    fails, gptr = [], inp["gptr"]
    n = int(gptr[-1])
    w, x = inp["w"].astype(LD), inp["x"][:n].astype(LD)
    ref, bound = np.zeros(n, LD), np.zeros(n)
    for g in range(case.p["ng"]):
        sl = slice(gptr[g], gptr[g + 1])
        s, sa = (w[sl] * x[sl]).sum(), np.abs(w[sl] * x[sl]).sum()
        ref[sl] = 2 * w[sl] * s - x[sl]
        bound[sl] = 2 * (gptr[g + 1] - gptr[g] + 2) * EPS * (2 * np.abs(w[sl]) * sa + np.abs(x[sl]))
    worst = _bounded("x", out["x"][:n], ref, bound, fails)
    if not same_bits(out["x"][n:n + OT_TAIL], inp["x"][n:]):
        fails.append("the tail of x behind gptr[ng] changed")
    if not untouched(out["x"], np.ones(n + OT_TAIL, bool)):
        fails.append("written behind x")
    return fails, worst


# ---- Householder transform of the separator blocks: two-pass route and the kept-entries kernel
HH_SHAPES = {
    # name: (group sizes, linked sets).  Linked sets: a group alone, three groups with a one-node group in the middle, a pair
    # of 18-node groups ((nI-1)(nJ-1) = 289 > 256), a set of one-node groups only (blk_len = 0: glink stays -1)
    "5x1": ([5], []),
    "40x6": ([9, 8, 1, 5, 4, 13], [[0], [1, 2, 3]]),
    "64x8": ([17, 18, 18, 1, 2, 3, 4, 1], [[1, 2], [4, 3, 5], [7], [0]]),
    "300x40": ([17, 18, 18, 9, 8, 5, 4, 3, 2, 1] * 3 + [9, 8, 5, 4, 3, 2, 1, 1, 7, 5], [[1, 2], [3, 9, 4], [0], [19, 29], [13, 36, 14]]),
    "300x260": ([1] * 100 + [9, 1, 9] + [1] * 100 + [9, 9, 9] + [1] * 54, [[100, 101, 102], [203], [0, 1], [204, 150, 205]]),
}
HH_KINDS = ["constant", "signs", "negative", "lead0", "zero", "tiny"]
HH_PAD = 7


def hh_layout(sizes, linked):
    """The record layout KeptD describes: V-sum x V-sum (ngl x ngl, column-major), then the non-V-sum block of every linked
    set.  Returns gptr, glink, goff, lboff, lblen, record length."""
    ngl = len(sizes)
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    glink, goff = np.full(ngl, -1), np.zeros(ngl, np.int64)
    lblen = [sum(sizes[g] - 1 for g in L) for L in linked]
    lboff, off = [], ngl * ngl
    for L, n in zip(linked, lblen):
        lboff.append(off)
        off += n * n
        o = 0
        for g in L:
            if n > 0:
                glink[g], goff[g] = linked.index(L), o
            o += sizes[g] - 1
    return gptr, glink, goff, lboff, lblen, off


def hh_inputs(case):
    rng = case.rng()
    sizes, linked = HH_SHAPES[case.p["shape"]]
    nbc, nS = case.p["nbc"], sum(sizes)
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    tv = np.zeros((nbc, nS))
    kinds = np.zeros((nbc, len(sizes)), np.int64)
    for s in range(nbc):
        for g, n in enumerate(sizes):
            kind = HH_KINDS[(g + 2 * s + (0 if nbc == 1 else 1)) % len(HH_KINDS)] if len(sizes) > 1 else HH_KINDS[2 if nbc == 1 else 3 + s]
            kinds[s, g] = HH_KINDS.index(kind)
            v = {"constant": np.full(n, 0.5 + s), "signs": rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 1, n),
                 "negative": np.concatenate([[-0.7], rng.uniform(-1, 1, n - 1)]), "lead0": np.concatenate([[0.0], rng.uniform(0.1, 1, n - 1)]),
                 "zero": np.zeros(n), "tiny": np.full(n, 1e-22)}[kind]
            tv[s, gptr[g]:gptr[g + 1]] = v
    S = rng.uniform(-1, 1, (nbc, nS, nS))                               # S[s][i, j]; the device block is column-major
    return {"sizes": sizes, "linked": linked, "tv": tv, "S": S, "kinds": kinds}


def tv_rule_failures(case):
    """Every slice is clearly on one side of the identity threshold."""
    inp, bad = inputs(case), []
    gptr = np.concatenate([[0], np.cumsum(inp["sizes"])])
    for s in range(case.p["nbc"]):
        for g in range(len(inp["sizes"])):
            v = inp["tv"][s, gptr[g]:gptr[g + 1]]
            nrm = float(np.sqrt((v.astype(LD) ** 2).sum()))
            if not (v[0] == 0.0 or nrm < 1e-20 or nrm > 1e-3):
                bad.append("%s: slot %d group %d: norm %.3g" % (case.name, s, g, nrm))
    return bad


def householder(v, dtype, mutant=None):
    """H of one test-vector slice as a dense matrix (Householder::Apply semantics)."""
    n = len(v)
    v = v.astype(dtype)
    sg = dtype(-1.0) if v[0] < 0 else (dtype(1.0) if v[0] > 0 else dtype(0.0))
    if mutant == "no_identity":                                         # a kernel that drops the identity cases
        sg = dtype(-1.0) if v[0] < 0 else dtype(1.0)
        if not np.any(v):
            return -np.eye(n, dtype=dtype)
    nrm = np.sqrt((v * v).sum()) * abs(sg)
    u = sg * v
    u[0] = u[0] + nrm
    if mutant != "no_identity" and (abs(u[0]) < 1e-14 or nrm < 1e-14):
        return np.eye(n, dtype=dtype)
    return np.outer(u, u) / (nrm * u[0]) - np.eye(n, dtype=dtype)


def hh_transform(inp, dtype, mutant=None):
    """T[s] = H S[s] H, H block diagonal with one dense H_g per group."""
    gptr = np.concatenate([[0], np.cumsum(inp["sizes"])])
    T = inp["S"].astype(dtype)
    for s in range(T.shape[0]):
        for g in range(len(inp["sizes"])):
            sl = slice(gptr[g], gptr[g + 1])
            H = householder(inp["tv"][s, sl], dtype, mutant)
            T[s, sl, :] = H @ T[s, sl, :]
        for g in range(len(inp["sizes"])):
            sl = slice(gptr[g], gptr[g + 1])
            H = householder(inp["tv"][s, sl], dtype, mutant)
            T[s, :, sl] = T[s, :, sl] @ H
    return T


def hh_pick(inp, mutant=None):
    """(row, column) of T for every record position."""
    sizes, linked = inp["sizes"], inp["linked"]
    gptr, glink, goff, lboff, lblen, rec = hh_layout(sizes, linked)
    ngl = len(sizes)
    ri, ci = np.full(rec, -1), np.full(rec, -1)
    for J in range(ngl):
        for I in range(ngl):
            ri[I + ngl * J], ci[I + ngl * J] = gptr[I], gptr[J]
    for li, L in enumerate(linked):
        for I in L:
            for J in L:
                for a in range(1, sizes[I]):
                    for b in range(1, sizes[J]):
                        k = lboff[li] + (goff[I] + a - 1) + lblen[li] * (goff[J] + b - 1)
                        if mutant == "swap_ij":                         # a kernel that swaps the roles of I and J in a linked block
                            ri[k], ci[k] = gptr[J] + b, gptr[I] + a
                        else:
                            ri[k], ci[k] = gptr[I] + a, gptr[J] + b
    assert ri.min() >= 0
    return ri, ci


_hh_ref = {}


def hh_reference(case):
    """(T in longdouble, error of the float64 restatement, bound of the case)."""
    if case.name not in _hh_ref:
        inp = inputs(case)
        T = hh_transform(inp, LD)
        f64_err = float(np.abs(hh_transform(inp, np.float64).astype(LD) - T).max())
        floor = EPS * float(np.abs(T).max())
        _hh_ref[case.name] = (T, f64_err, 16 * max(f64_err, floor), floor)
    return _hh_ref[case.name]


def hh_run(lib, case, inp):
    sizes, linked, nbc = inp["sizes"], inp["linked"], case.p["nbc"]
    gptr, glink, goff, lboff, lblen, rec = hh_layout(sizes, linked)
    nS, ngl, stride = int(gptr[-1]), len(sizes), rec + HH_PAD
    Scm = np.ascontiguousarray(inp["S"].transpose(0, 2, 1))            # column-major blocks
    tv = np.ascontiguousarray(inp["tv"])
    res = {"fits": np.array([lib.kept_fits(nS, ngl)])}
    out = lib.out(nbc * stride)
    lib.run("sblock_kept", nS, ngl, i32(gptr), i32(glink), i32(goff), len(linked), i64(lboff + [0]), i32(lblen + [0]), tv, Scm, nbc,
            out, stride, words(out))
    res["kept"] = out
    ri, ci = hh_pick(inp)
    sb, out2 = lib.out(nbc * nS * nS, init=Scm.ravel()), lib.out(nbc * stride)
    lib.run("transform_extract", nS, ngl, i32(gptr), tv, sb, words(sb), nbc, rec, i32(ri + nS * ci), out2, stride, words(out2))
    res["two_pass"], res["sblock"] = out2, sb
    return res


def hh_check(case, inp, out, mutant=None):
    fails = []
    T, _, bound, _ = hh_reference(case)
    nbc, nS = case.p["nbc"], T.shape[1]
    ri, ci = hh_pick(inp)
    rec = len(ri)
    stride = rec + HH_PAD
    want = np.stack([T[s][ri, ci] for s in range(nbc)])
    defined = np.zeros(nbc * stride, bool)
    for s in range(nbc):
        defined[s * stride:s * stride + rec] = True
    worst = 0.0
    for route in ("kept", "two_pass"):
        got = out[route][:nbc * stride].reshape(nbc, stride)[:, :rec]
        worst = max(worst, _bounded(route, got, want, np.full(want.shape, bound), fails))
        if not untouched(out[route], defined):
            fails.append("%s: written outside the records" % route)
    full = out["sblock"][:nbc * nS * nS].reshape(nbc, nS, nS).transpose(0, 2, 1)
    worst = max(worst, _bounded("transformed block", full, T, np.full(T.shape, bound), fails))
    if not untouched(out["sblock"], np.ones(nbc * nS * nS, bool)):
        fails.append("written behind the separator blocks")
    return fails, worst


def hh_mutant_record(case, mutant):
    """The records a wrong kernel would produce (float64 numpy), in the layout of the kept-entries output."""
    inp = inputs(case)
    T = hh_transform(inp, np.float64, "no_identity" if mutant == "no_identity" else None)
    ri, ci = hh_pick(inp, "swap_ij" if mutant == "swap_ij" else None)
    return np.stack([T[s][ri, ci] for s in range(case.p["nbc"])])


# ---- dense_invert / dense_invert_all
def inv_block(rng, nb, kind):
    B = rng.uniform(-1, 1, (nb, nb))
    if kind == "dominant" or nb == 1:
        B += nb * np.eye(nb)
    elif kind == "zero_diag":
        B[np.arange(nb), np.arange(nb)] = 0.0                           # no LU without interchanges
    elif kind == "tridiag":
        B = 65536.0 * (np.diag(np.full(nb, 6.0)) - np.diag(np.ones(nb - 1), 1) - np.diag(np.ones(nb - 1), -1))
    elif kind == "singular":
        B[:, nb // 3] = 0.0
    return B


INV_KINDS = ["dominant", "zero_diag", "tridiag", "random"]


def inv_inputs(case):
    rng = case.rng()
    orders = case.p["orders"]
    kinds = case.p.get("kinds") or [INV_KINDS[(k + 1) % 4] for k in range(len(orders))]
    return {"blocks": [inv_block(rng, nb, kd) for nb, kd in zip(orders, kinds)], "kinds": kinds}


def inv_run(lib, case, inp):
    orders, flag = case.p["orders"], np.zeros(1, np.int32)
    flat = np.concatenate([B.T.ravel() for B in inp["blocks"]])        # column-major
    buf = lib.out(len(flat), init=flat)
    if case.p.get("uniform"):
        lib.run("dense_invert", orders[0], len(orders), buf, words(buf), flag)
    else:
        boff = np.concatenate([[0], np.cumsum([nb * nb for nb in orders])])[:-1]
        lib.run("dense_invert_all", len(orders), i32(orders), i64(boff), buf, len(flat), words(buf), max(orders), flag)
    return {"flat": buf, "flag": flag}


def inv_check(case, inp, out):
    fails, worst, off = [], 0.0, 0
    singular = "singular" in inp["kinds"]
    if bool(out["flag"][0]) != singular:
        fails.append("flag %d" % out["flag"][0])
    for q, (nb, B) in enumerate(zip(case.p["orders"], inp["blocks"])):
        X = out["flat"][off:off + nb * nb].reshape(nb, nb).T
        off += nb * nb
        if inp["kinds"][q] == "singular":
            continue
        ref, cond = np.linalg.inv(B), np.linalg.cond(B)
        if not np.all(np.isfinite(X)):
            fails.append("block %d (order %d): not finite" % (q, nb))
            continue
        r1 = np.abs(X - ref).max() / (1e-13 * cond * np.abs(ref).max())
        r2 = np.abs(X @ B - np.eye(nb)).max() / (1e-13 * cond)
        worst = max(worst, r1, r2)
        if r1 > 1 or r2 > 1:
            fails.append("block %d (order %d, %s): |X - inv| at %.3g, |X A - I| at %.3g of the bound" % (q, nb, inp["kinds"][q], r1, r2))
    if not untouched(out["flat"], np.ones(off, bool)):
        fails.append("written behind the blocks")
    return fails, float(worst)


# ---- blocks_apply / blocks_apply_all / blocks_apply_all_mv
BA_TABLES = {
    # (order, r0) per descriptor; r0 < 0: all rows
    "mixed": [(1, -1), (7, -1), (8, -1), (9, -1), (63, -1), (64, -1), (65, -1)],
    "tiles130": [(130, 0), (130, 64), (130, 128)],                      # one block of order 130 as three row tiles
    "tile_alone": [(130, 64)],
}


def ba_inputs(case):
    rng = case.rng()
    if case.family == "blocks_apply":
        nb, nblk = case.p["nb"], 2
        n = nb * nblk + 37
        return {"binv": rng.uniform(-1, 1, (nblk, nb, nb)), "ids": i32(rng.permutation(n)[:nb * nblk].reshape(nblk, nb)), "n": n,
                "x": rng.uniform(-1, 1, n)}
    table = BA_TABLES[case.p["table"]]
    blocks, ids, tiles = [], [], []
    shared = len({nb for nb, _ in table}) == 1 and len(table) > 1      # the tiles of one block share its entries and ids
    total = table[0][0] if shared or len(table) == 1 else sum(nb for nb, _ in table)
    n = total + 41
    perm = rng.permutation(n)[:total]                                   # a random injection into a longer vector
    off = 0
    for k, (nb, r0) in enumerate(table):
        if k == 0 or not shared:
            blocks.append(rng.uniform(-1, 1, (nb, nb)))
            ids.append(perm[off:off + nb])
            off += nb
        tiles.append((len(blocks) - 1, nb, r0))
    nv = max(case.p.get("nv", 1), 1)
    return {"blocks": blocks, "ids": ids, "tiles": tiles, "n": n, "x": rng.uniform(-1, 1, (nv, n))}


def ba_run(lib, case, inp):
    if case.family == "blocks_apply":
        nb, y = case.p["nb"], lib.out(inp["n"])
        lib.run("blocks_apply", nb, 2, np.ascontiguousarray(inp["binv"].transpose(0, 2, 1)), inp["ids"], inp["x"], inp["n"], y, words(y))
        return {"y": y}
    flat = np.concatenate([B.T.ravel() for B in inp["blocks"]])
    boffs = np.concatenate([[0], np.cumsum([B.size for B in inp["blocks"]])])
    ioffs = np.concatenate([[0], np.cumsum([len(i) for i in inp["ids"]])])
    ids = i32(np.concatenate(inp["ids"]))
    nbs, r0s = i32([nb for _, nb, _ in inp["tiles"]]), i32([r0 for _, _, r0 in inp["tiles"]])
    boff, ioff = i64([boffs[b] for b, _, _ in inp["tiles"]]), i64([ioffs[b] for b, _, _ in inp["tiles"]])
    n, nv, max_nb = inp["n"], case.p.get("nv", 0), int(nbs.max())
    if nv == 0:
        y = lib.out(n)
        lib.run("blocks_apply_all", len(nbs), nbs, r0s, boff, ioff, flat, len(flat), ids, len(ids), max_nb, inp["x"][0].copy(), n, y, words(y))
        return {"y": y}
    ldx, ldy = n + 5, n + 3
    x = np.zeros((nv, ldx))
    x[:, :n] = inp["x"]
    y = lib.out(nv * ldy)
    lib.run("blocks_apply_all_mv", len(nbs), nbs, r0s, boff, ioff, flat, len(flat), ids, len(ids), max_nb, x, ldx, y, ldy, nv, words(y))
    return {"y": y}


def ba_check(case, inp, out):
    fails, n = [], inp["n"]
    if case.family == "blocks_apply":
        nv, ldy = 1, n
        tiles = [(b, case.p["nb"], -1) for b in range(2)]
        blocks, ids, xs = list(inp["binv"]), list(inp["ids"]), inp["x"][None, :]
    else:
        nv = max(case.p.get("nv", 0), 1)
        ldy = n + 3 if case.p.get("nv", 0) else n
        tiles, blocks, ids, xs = inp["tiles"], inp["blocks"], inp["ids"], inp["x"]
    ref, bound = np.zeros((nv, ldy), LD), np.zeros((nv, ldy))
    defined = np.zeros((nv, ldy), bool)
    for b, nb, r0 in tiles:
        rows = slice(0, nb) if r0 < 0 else slice(r0, min(nb, r0 + 64))
        M = blocks[b][rows].astype(LD)
        for v in range(nv):
            xv = xs[v][ids[b]].astype(LD)
            ref[v, ids[b][rows]] = M @ xv
            bound[v, ids[b][rows]] = 2 * nb * EPS * (np.abs(M) @ np.abs(xv)).astype(np.float64)
            defined[v, ids[b][rows]] = True
    got = out["y"][:nv * ldy].reshape(nv, ldy)
    worst = _bounded("y", got[defined], ref[defined], bound[defined], fails)
    if not untouched(out["y"], defined.ravel()):
        fails.append("y written outside the rows of the descriptors")
    return fails, worst


# ---- one row tile of a block of order 8200: 65600 bytes of dynamic LDS for the gathered x
BIG_NB, BIG_R0 = 8200, 8192


def big_inputs(case):
    rng = case.rng()
    nv = max(case.p["nv"], 1)
    return {"rows": rng.uniform(-1, 1, (BIG_NB - BIG_R0, BIG_NB)), "x": rng.uniform(-1, 1, (nv, BIG_NB))}


def big_run(lib, case, inp):
    nv = case.p["nv"]
    y = lib.out(max(nv, 1) * BIG_NB)
    lib.run("blocks_apply_tile", BIG_NB, BIG_R0, BIG_NB - BIG_R0, inp["rows"], inp["x"], BIG_NB, y, BIG_NB, nv, words(y))
    return {"y": y}


def big_check(case, inp, out):
    fails, nv = [], max(case.p["nv"], 1)
    M = inp["rows"].astype(LD)
    ref = np.stack([M @ inp["x"][v].astype(LD) for v in range(nv)])
    bound = np.stack([2 * BIG_NB * EPS * (np.abs(M) @ np.abs(inp["x"][v]).astype(LD)).astype(np.float64) for v in range(nv)])
    got = out["y"][:nv * BIG_NB].reshape(nv, BIG_NB)
    worst = _bounded("y", got[:, BIG_R0:], ref, bound, fails)
    defined = np.zeros((nv, BIG_NB), bool)
    defined[:, BIG_R0:] = True
    if not untouched(out["y"], defined.ravel()):
        fails.append("y written outside the rows of the tile")
    return fails, worst


FAMILIES = {
    "gather_scatter": (gs_inputs, gs_run, gs_check), "pull_sum": (ps_inputs, ps_run, ps_check),
    "pull_sum_blocks": (psb_inputs, psb_run, psb_check), "build_pull_tables": (bpt_inputs, bpt_run, bpt_check),
    "member_sources": (ms_inputs, ms_run, ms_check), "offdiag": (od_inputs, od_run, od_check), "spmv": (spmv_inputs, spmv_run, spmv_check),
    "dot": (dot_inputs, dot_run, dot_check), "ot_apply": (ot_inputs, ot_run, ot_check), "householder": (hh_inputs, hh_run, hh_check),
    "invert": (inv_inputs, inv_run, inv_check), "blocks_apply": (ba_inputs, ba_run, ba_check),
    "blocks_apply_all": (ba_inputs, ba_run, ba_check), "blocks_apply_all_mv": (ba_inputs, ba_run, ba_check),
    "blocks_apply_big": (big_inputs, big_run, big_check),
}
EXACT_FAMILIES = {"gather_scatter", "pull_sum", "pull_sum_blocks", "build_pull_tables", "member_sources", "offdiag"}

# ------------------------------------------------------------------ the cases
MV_VARIANTS = ("default", "mv_group_1", "mv_group_2")
CASES = (
    [Case("gs_" + op, "gather_scatter", op=op) for op in ("gather", "scatter", "scatter_add")] +
    [Case("pull_sum", "pull_sum")] +
    [Case("pull_sum_blocks_%d" % b, "pull_sum_blocks", blen=b) for b in (1, 255, 257, 16389)] +
    [Case("pull_tables_runs", "build_pull_tables", rows=[[1, 5, 1], [], [5, 1]], big=(2, 3)),
     Case("pull_tables_one_row", "build_pull_tables", rows=[[5, 1, 1]])] +
    [Case("member_sources", "member_sources")] +
    [Case("offdiag_tb", "offdiag", tb=True), Case("offdiag_no_tb", "offdiag", tb=False)] +
    [Case("spmv_%d_L%d" % (n, L), "spmv", nrows=n, lanes=L) for n in (1, 63, 65, 257) for L in (1, 2, 4, 8, 0)] +
    [Case("dot_%d" % n, "dot", n=n) for n in (1, 255, 256, 257, 262147)] +
    [Case("ot_%d" % ng, "ot_apply", ng=ng) for ng in (1, 31, 32, 33, 65)] +
    [Case("hh_%s_nbc%d" % (s, nbc), "householder", shape=s, nbc=nbc) for s in HH_SHAPES for nbc in (1, 3)] +
    [Case("invert_all_a", "invert", orders=[1, 2, 16, 17, 88]),
     Case("invert_all_b", "invert", orders=[3, 88, 89, 100, 159]),
     Case("invert_all_c", "invert", variants=("blocked_min",), orders=[5, 89, 257, 300]),
     Case("invert_all_small", "invert", orders=[2, 40, 17]),               # the LDS launch sized by max_nb itself
     Case("invert_all_singular", "invert", orders=[17, 40, 100, 40, 17], kinds=["dominant", "random", "singular", "zero_diag", "tridiag"]),
     Case("invert_257", "invert", variants=("blocked_min",), orders=[257] * 3, uniform=True, kinds=["dominant", "zero_diag", "tridiag"]),
     Case("invert_300", "invert", variants=("blocked_min",), orders=[300] * 3, uniform=True, kinds=["dominant", "zero_diag", "tridiag"])] +
    [Case("apply_%d" % nb, "blocks_apply", nb=nb) for nb in (1, 64, 65, 128, 129, 257)] +
    [Case("apply_all_" + t, "blocks_apply_all", table=t) for t in BA_TABLES] +
    [Case("apply_mv%d_%s" % (nv, t), "blocks_apply_all_mv", variants=MV_VARIANTS, table=t, nv=nv) for t in BA_TABLES for nv in (1, 2, 3, 4, 5, 7)] +
    [Case("apply_big_tile", "blocks_apply_big", sim=False, nv=0), Case("apply_big_tile_mv2", "blocks_apply_big", sim=False, nv=2)]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases_of(variant):
    return [c for c in CASES if variant in c.variants]


# ------------------------------------------------------------------ coverage
def mv_groups(nv, max_nb, cap):
    """The column groups blocks_apply_all_mv walks through (device_hip.hip)."""
    v, out = 0, []
    while v < nv:
        g = 4 if nv - v >= 4 else (2 if nv - v >= 2 else 1)
        while g > 1 and (max_nb * g * 8 > 64 * 1024 or g > cap):
            g >>= 1
        out.append(g)
        v += g
    return out


def coverage(lib, cases, env=None):
    """The branch tags the cases reach, from their shapes and the route predicates the harness exports."""
    env = os.environ if env is None else env
    cap = max(1, int(env.get("HYMLS_MI_MV_GROUP_BLK", "4")))
    tags = set()
    for c in cases:
        inp, p = inputs(c), c.p
        if c.family == "gather_scatter":
            tags.add(p["op"])
            if p["op"] == "scatter_add" and len(set(inp["idx"])) < len(inp["idx"]):
                tags.add("scatter_add_repeated")
        elif c.family == "pull_sum":
            lens = set(np.diff(inp["ptr"]))
            tags |= {"pull_sum_len=%d" % n for n in lens}
        elif c.family == "pull_sum_blocks":
            tags.add("pull_blocks_empty_range")
            tags.add("pull_blocks_tail" if p["blen"] > 64 * 256 else ("pull_blocks_partial" if p["blen"] % 256 else "pull_blocks_full"))
        elif c.family == "build_pull_tables":
            runs = {n for r in p["rows"] for n in r}
            tags |= {"pull_tables_run=%d" % n for n in runs}
            if np.any((inp["keys"] & np.uint64((1 << 33) - 1)) >= np.uint64(1 << 32)):
                tags.add("pull_tables_bit32")
            if len(p["rows"]) == 1:
                tags.add("pull_tables_one_row")
            if [] in p["rows"]:
                tags.add("pull_tables_empty_row")
        elif c.family == "member_sources":
            want, missing = ms_reference(inp)
            r = inp["ext"][0][inp["er"]]
            if MS["nent"] > 64 * 256:
                tags.add("member_sources_tail")
            if np.any(want[0] == inp["krow"][r]):
                tags.add("member_sources_first")
            if np.any(want[0] == inp["krow"][r + 1] - 1):
                tags.add("member_sources_last")
            if missing:
                tags.add("member_sources_missing")
        elif c.family == "offdiag":
            tags.add("offdiag_tb" if p["tb"] else "offdiag_no_tb")
            count = od_reference(c, inp)[0]
            if 0 in count:
                tags.add("offdiag_empty_row")
            if p["tb"] and np.any((inp["ta"] < 0) & (inp["excl"] >= 0) & (inp["tb"] >= 0)):
                tags.add("offdiag_excluded")
        elif c.family == "spmv":
            tags.add("spmv_L=%d" % lib.spmv_lanes(p["nrows"], spmv_hint(c, inp)))
            if p["lanes"] == 0:
                tags.add("spmv_no_hint")
            L = lib.spmv_lanes(p["nrows"], spmv_hint(c, inp))
            if p["nrows"] % (256 // L):
                tags.add("spmv_partial_block")
            lens = set(np.diff(inp["rp"]))
            if 0 in lens:
                tags.add("spmv_empty_row")
            if any(n % 8 for n in lens if n > 8):
                tags.add("spmv_row_tail")
        elif c.family == "dot":
            n = p["n"]
            tags.add("dot_tail" if n > 1024 * 256 else ("dot_partial" if n % 256 else "dot_full"))
        elif c.family == "ot_apply":
            sizes = np.diff(inp["gptr"])
            tags |= {"ot_size<8" if n < 8 else ("ot_size=8" if n == 8 else "ot_size>8") for n in sizes}
            tags.add("ot_ng%%32=%d" % min(p["ng"] % 32, 2))
            if p["ng"] > 32:
                tags.add("ot_blocks>1")
            if any(not np.any(inp["w"][a:b]) for a, b in zip(inp["gptr"][:-1], inp["gptr"][1:])):
                tags.add("ot_w=0")
        elif c.family == "householder":
            sizes, linked = inp["sizes"], inp["linked"]
            nS, ngl = sum(sizes), len(sizes)
            tags |= {"hh_" + HH_KINDS[k] for k in np.unique(inp["kinds"])}
            tags |= {"hh_size<8" if n < 8 else ("hh_size=8" if n == 8 else "hh_size>8") for n in sizes}
            if (ngl * nS) % 32:
                tags.add("hh_rows_partial_block")
            if nS > 256:
                tags.add("kept_nS>256")
            if ngl > 256:
                tags.add("kept_ngl>256")
            tags |= {"kept_nJ=%d" % n for n in sizes if n <= 5}
            tags |= {"kept_nJ%%4=%d" % (n % 4) for n in sizes if n > 5}
            in_set = {g for L in linked for g in L}
            if len(in_set) < ngl:
                tags.add("kept_unlinked")
            for L in linked:
                n = [sizes[g] for g in L]
                if sum(n) == len(n):
                    tags.add("kept_blk_len=0")
                elif len(L) == 1:
                    tags.add("kept_set_of_one")
                else:
                    tags.add("kept_set_of_many")
                    if len(L) >= 3 and 1 in n[1:-1]:
                        tags.add("kept_one_node_in_the_middle")
                    if sum(1 for k in n if k >= 2) >= 2:
                        tags.add("kept_c0_reused")
                    if max((a - 1) * (b - 1) for a in n for b in n) > 256:
                        tags.add("kept_block>256")
            tags.add("kept_stride>record")
            tags.add("kept_nbc=%d" % p["nbc"])
            if lib.kept_fits(nS, ngl):
                tags.add("kept_fits")
        elif c.family == "invert":
            orders = p["orders"]
            tags |= {"invert_" + k for k in inp["kinds"]}
            if p.get("uniform"):
                if not lib.blocked_order(orders[0]):
                    tags.add("invert<1024,false>" if orders[0] > 256 else ("invert<256,false>" if orders[0] > GJ_LDS_NB else "invert<256,true>"))
            else:
                small, large = [n for n in orders if n <= GJ_LDS_NB], [n for n in orders if n > GJ_LDS_NB]
                if small:
                    tags.add("invert_all_lds")
                    tags.add("invert_all_lds_sized_by_%s" % ("88" if max(orders) >= GJ_LDS_NB else "max_nb"))
                if large:
                    tags.add("invert_all<1024,false>" if max(orders) > 256 else "invert_all<256,false>")
                if small and large:
                    tags.add("invert_all_both_launches")
        elif c.family == "blocks_apply":
            tags.add("apply_bs=%d" % (64 if p["nb"] <= 64 else (128 if p["nb"] <= 128 else 256)))
            tags.add("apply_nb%%2=%d" % (p["nb"] % 2))
            if p["nb"] > 256:
                tags.add("apply_strided")
        elif c.family in ("blocks_apply_all", "blocks_apply_all_mv"):
            pre = "apply_all_" if c.family == "blocks_apply_all" else "apply_mv_"
            max_nb = max(nb for _, nb, _ in inp["tiles"])
            for _, nb, r0 in inp["tiles"]:
                tags.add(pre + ("nb<8" if nb < 8 else ("nb%%8=%d" % min(nb % 8, 2))))
                if r0 >= 0:
                    tags.add(pre + ("partial_tile" if r0 + 64 > nb else "full_tile"))
                if nb < max_nb:
                    tags.add(pre + "XS>nb")
            if len(inp["tiles"]) == 1 and inp["tiles"][0][2] >= 0:
                tags.add(pre + "tile_alone")
            if c.family == "blocks_apply_all_mv":
                tags.add("apply_mv_ldx!=ldy")
                tags |= {"apply_mv_group=%d" % g for g in mv_groups(p["nv"], max_nb, cap)}
                tags.add("apply_mv_nv=%d" % p["nv"])
        elif c.family == "blocks_apply_big":
            tags.add("apply_lds>64KiB" if BIG_NB * 8 > 64 * 1024 else "apply_lds<=64KiB")
            if p["nv"]:
                tags.add("apply_mv_halved_to_1")
    return tags


# the branches listed in the lab's design notes, by kernel
REQUIRED_SIM = (
    # k_ot, k_sblock_hh_rows: 1-7, 8, 9+ nodes; ng and ng * nS no multiple of 32; w = 0
    {"ot_size<8", "ot_size=8", "ot_size>8", "ot_ng%32=0", "ot_ng%32=1", "ot_ng%32=2", "ot_blocks>1", "ot_w=0",
     "hh_size<8", "hh_size=8", "hh_size>8", "hh_rows_partial_block"} |
    # hh_setup: identity cases and a negative leading entry
    {"hh_" + k for k in HH_KINDS} |
    # k_sblock_kept
    {"kept_nS>256", "kept_ngl>256", "kept_nJ=1", "kept_nJ=2", "kept_nJ=3", "kept_nJ=4", "kept_nJ=5", "kept_nJ%4=0", "kept_nJ%4=1",
     "kept_nJ%4=2", "kept_set_of_one", "kept_set_of_many", "kept_one_node_in_the_middle", "kept_unlinked", "kept_block>256",
     "kept_c0_reused", "kept_blk_len=0", "kept_stride>record", "kept_nbc=1", "kept_nbc=3", "kept_fits"} |
    # k_dense_invert through dense_invert_all
    {"invert_all_lds", "invert_all_lds_sized_by_88", "invert_all_lds_sized_by_max_nb", "invert_all<256,false>", "invert_all<1024,false>",
     "invert_all_both_launches", "invert_zero_diag", "invert_tridiag", "invert_singular"} |
    # k_blocks_apply*, rows and columns
    {"apply_all_nb<8", "apply_all_nb%8=0", "apply_all_nb%8=1", "apply_all_nb%8=2", "apply_all_partial_tile", "apply_all_full_tile",
     "apply_all_tile_alone", "apply_all_XS>nb", "apply_mv_nb<8", "apply_mv_nb%8=0", "apply_mv_nb%8=1", "apply_mv_partial_tile",
     "apply_mv_tile_alone", "apply_mv_XS>nb", "apply_mv_ldx!=ldy", "apply_mv_nv=3", "apply_mv_nv=5", "apply_mv_nv=7",
     "apply_bs=64", "apply_bs=128", "apply_bs=256", "apply_nb%2=0", "apply_nb%2=1", "apply_strided"} |
    # k_spmv
    {"spmv_no_hint", "spmv_empty_row", "spmv_row_tail", "spmv_partial_block"} |
    # sums and tables
    {"pull_sum_len=0", "pull_sum_len=1", "pull_sum_len=1000", "pull_blocks_empty_range", "pull_blocks_tail", "pull_blocks_partial",
     "scatter_add_repeated", "dot_tail", "dot_partial", "dot_full", "pull_tables_run=1", "pull_tables_run=5", "pull_tables_bit32",
     "pull_tables_one_row", "member_sources_tail", "member_sources_first", "member_sources_last", "member_sources_missing",
     "offdiag_tb", "offdiag_no_tb", "offdiag_empty_row", "offdiag_excluded"})
# what only the product library can reach: the lane counts, the column groups, the 1024-thread scalar inversion, the raised
# LDS limit
REQUIRED_GPU = {
    "default": REQUIRED_SIM - {"invert_all<1024,false>"} | {"spmv_L=1", "spmv_L=2", "spmv_L=4", "spmv_L=8", "apply_mv_group=4", "apply_mv_group=2",
                                                           "apply_mv_group=1", "apply_lds>64KiB", "apply_mv_halved_to_1"},
    "blocked_min": {"invert<1024,false>", "invert_all<1024,false>", "invert_all_both_launches"},
    "mv_group_1": {"apply_mv_group=1"},
    "mv_group_2": {"apply_mv_group=2", "apply_mv_group=1"},
}
