"""Kernel lab of the Krylov layer: the vector, reduction and update launchers of krylov.hpp one by one, their batched
(lock-step) forms, and the multi-vector SpMV of device.hpp.  This module holds the case list, the inputs, the ctypes driver
of the harness (kry_harness.cpp), the numpy references, the checks and the coverage bookkeeping.

The harness is linked twice.  Against the test-only simulators a batched launcher is a loop over the single launcher and
spmv_mv a loop over spmv, so the simulator run proves the harness, the references, the canaries, the bounds and the
coverage bookkeeping on a machine without a GPU; it does not test the batched kernels.  The run through the product
library (tests/test_krylab_gpu.py) pins the kernels.

The references restate the OPERATION in numpy (np.longdouble where a bound applies); none is derived from a simulator or
from a kernel.

The bound rule, stated once:  an output that is a sum of m terms (a product counts as one term) satisfies
    |got - ref| <= 2 m eps sum|terms|,   eps = 2^-53,
for ANY order of the sum and with or without contracted multiply-adds (the textbook bound m eps sum|terms| to first order;
the factor 2 is the only margin).  m per output:
  cg_p, and x and r of cg_xr    2           (z + beta p;  x + alpha p;  r - alpha q)
  update                        k + 1       (x + sum_j V_j y_j)
  dot                           n
  r.r of cg_xr                  n, against the extended-precision sum of squares of the r THE LAUNCHER RETURNED: this
                                isolates the reduction from the element-wise step, which has its own check
  spmv_mv                       per column, the spmv bound of tests/seplab: 2 (len |alpha| eps sum|a x| + eps |beta y|)
Exact outputs: sub, add, div, scale_by, widen, round_div and round_scale_by round once per output and must equal numpy's
float64 / float32 arithmetic bit for bit (FP64 division is correctly rounded on both sides; round_div is
(x / s).astype(float32)).  Where the device scalar is not > 0, scale_by leaves x untouched and round_scale_by writes
(float) x.
Batched launches: column c must equal, bit for bit, what the single launcher of the same library gives on column c's
operands (compared through SHA-256 digests taken in the same process), and must pass the reference check itself.
Canaries: every output buffer -- KryWork::part and KryWork::out included -- comes back whole; nothing outside the defined
output set (nb partials and out[0] of a reduction, the n entries of a column) may have lost the canary pattern.
"""
import ctypes
import hashlib
import os
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"sim": os.path.join(HERE, "libkrylab_sim.so"), "gpu": os.path.join(HERE, "libkrylab_gpu.so")}

EPS = 2.0 ** -53
LD = np.longdouble
CANARY = 0x7ff4dead5eed5eed

N_LIST = [0, 1, 255, 256, 257, 65281, 65537, 524288, 524289, 1048579]
AB = [0.75, -1.25, 0.0]                         # alpha of cg_xr, beta of cg_p
D_CLASSES = {"pos": 1.7320508, "+0": 0.0, "-0": -0.0, "neg": -1.7320508, "nan": float("nan")}
MV_N = [1, 257, 65537, 524289]
MV_S = [0.75, -1.25, 0.0, 1.5]                  # host scalar of column c
MV_D = [1.3, 1.67, 2.04, 2.41]                  # device scalar of column c
UPD_K = [1, 2, 7, 8, 9, 256]
UPD_N = [1, 257, 4099]
SPMV_AB = [(1.0, 0.0), (-1.0, 1.0), (2.5, -0.5)]      # as tests/seplab
# Row lengths: the seplab bound charges len roundings to the row, but alpha * s and the last add cost two more, so it is a
# proof only where len + 2 <= 2 len; the rows here are empty or have at least 3 entries (an empty row gives alpha * 0 + beta y,
# which the second term covers)
SPMV_LENS = [0, 3, 5, 33, 100]
SPMV_LONG = 300


class Case:
    def __init__(self, name, family, **params):
        self.name, self.family, self.p = name, family, params

    def rng(self, salt=0):
        return np.random.default_rng(zlib.crc32(self.name.encode()) + salt)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------ the harness
def build(which):
    subprocess.check_call(["make", "-s", "-j8", "-C", HERE, which])
    return LIBS[which]


_MV_SIG = "qipqpqpqqpqqpppqpqp"
_SIGS = {
    "sub": "qpppq", "add": "qppq", "div": "qpdpq", "scale_by": "qpqp", "widen": "qppq", "round_div": "qpdpq",
    "round_scale_by": "qpppq", "dot": "qpppqpq", "cg_xr": "qdpppqpqpqpq", "cg_p": "qdppq", "update_f64": "qipqppq",
    "update_f32": "qipqppq", "scale_by_mv": _MV_SIG, "round_scale_by_mv": _MV_SIG, "widen_mv": _MV_SIG, "dot_mv": _MV_SIG,
    "cg_xr_mv": _MV_SIG, "cg_p_mv": _MV_SIG, "spmv": "ippppqpqqddq", "spmv_mv": "ippppqqpqqqiddq",
}
_CT = {"q": ctypes.c_int64, "i": ctypes.c_int32, "p": ctypes.c_void_p, "d": ctypes.c_double}
_loaded = {}


class Lib:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name, sig in _SIGS.items():
            f = getattr(self.lib, "krylab_" + name)
            f.argtypes = [_CT[c] for c in sig] + [ctypes.c_char_p, ctypes.c_int32]
            f.restype = ctypes.c_int
        self.lib.krylab_row_grid.argtypes, self.lib.krylab_row_grid.restype = [ctypes.c_int64], ctypes.c_int32
        self.lib.krylab_spmv_lanes.argtypes, self.lib.krylab_spmv_lanes.restype = [ctypes.c_int32, ctypes.c_int64], ctypes.c_int32
        self.lib.krylab_guard_words.restype = ctypes.c_int64
        self.guard = int(self.lib.krylab_guard_words())
        self.maxgrid, self.kmax, self.lockstep_max = (int(self.lib.krylab_maxgrid()), int(self.lib.krylab_kmax()),
                                                      int(self.lib.krylab_lockstep_max()))

    def call(self, name, *args):
        """Returns (code, message); arrays are passed by pointer and must be contiguous."""
        assert len(args) == len(_SIGS[name]), name
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
        err = ctypes.create_string_buffer(512)
        code = getattr(self.lib, "krylab_" + name)(*conv, err, 512)
        return code, err.value.decode(errors="replace")

    def run(self, name, *args):
        code, msg = self.call(name, *args)
        if code != 0:
            raise RuntimeError("krylab_%s: error %d: %s" % (name, code, msg))

    def row_grid(self, n):
        """kry_row_grid of krylov.hpp."""
        return int(self.lib.krylab_row_grid(n))

    def vec_grid(self, n):
        """The vec_grid formula of krylov_hip.hip, from the product's KRY_MAXGRID."""
        return max(1, min((n + 255) // 256, self.maxgrid))

    def spmv_lanes(self, nrows, hint):
        return int(self.lib.krylab_spmv_lanes(nrows, hint))

    def out(self, n, dtype=np.float64, init=None):
        """Host side of an output buffer: n payload elements and the guard tail, everything canary except the initial
        content (the harness fills the device buffer the same way behind the bytes it is told to take from here)."""
        item = np.dtype(dtype).itemsize
        words = (n * item + 7) // 8 + self.guard
        a = np.full(words, CANARY, dtype=np.uint64).view(dtype)
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
    """True where every element outside `defined` (boolean mask over the front of the buffer; the guard tail is never
    defined) still holds the canary bits."""
    raw = np.uint64 if buf.dtype.itemsize == 8 else np.uint32
    want = np.full(buf.nbytes // 8, CANARY, dtype=np.uint64).view(raw)
    same = buf.view(raw) == want
    mask = np.zeros(buf.size, dtype=bool)
    mask[:len(defined)] = defined
    return bool(np.all(same[~mask]))


def all_written(buf):
    """No element of buf holds the canary bits."""
    if buf.dtype.itemsize == 8:
        return not np.any(buf.view(np.uint64) == np.uint64(CANARY))
    return True


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ------------------------------------------------------------------ checks shared by the single and the batched families
def _exact(name, got, want, fails):
    want = np.asarray(want, dtype=got.dtype)
    if not same_bits(np.asarray(got), want):
        raw = np.uint64 if got.dtype.itemsize == 8 else np.uint32
        bad = np.flatnonzero(np.ascontiguousarray(got).view(raw) != np.ascontiguousarray(want).view(raw))
        fails.append("%s differs from the restatement at %d positions (first %s)" % (name, bad.size, bad[:3]))


def _bounded(name, got, ref, bound, fails):
    """|got - ref| <= bound elementwise (ref longdouble); returns the largest error / bound."""
    got = np.atleast_1d(np.asarray(got))
    if not np.all(np.isfinite(got)):
        fails.append("%s: not finite, above any bound" % name)
        return np.inf
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        k = int(np.argmax(ratio))
        fails.append("%s: error %.3g above the bound %.3g at %d" % (name, err.ravel()[k], bound.ravel()[k], k))
    return worst


def exact_want(op, a, b=None, s=None):
    """The one-rounding kernels in numpy's float64 / float32 arithmetic."""
    with np.errstate(all="ignore"):
        if op == "sub":
            return a - b
        if op == "add":
            return b + a                                   # y <- y + x
        if op == "div":
            return a / s
        if op == "scale_by":
            return a / s if s > 0 else a
        if op == "widen":
            return a.astype(np.float64)
        if op == "round_div":
            return (a / s).astype(np.float32)
        if op == "round_scale_by":
            return (a / s).astype(np.float32) if s > 0 else a.astype(np.float32)
    raise KeyError(op)


def chk_axpy(name, alpha, p, x0, x, fails):
    """x = x0 + alpha p, a sum of two terms."""
    t = LD(alpha) * p.astype(LD)
    return _bounded(name, x, x0.astype(LD) + t, 2 * 2 * EPS * (np.abs(x0) + np.abs(t).astype(np.float64)), fails)


def chk_reduction(name, n, ref, sum_abs, part, out, fails, part_full=None, out_full=None):
    """out[0] against ref with m = n; the nb partials all written and consistent with out[0]; nothing else written."""
    nb = vec_grid(n)
    worst = _bounded(name, out[:1], np.array([ref], dtype=LD), [2 * n * EPS * float(sum_abs)], fails)
    if n == 0 and (out[0] != 0.0 or np.signbit(out[0])):
        fails.append("%s: n = 0 must give +0.0, got %r" % (name, out[0]))
    if not all_written(part[:nb]):
        fails.append("%s: fewer than %d partials written" % (name, nb))
    elif np.all(np.isfinite(part[:nb])):
        pl = part[:nb].astype(LD)
        _bounded(name + " (stage two over its partials)", out[:1], np.array([pl.sum()]), [2 * nb * EPS * float(np.abs(pl).sum())], fails)
    if part_full is not None and not untouched(part_full, np.arange(len(part_full)) < nb):
        fails.append("%s: written outside part[0:%d]" % (name, nb))
    if out_full is not None and not untouched(out_full, np.arange(len(out_full)) < 1):
        fails.append("%s: written outside out[0]" % name)
    return worst


MAXGRID = 2048          # KRY_MAXGRID of krylov.hpp; run_case() asserts that the library agrees


def vec_grid(n):
    """Workgroups (and stage-one partials) of a vector pass over n rows: the vec_grid formula of krylov_hip.hip."""
    return max(1, min((n + 255) // 256, MAXGRID))


def chk_dot(name, n, x, y, part, out, fails, part_full=None, out_full=None):
    prod = x.astype(LD) * y.astype(LD)
    return chk_reduction(name, n, prod.sum() if n else LD(0), np.abs(prod).sum() if n else 0.0, part, out, fails, part_full, out_full)


def chk_cg_xr(name, n, alpha, p, q, x0, r0, x, r, part, out, fails, part_full=None, out_full=None):
    worst = chk_axpy(name + " x", alpha, p, x0, x, fails)
    worst = max(worst, chk_axpy(name + " r", -alpha, q, r0, r, fails))
    rr = r.astype(LD) ** 2 if np.all(np.isfinite(r)) else np.zeros(n, LD)
    return max(worst, chk_reduction(name + " r.r", n, rr.sum() if n else LD(0), rr.sum() if n else 0.0, part, out, fails,
                                    part_full, out_full))


def chk_cg_p(name, beta, z, p0, p, fails):
    return chk_axpy(name, beta, p0, z, p, fails)


# ------------------------------------------------------------------ families
# Every family has inputs(case) -> dict (deterministic), run(lib, case, inp) -> dict of arrays (whole buffers) and
# check(case, inp, out) -> (list of failures, largest error / bound).
_inputs = {}


def inputs(case, keep=True):
    if case.name in _inputs:
        return _inputs[case.name]
    inp = FAMILIES[case.family][0](case)
    if keep and sum(v.nbytes for v in inp.values() if isinstance(v, np.ndarray)) < (1 << 20):
        _inputs[case.name] = inp
    return inp


def run_case(lib, case):
    assert lib.maxgrid == MAXGRID
    return FAMILIES[case.family][1](lib, case, inputs(case))


def check_case(case, out):
    return FAMILIES[case.family][2](case, inputs(case), out)


def vec(rng, n):
    return rng.uniform(-1.0, 1.0, n)


def crafted_quotients():
    """FP64 quotients whose rounding to float is not the everyday case (see the checks in ev_check)."""
    q = [1 + 2.0 ** -24,                    # exact tie between 1 and 1 + 2^-23: to even, 1
         1 + 3 * 2.0 ** -24,                # tie between 1 + 2^-23 and 1 + 2^-22: to even, 1 + 2^-22
         -(1 + 2.0 ** -24),
         2.0 ** -149, 1.5 * 2.0 ** -140, 2.0 ** -127, 1.25 * 2.0 ** -149,     # float subnormals
         2.0 ** -150,                       # tie between 0 and the smallest subnormal: 0
         3 * 2.0 ** -150,                   # tie between 2^-149 and 2^-148: 2^-148
         -0.0,                              # a negative zero
         -2.0 ** -151,                      # rounds to a negative zero
         2.0 ** -127 * (1 + 2.0 ** -23 + 2.0 ** -30)]    # times 2: float32(x) / float32(2) rounds twice and differs
    return np.array(q)


# ---- the element-wise kernels with one rounding per output
def ev_inputs(case):
    rng, n, op = case.rng(), case.p["n"], case.family
    inp = {}
    if op == "widen":
        a = vec(rng, n).astype(np.float32)
        if n >= 255:
            a[:6] = np.array([2.0 ** -149, -2.0 ** -140, -0.0, 2.0 ** -126, 3.4e38, -1.0], dtype=np.float32)
        return {"a": a}
    a = vec(rng, n)
    if op in ("sub", "add"):
        inp["b"] = vec(rng, n)
    if op in ("div", "round_div"):
        s = float(rng.uniform(1.1, 1.9))                # no power of two
        if case.p.get("crafted"):
            s = float(case.p["crafted"])
            q = crafted_quotients()
            a[:len(q)] = q * s                          # exact: s is 1 or 2
        inp["s"] = np.array([s])
    if op in ("scale_by", "round_scale_by"):
        s = D_CLASSES[case.p["d"]]
        if case.p.get("crafted"):
            s = float(case.p["crafted"])
            q = crafted_quotients()
            a[:len(q)] = q * s
        inp["s"] = np.array([s])
    inp["a"] = a
    return inp


def ev_run(lib, case, inp):
    n, op = case.p["n"], case.family
    if op == "sub":
        o = lib.out(n)
        lib.run("sub", n, inp["a"], inp["b"], o, words(o))
    elif op == "add":
        o = lib.out(n, init=inp["b"])
        lib.run("add", n, inp["a"], o, words(o))
    elif op == "div":
        o = lib.out(n)
        lib.run("div", n, inp["a"], float(inp["s"][0]), o, words(o))
    elif op == "scale_by":
        o = lib.out(n, init=inp["a"])
        lib.run("scale_by", n, o, words(o), inp["s"])
    elif op == "widen":
        o = lib.out(n)
        lib.run("widen", n, inp["a"], o, words(o))
    elif op == "round_div":
        o = lib.out(n, np.float32)
        lib.run("round_div", n, inp["a"], float(inp["s"][0]), o, words(o))
    else:
        o = lib.out(n, np.float32)
        lib.run("round_scale_by", n, inp["a"], inp["s"], o, words(o))
    return {"o": o}


def ev_check(case, inp, out):
    fails, n, op = [], case.p["n"], case.family
    s = float(inp["s"][0]) if "s" in inp else None
    want = exact_want(op, inp["a"], inp.get("b"), s)
    _exact(op, out["o"][:n], want, fails)
    if not untouched(out["o"], np.ones(n, bool)):
        fails.append("written behind the output")
    if case.p.get("crafted") and op in ("round_div", "round_scale_by"):
        # the crafted entries are what their comments say (a check of the test vector, not of the kernel)
        w = want[:12].astype(np.float64)
        assert w[0] == 1.0 and w[1] == 1 + 2.0 ** -22 and w[2] == -1.0 and w[3] == 2.0 ** -149 and w[7] == 0.0 and w[8] == 2.0 ** -148
        assert np.signbit(want[9]) and want[9] == 0 and np.signbit(want[10]) and want[10] == 0
    return fails, 0.0


# ---- dot
def dot_inputs(case):
    rng, n = case.rng(), case.p["n"]
    return {"x": vec(rng, n), "y": vec(rng, n)}


def dot_run(lib, case, inp):
    res = {}
    for rep in ("", "_again"):                           # two calls: the same bits
        part, out = lib.out(lib.maxgrid), lib.out(8)
        lib.run("dot", case.p["n"], inp["x"], inp["y"], part, words(part), out, words(out))
        res["part" + rep], res["out" + rep] = part, out
    return res


def dot_check(case, inp, out):
    fails = []
    worst = chk_dot("dot", case.p["n"], inp["x"], inp["y"], out["part"], out["out"], fails, out["part"], out["out"])
    if not (same_bits(out["part"], out["part_again"]) and same_bits(out["out"], out["out_again"])):
        fails.append("dot: two calls differ")
    return fails, worst


# ---- cg_xr, cg_p
def cg_inputs(case):
    rng, n = case.rng(), case.p["n"]
    if case.family == "cg_p":
        return {"z": vec(rng, n), "p": vec(rng, n)}
    return {"p": vec(rng, n), "q": vec(rng, n), "x": vec(rng, n), "r": vec(rng, n)}


def cg_run(lib, case, inp):
    n, res = case.p["n"], {}
    for k, ab in enumerate(AB):
        if case.family == "cg_p":
            p = lib.out(n, init=inp["p"])
            lib.run("cg_p", n, ab, inp["z"], p, words(p))
            res["p%d" % k] = p
            continue
        for rep in ("", "_again") if k == 0 else ("",):
            x, r, part, out = lib.out(n, init=inp["x"]), lib.out(n, init=inp["r"]), lib.out(lib.maxgrid), lib.out(8)
            lib.run("cg_xr", n, ab, inp["p"], inp["q"], x, words(x), r, words(r), part, words(part), out, words(out))
            if rep:
                res["same_again"] = np.array([same_bits(x, res["x0"]) and same_bits(r, res["r0"]) and same_bits(part, res["part0"]) and
                                              same_bits(out, res["out0"])])
            else:
                res["x%d" % k], res["r%d" % k], res["part%d" % k], res["out%d" % k] = x, r, part, out
    return res


def cg_check(case, inp, out):
    fails, worst, n = [], 0.0, case.p["n"]
    for k, ab in enumerate(AB):
        if case.family == "cg_p":
            worst = max(worst, chk_cg_p("p (beta %g)" % ab, ab, inp["z"], inp["p"], out["p%d" % k][:n], fails))
            if not untouched(out["p%d" % k], np.ones(n, bool)):
                fails.append("written behind p")
            continue
        x, r = out["x%d" % k], out["r%d" % k]
        worst = max(worst, chk_cg_xr("cg_xr (alpha %g)" % ab, n, ab, inp["p"], inp["q"], inp["x"], inp["r"], x[:n], r[:n],
                                     out["part%d" % k], out["out%d" % k], fails, out["part%d" % k], out["out%d" % k]))
        if not (untouched(x, np.ones(n, bool)) and untouched(r, np.ones(n, bool))):
            fails.append("written behind x or r")
    if case.family == "cg_xr" and not bool(out["same_again"][0]):
        fails.append("cg_xr: two calls differ")
    return fails, worst


# ---- update: x += V y in place
def upd_inputs(case):
    rng, n, k, ld = case.rng(), case.p["n"], case.p["k"], case.p["ld"]
    nV = (k - 1) * ld + n if k > 0 else 0
    V = vec(rng, nV)
    if case.p["f32"]:
        V = V.astype(np.float32)
    return {"V": V, "y": vec(rng, k), "x": vec(rng, n)}


def upd_run(lib, case, inp):
    n, k = case.p["n"], case.p["k"]
    x = lib.out(n, init=inp["x"])
    code, _ = lib.call("update_f32" if case.p["f32"] else "update_f64", n, k, inp["V"], case.p["ld"], inp["y"], x, words(x))
    return {"x": x, "code": np.array([code])}


def upd_columns(case, inp):
    n, k, ld = case.p["n"], case.p["k"], case.p["ld"]
    return np.stack([inp["V"][j * ld:j * ld + n] for j in range(k)]) if k else np.zeros((0, n))


def upd_check(case, inp, out):
    fails, n, k = [], case.p["n"], case.p["k"]
    x, code = out["x"], int(out["code"][0])
    if not untouched(x, np.ones(n, bool)):
        fails.append("written behind x")
    if k > 256:
        if code != -2:
            fails.append("k = %d: error %d instead of -2" % (k, code))
        if not same_bits(x[:n], inp["x"]):
            fails.append("k = %d: x changed" % k)
        return fails, 0.0
    if code != 0:
        return fails + ["error %d" % code], 0.0
    if k == 0:
        if not same_bits(x[:n], inp["x"]):
            fails.append("k = 0: x changed")
        return fails, 0.0
    terms = upd_columns(case, inp).astype(LD) * inp["y"].astype(LD)[:, None]
    ref = inp["x"].astype(LD) + terms.sum(axis=0)
    bound = 2 * (k + 1) * EPS * (np.abs(inp["x"]) + np.abs(terms).sum(axis=0).astype(np.float64))
    return fails, _bounded("x", x[:n], ref, bound, fails)


# ---- batched launchers
MV_OPS = ("scale_by_mv", "round_scale_by_mv", "widen_mv", "dot_mv", "cg_xr_mv", "cg_p_mv")
MV_PART_STRIDE, MV_OUT_STRIDE = MAXGRID + 3, 5


def mv_offsets(n, nb):
    """Element offsets of the columns of one flat array: the first column starts at element 1, the gap behind column c is
    2 + c elements, so odd and even starts (4-byte / 8-byte and 8-byte / 16-byte aligned) both occur."""
    off = [1]
    for c in range(1, 4):
        off.append(off[-1] + n + 1 + c)
    return i64(off), int(off[nb - 1] + n) if nb else 0


def mv_zero_col(case):
    """The column whose device scalar is 0 (scale kernels): one column, its neighbours positive; none when nb = 1."""
    nb = case.p["nb"]
    return None if not 2 <= nb <= 4 or case.family not in ("scale_by_mv", "round_scale_by_mv") else (1 if nb >= 3 else 0)


def mv_flat(cols, off, total, dtype=np.float64):
    a = np.full(total, np.nan, dtype=dtype)              # a read of a gap is a NaN in the result
    for c, v in enumerate(cols):
        a[off[c]:off[c] + len(v)] = v
    return a


def mv_inputs(case):
    rng, n, nb, op = case.rng(), case.p["n"], case.p["nb"], case.family
    cols = min(max(nb, 0), 4)
    inp = {"d": f64(MV_D[:cols]), "s": f64(MV_S)}
    z = mv_zero_col(case)
    if z is not None:
        inp["d"][z] = 0.0
    for key in {"scale_by_mv": "y", "round_scale_by_mv": "a", "widen_mv": "a", "dot_mv": "ab", "cg_xr_mv": "abyr", "cg_p_mv": "ay"}[op]:
        v = [vec(rng, n) for _ in range(cols)]
        if op == "widen_mv":
            v = [c.astype(np.float32) for c in v]
        inp[key] = np.stack(v) if cols else np.zeros((0, n))
    return inp


def mv_single(lib, case, inp, c):
    """The single launcher on column c's operands: the arrays it returns (payload only)."""
    n, op = case.p["n"], case.family
    if op == "scale_by_mv":
        o = lib.out(n, init=inp["y"][c])
        lib.run("scale_by", n, o, words(o), inp["d"][c:c + 1].copy())
        return {"y": o[:n]}
    if op == "round_scale_by_mv":
        o = lib.out(n, np.float32)
        lib.run("round_scale_by", n, inp["a"][c].copy(), inp["d"][c:c + 1].copy(), o, words(o))
        return {"y": o[:n]}
    if op == "widen_mv":
        o = lib.out(n)
        lib.run("widen", n, inp["a"][c].copy(), o, words(o))
        return {"y": o[:n]}
    if op == "dot_mv":
        part, out = lib.out(lib.maxgrid), lib.out(8)
        lib.run("dot", n, inp["a"][c].copy(), inp["b"][c].copy(), part, words(part), out, words(out))
        return {"p": part[:lib.vec_grid(n)], "o": out[:1]}
    if op == "cg_xr_mv":
        x, r, part, out = lib.out(n, init=inp["y"][c]), lib.out(n, init=inp["r"][c]), lib.out(lib.maxgrid), lib.out(8)
        lib.run("cg_xr", n, float(inp["s"][c]), inp["a"][c].copy(), inp["b"][c].copy(), x, words(x), r, words(r), part, words(part), out, words(out))
        return {"y": x[:n], "r": r[:n], "p": part[:lib.vec_grid(n)], "o": out[:1]}
    o = lib.out(n, init=inp["y"][c])
    lib.run("cg_p", n, float(inp["s"][c]), inp["a"][c].copy(), o, words(o))
    return {"y": o[:n]}


def mv_layout(case):
    n, nb, op = case.p["n"], case.p["nb"], case.family
    cols = min(max(nb, 0), 4)
    off, total = mv_offsets(n, cols)
    table = np.zeros((6, 4), np.int64)
    table[0], table[1], table[2], table[3] = off, off, off, off
    table[4] = np.arange(4) * MV_PART_STRIDE
    table[5] = np.arange(4) * MV_OUT_STRIDE
    return off, total, table


def mv_run(lib, case, inp):
    n, nb, op = case.p["n"], case.p["nb"], case.family
    cols = min(max(nb, 0), 4)
    off, total, table = mv_layout(case)
    a_type = np.float32 if op == "widen_mv" else np.float64
    y_type = np.float32 if op == "round_scale_by_mv" else np.float64
    A = mv_flat(inp["a"], off, total, a_type) if "a" in inp else None
    B = mv_flat(inp["b"], off, total) if "b" in inp else None
    Y = lib.out(total, y_type)
    y_init = 0
    if "y" in inp:                                       # in place: the columns, canary in the gaps
        for c in range(cols):
            Y[off[c]:off[c] + n] = inp["y"][c]
        y_init = total * 8
    R = r_init = None
    if "r" in inp:
        R = lib.out(total)
        for c in range(cols):
            R[off[c]:off[c] + n] = inp["r"][c]
        r_init = total * 8
    red = op in ("dot_mv", "cg_xr_mv")
    P = lib.out(4 * MV_PART_STRIDE) if red else None
    O = lib.out(4 * MV_OUT_STRIDE) if red else None
    code, msg = lib.call(op, n, nb, A, total, B, total if B is not None else 0, Y, y_init, words(Y), R, r_init or 0,
                         words(R) if R is not None else 0, inp["d"] if cols else None, inp["s"], P, words(P) if red else 0, O,
                         words(O) if red else 0, table)
    res = {"code": np.array([code]), "Y": Y}
    if R is not None:
        res["R"] = R
    if red:
        res["P"], res["O"] = P, O
    if code == 0:
        for c in range(cols):
            for key, arr in mv_single(lib, case, inp, c).items():
                res["single_%s%d" % (key, c)] = digest(arr)
    return res


def mv_check(case, inp, out):
    fails, worst = [], 0.0
    n, nb, op = case.p["n"], case.p["nb"], case.family
    code = int(out["code"][0])
    off, total, table = mv_layout(case)
    if nb < 1 or nb > 4:
        if code != -2:
            fails.append("nb = %d: error %d instead of -2" % (nb, code))
        for key, src in (("Y", "y"), ("R", "r"), ("P", None), ("O", None)):
            if key not in out:
                continue
            want = np.full(words(out[key]), CANARY, dtype=np.uint64).view(out[key].dtype)
            for c in range(min(max(nb, 0), 4) if src in inp else 0):
                want[off[c]:off[c] + n] = inp[src][c]
            if not same_bits(out[key], want):
                fails.append("nb = %d: %s was written" % (nb, key))
        return fails, 0.0
    if code != 0:
        return ["error %d" % code], 0.0
    nbk = vec_grid(n)
    defined = np.zeros(total, bool)
    for c in range(nb if op != "dot_mv" else 0):
        defined[off[c]:off[c] + n] = True
    if not untouched(out["Y"], defined) or ("R" in out and not untouched(out["R"], defined)):
        fails.append("written outside the columns (a gap between two columns or the tail)")
    if "P" in out:
        pdef, odef = np.zeros(4 * MV_PART_STRIDE, bool), np.zeros(4 * MV_OUT_STRIDE, bool)
        for c in range(nb):
            pdef[c * MV_PART_STRIDE:c * MV_PART_STRIDE + nbk] = True
            odef[c * MV_OUT_STRIDE] = True
        if not (untouched(out["P"], pdef) and untouched(out["O"], odef)):
            fails.append("written outside the %d partials or the result of a column" % nbk)
    for c in range(nb):
        y = out["Y"][off[c]:off[c] + n]
        got = {"y": y}
        if "R" in out:
            got["r"] = out["R"][off[c]:off[c] + n]
        if "P" in out:
            got["p"] = out["P"][c * MV_PART_STRIDE:c * MV_PART_STRIDE + nbk]
            got["o"] = out["O"][c * MV_OUT_STRIDE:c * MV_OUT_STRIDE + 1]
        if op == "dot_mv":
            del got["y"]
        for key, arr in got.items():
            if not same_bits(digest(arr), out["single_%s%d" % (key, c)]):
                fails.append("column %d: %s differs from the single launch" % (c, key))
        nm = "column %d" % c
        d, s = float(inp["d"][c]), float(inp["s"][c])
        if op == "scale_by_mv":
            _exact(nm, y, exact_want("scale_by", inp["y"][c], s=d), fails)
        elif op == "round_scale_by_mv":
            _exact(nm, y, exact_want("round_scale_by", inp["a"][c], s=d), fails)
        elif op == "widen_mv":
            _exact(nm, y, exact_want("widen", inp["a"][c]), fails)
        elif op == "dot_mv":
            worst = max(worst, chk_dot(nm, n, inp["a"][c], inp["b"][c], got["p"], got["o"], fails))
        elif op == "cg_xr_mv":
            worst = max(worst, chk_cg_xr(nm, n, s, inp["a"][c], inp["b"][c], inp["y"][c], inp["r"][c], y, got["r"], got["p"], got["o"], fails))
        else:
            worst = max(worst, chk_cg_p(nm, s, inp["a"][c], inp["y"][c], y, fails))
    return fails, worst


# ---- spmv_mv
def spmv_shape(case):
    nrows = case.p["nrows"]
    ncols = nrows + 11                                    # not square
    return nrows, ncols, ncols + 3, nrows + 5             # ldx != ldy


def spmv_inputs(case):
    rng, nv = case.rng(), case.p["nv"]
    nrows, ncols, ldx, ldy = spmv_shape(case)
    lens = np.array([SPMV_LENS[(i * 7 + i // 5) % 5] for i in range(nrows)])
    lens[nrows // 2] = SPMV_LONG                          # one long row
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = rng.integers(0, ncols, rp[-1])
    for i in range(nrows):
        if lens[i] >= 2:
            col[rp[i] + 1] = col[rp[i]]                   # a repeated column index in the row
    x = np.full((nv - 1) * ldx + ncols, np.nan)
    y = rng.uniform(-1, 1, (nv, nrows))
    for v in range(nv):
        x[v * ldx:v * ldx + ncols] = rng.uniform(-1, 1, ncols)
    return {"rp": i32(rp), "col": i32(col), "val": rng.uniform(-1, 1, rp[-1]), "x": x, "y": y}


def spmv_hint(case):
    """Chosen so that spmv_lanes gives case.p["lanes"] lanes per row (as the spmv cases of tests/seplab)."""
    return {1: 1, 2: 3, 4: 10, 8: 40}[case.p["lanes"]] * case.p["nrows"]


def spmv_run(lib, case, inp):
    nv, res = case.p["nv"], {}
    nrows, ncols, ldx, ldy = spmv_shape(case)
    hint = spmv_hint(case)
    for k, (alpha, beta) in enumerate(SPMV_AB):
        y0 = np.full((nv, nrows), np.nan) if beta == 0.0 else inp["y"]
        total = (nv - 1) * ldy + nrows
        Y = lib.out(total)
        for v in range(nv):
            Y[v * ldy:v * ldy + nrows] = y0[v]
        lib.run("spmv_mv", nrows, inp["rp"], inp["col"], inp["val"], inp["x"], len(inp["x"]), ldx, Y, total, words(Y), ldy, nv, alpha, beta, hint)
        res["y%d" % k] = Y
        single = []
        for v in range(nv):
            y1 = lib.out(nrows, init=y0[v])
            lib.run("spmv", nrows, inp["rp"], inp["col"], inp["val"], inp["x"][v * ldx:v * ldx + ncols].copy(), ncols, y1, nrows, words(y1),
                    alpha, beta, hint)
            single.append(digest(y1[:nrows]))
        res["single%d" % k] = np.stack(single)
    return res


def spmv_check(case, inp, out):
    fails, worst, nv, rp = [], 0.0, case.p["nv"], inp["rp"]
    nrows, ncols, ldx, ldy = spmv_shape(case)
    n = np.diff(rp)
    defined = np.zeros((nv - 1) * ldy + nrows, bool)
    for v in range(nv):
        defined[v * ldy:v * ldy + nrows] = True
    row = np.repeat(np.arange(nrows), n)
    for v in range(nv):
        prod = inp["val"].astype(LD) * inp["x"][v * ldx:v * ldx + ncols][inp["col"]].astype(LD)
        s, sa = np.zeros(nrows, LD), np.zeros(nrows, LD)
        np.add.at(s, row, prod)
        np.add.at(sa, row, np.abs(prod))
        for k, (alpha, beta) in enumerate(SPMV_AB):
            by = LD(beta) * inp["y"][v].astype(LD) if beta != 0.0 else np.zeros(nrows, LD)
            ref = LD(alpha) * s + by
            bound = 2 * (n * EPS * abs(alpha) * sa + EPS * np.abs(by))
            got = out["y%d" % k][v * ldy:v * ldy + nrows]
            worst = max(worst, _bounded("column %d (alpha %g, beta %g)" % (v, alpha, beta), got, ref, bound, fails))
            if not same_bits(digest(got), out["single%d" % k][v]):
                fails.append("column %d (alpha %g, beta %g) differs from spmv()" % (v, alpha, beta))
    for k in range(len(SPMV_AB)):
        if not untouched(out["y%d" % k], defined):
            fails.append("y written outside the columns (a gap between two columns or the tail)")
    return fails, worst


EXACT_OPS = ("sub", "add", "div", "scale_by", "widen", "round_div", "round_scale_by")
FAMILIES = {op: (ev_inputs, ev_run, ev_check) for op in EXACT_OPS}
FAMILIES.update({"dot": (dot_inputs, dot_run, dot_check), "cg_xr": (cg_inputs, cg_run, cg_check), "cg_p": (cg_inputs, cg_run, cg_check),
                 "update": (upd_inputs, upd_run, upd_check), "spmv_mv": (spmv_inputs, spmv_run, spmv_check)})
FAMILIES.update({op: (mv_inputs, mv_run, mv_check) for op in MV_OPS})
BOUNDED_FAMILIES = ("dot", "cg_xr", "cg_p", "update", "dot_mv", "cg_xr_mv", "cg_p_mv", "spmv_mv")
BITWISE_FAMILIES = EXACT_OPS + ("scale_by_mv", "round_scale_by_mv", "widen_mv")

# ------------------------------------------------------------------ the cases
CASES = (
    [Case("%s_%d" % (op, n), op, n=n) for op in ("sub", "add", "div", "widen", "round_div") for n in N_LIST] +
    [Case("%s_%d_pos" % (op, n), op, n=n, d="pos") for op in ("scale_by", "round_scale_by") for n in N_LIST] +
    [Case("%s_%d_%s" % (op, n, d), op, n=n, d=d) for op in ("scale_by", "round_scale_by") for n in (257, 65537) for d in D_CLASSES
     if d != "pos"] +
    [Case("round_div_crafted_s%d" % s, "round_div", n=257, crafted=s) for s in (1, 2)] +
    [Case("round_scale_by_crafted_s%d" % s, "round_scale_by", n=257, crafted=s, d="pos") for s in (1, 2)] +
    [Case("%s_%d" % (op, n), op, n=n) for op in ("dot", "cg_xr", "cg_p") for n in N_LIST] +
    [Case("update_%s_n%d_k%d_ld%d" % ("f32" if f32 else "f64", n, k, pad), "update", n=n, k=k, ld=n + pad, f32=f32)
     for f32 in (False, True) for n in UPD_N for k in UPD_K for pad in (0, 5)] +
    [Case("update_%s_n524289_k3" % ("f32" if f32 else "f64"), "update", n=524289, k=3, ld=524289, f32=f32) for f32 in (False, True)] +
    [Case("update_%s_n257_k%d" % ("f32" if f32 else "f64", k), "update", n=257, k=k, ld=262, f32=f32) for f32 in (False, True) for k in (0, 257)] +
    [Case("%s_n%d_nb%d" % (op, n, nb), op, n=n, nb=nb) for op in MV_OPS for n in MV_N for nb in (1, 2, 3, 4)] +
    [Case("%s_n257_nb%d" % (op, nb), op, n=257, nb=nb) for op in MV_OPS for nb in (0, 5)] +
    [Case("spmv_mv_%d_L%d_nv%d" % (n, L, nv), "spmv_mv", nrows=n, lanes=L, nv=nv) for n in (1, 63, 65, 257) for L in (1, 2, 4, 8)
     for nv in (1, 2, 3, 4, 5, 6, 7, 9)]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------ numpy restatements in float64 (and their mutants)
def block_partials(n, terms):
    """Stage one of a reduction: partial b holds the rows of the workgroups b, b + nb, ... (256 rows each)."""
    nb = vec_grid(n)
    part = np.zeros(nb)
    np.add.at(part, (np.arange(n) // 256) % nb, terms)
    return part


def restate_dot(case, out, mutant=None):
    """out with part / out[0] replaced by a float64 numpy dot (sums in numpy's order).  Mutants: "ragged" skips the rows of
    the ragged last workgroup, "first256" sums only the first 256 partials."""
    inp, n = inputs(case), case.p["n"]
    terms = inp["x"] * inp["y"]
    if mutant == "ragged":
        terms = terms.copy()
        terms[(n // 256) * 256:] = 0.0
    part = block_partials(n, terms)
    res = {k: v.copy() for k, v in out.items()}
    for rep in ("", "_again"):
        res["part" + rep][:len(part)] = part
        res["out" + rep][0] = part[:256].sum() if mutant == "first256" else part.sum()
    return res


def restate_mv(case, out, mutant=None):
    """out with the columns replaced by float64 numpy restatements (element-wise outputs only).  Mutants: "swap12"
    exchanges columns 1 and 2, "alpha0" uses column 0's alpha for every column of cg_xr_mv."""
    inp, n, nb, op = inputs(case), case.p["n"], case.p["nb"], case.family
    off = mv_layout(case)[0]
    res = {k: v.copy() for k, v in out.items()}
    for c in range(nb):
        src = {1: 2, 2: 1}.get(c, c) if mutant == "swap12" else c
        s, d = float(inp["s"][0 if mutant == "alpha0" else src]), float(inp["d"][src])
        sl = slice(off[c], off[c] + n)
        if op == "cg_xr_mv":
            res["Y"][sl] = inp["y"][src] + s * inp["a"][src]
            res["R"][sl] = inp["r"][src] - s * inp["b"][src]
        elif op == "cg_p_mv":
            res["Y"][sl] = inp["a"][src] + s * inp["y"][src]
        elif op == "scale_by_mv":
            res["Y"][sl] = exact_want("scale_by", inp["y"][src], s=d)
        elif op == "round_scale_by_mv":
            res["Y"][sl] = exact_want("round_scale_by", inp["a"][src], s=d)
        elif op == "widen_mv":
            res["Y"][sl] = exact_want("widen", inp["a"][src])
    return res


def restate_spmv(case, out, mutant=None):
    """out with y replaced by a float64 numpy product.  Mutants: "ldy" reads X with ldy instead of ldx, "beta_nan" forms
    beta y where beta = 0 and y holds NaN."""
    inp, nv, rp = inputs(case), case.p["nv"], inputs(case)["rp"]
    nrows, ncols, ldx, ldy = spmv_shape(case)
    row = np.repeat(np.arange(nrows), np.diff(rp))
    res = {k: v.copy() for k, v in out.items()}
    for v in range(nv):
        x0 = v * (ldy if mutant == "ldy" else ldx)
        s = np.zeros(nrows)
        np.add.at(s, row, inp["val"] * inp["x"][x0:x0 + ncols][inp["col"]])
        for k, (alpha, beta) in enumerate(SPMV_AB):
            y0 = np.full(nrows, np.nan) if beta == 0.0 else inp["y"][v]
            res["y%d" % k][v * ldy:v * ldy + nrows] = alpha * s + (beta * y0 if beta != 0.0 or mutant == "beta_nan" else 0.0)
    return res


# ------------------------------------------------------------------ coverage
def spmv_groups(nv):
    """The column groups spmv_mv walks through (device_hip.hip): four at a time, then the rest."""
    return [min(4, nv - v0) for v0 in range(0, nv, 4)]


def coverage(lib, cases):
    """The branch tags the cases reach, from their parameters and the product's own grid functions."""
    tags = set()
    for c in cases:
        p, F = c.p, c.family
        if F in EXACT_OPS + ("dot", "cg_xr", "cg_p") + MV_OPS:
            n, nb = p["n"], lib.vec_grid(p["n"])
            if "nb" in p and not 1 <= p["nb"] <= lib.lockstep_max:
                tags.add("%s:nb=%d refused" % (F, p["nb"]))
                continue
            tags.add("%s:%s" % (F, "n=0" if n == 0 else ("ragged" if n % 256 else "exact")))
            if n > nb * 256:
                tags.add(F + ":second_trip")
            if nb == lib.maxgrid and n <= nb * 256:
                tags.add(F + ":full_grid_one_trip")
            if F in ("dot", "cg_xr", "dot_mv", "cg_xr_mv"):
                tags.add(F + (":stage2>256" if nb > 256 else ":stage2<=256"))
                if nb in (256, 257):                     # one partial per thread of stage two; thread 0 takes a second
                    tags.add("%s:stage2=%d" % (F, nb))
            if "d" in p:
                tags.add("%s:d=%s" % (F, p["d"]))
            if p.get("crafted"):
                tags.add("%s:crafted_s=%d" % (F, p["crafted"]))
            if "nb" in p:
                tags.add("%s:nb=%d" % (F, p["nb"]))
                off = mv_offsets(n, p["nb"])[0][:p["nb"]]
                kinds = {"widen_mv": ("float", "double"), "round_scale_by_mv": ("double", "float")}.get(F, ("double", "double"))
                for kind in set(kinds):
                    if np.any(off % 2 == 1):
                        tags.add("%s:misaligned_%s_column" % (F, kind))
                    if np.any(off % 2 == 0):
                        tags.add("%s:aligned_%s_column" % (F, kind))
                if mv_zero_col(c) is not None:
                    tags.add(F + ":one_column_d=0")
        elif F == "update":
            n, k = p["n"], p["k"]
            tags.add("update:" + ("f32" if p["f32"] else "f64"))
            tags.add("update:k=%d" % k if k in (0, 1, 8, 9, lib.kmax) else ("update:k>kmax" if k > lib.kmax else "update:k=other"))
            if 0 < k <= lib.kmax:
                tags.add("update:" + ("ragged" if n % 256 else "exact"))
                tags.add("update:ld>n" if p["ld"] > n else "update:ld=n")
                if n > lib.row_grid(n) * 256:
                    tags.add("update:second_trip")
        elif F == "spmv_mv":
            inp = inputs(c)
            nrows, ncols, ldx, ldy = spmv_shape(c)
            L = lib.spmv_lanes(nrows, spmv_hint(c))
            tags.add("spmv_mv:L=%d" % L)
            for g in spmv_groups(p["nv"]):
                tags.add("spmv_mv:group=%d" % g if g > 1 else "spmv_mv:trailing_single_column")
            lens = np.diff(inp["rp"])
            if ldx != ldy and ncols != nrows:
                tags.add("spmv_mv:ldx!=ldy")
            if any(b == 0.0 for _, b in SPMV_AB):
                tags.add("spmv_mv:beta=0_over_nan")
            if 0 in lens:
                tags.add("spmv_mv:empty_row")
            if lens.max() > 8 * 32:
                tags.add("spmv_mv:long_row")
            if any(len(set(inp["col"][a:b])) < b - a for a, b in zip(inp["rp"][:-1], inp["rp"][1:])):
                tags.add("spmv_mv:repeated_column")
            if nrows % (256 // L):
                tags.add("spmv_mv:partial_block")
    return tags


_VEC = EXACT_OPS + ("dot", "cg_xr", "cg_p")
REQUIRED = (
    # every vector and reduction launcher: n = 0, ragged and exact last workgroup, the full grid in one trip, a second trip
    {"%s:%s" % (F, t) for F in _VEC for t in ("n=0", "ragged", "exact", "full_grid_one_trip", "second_trip")} |
    {"%s:%s" % (F, t) for F in ("dot", "cg_xr") for t in ("stage2<=256", "stage2>256", "stage2=256", "stage2=257")} |
    # the device scalar of the scale kernels, the crafted roundings
    {"%s:d=%s" % (F, d) for F in ("scale_by", "round_scale_by") for d in D_CLASSES} |
    {"%s:crafted_s=%d" % (F, s) for F in ("round_div", "round_scale_by") for s in (1, 2)} |
    # x += V y
    {"update:f64", "update:f32", "update:k=0", "update:k=1", "update:k=8", "update:k=9", "update:k=256", "update:k>kmax", "update:ragged",
     "update:ld>n", "update:ld=n", "update:second_trip"} |
    # batched launchers
    {"%s:%s" % (F, t) for F in MV_OPS for t in ("nb=1", "nb=2", "nb=3", "nb=4", "nb=0 refused", "nb=5 refused", "ragged", "second_trip",
                                                 "misaligned_double_column", "aligned_double_column")} |
    {"widen_mv:misaligned_float_column", "round_scale_by_mv:misaligned_float_column", "scale_by_mv:one_column_d=0",
     "round_scale_by_mv:one_column_d=0", "dot_mv:stage2>256", "cg_xr_mv:stage2>256", "dot_mv:stage2<=256", "cg_xr_mv:stage2<=256"} |
    # spmv_mv
    {"spmv_mv:L=1", "spmv_mv:L=2", "spmv_mv:L=4", "spmv_mv:L=8", "spmv_mv:group=2", "spmv_mv:group=3", "spmv_mv:group=4",
     "spmv_mv:trailing_single_column", "spmv_mv:ldx!=ldy", "spmv_mv:beta=0_over_nan", "spmv_mv:empty_row", "spmv_mv:long_row",
     "spmv_mv:repeated_column", "spmv_mv:partial_block"})
