"""Kernel lab of the Krylov layer: the vector, reduction and update launchers of krylov.hpp one by one, the orthogonalisation
passes A, B and C pass by pass (both basis types), the projection and border-product launchers, their batched (lock-step)
forms, and the multi-vector SpMV of device.hpp.  This module holds the case list, the inputs, the ctypes driver of the
harness (kry_harness.cpp), the numpy references, the checks and the coverage bookkeeping.

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
  passes A, B, C, projection    stated with their families below: every coefficient, every stage-one partial against its
  and border product            own rows, stage two against the returned partials, every row of w / dst / y
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
_PASS_SIG = "ippqqpqqpqpqpqqpqqpqp"
_SIGS.update({"pass_%s_%s" % (ab, t): "qq" + _PASS_SIG for ab in "abc" for t in ("f64", "f32")})
_SIGS.update({"pass_%s_mv" % ab: "qqii" + _PASS_SIG for ab in "abc"})
_SIGS.update({"proj_coeffs": "qipqqpqpqpqpqq", "proj_update": "qipqqpqpqqpqq", "oblique_project": "qipqqpqpqqpqpqqpqpqq",
              "border_product": "qipqqpqqpqpqqpqqpq"})
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
        for name in ("krylab_tile_grid", "krylab_tile_grid_f32"):
            getattr(self.lib, name).argtypes, getattr(self.lib, name).restype = [ctypes.c_int64, ctypes.c_int32], ctypes.c_int32
        self.tile, self.proj_max, self.proj_chunk, self.border_max, self.border_chunk = (
            int(getattr(self.lib, "krylab_" + name)()) for name in ("tile", "proj_max", "proj_chunk", "border_max", "border_chunk"))
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

    def tile_grid(self, n, k, f32=False):
        """kry_tile_grid / kry_tile_grid_f32 of krylov.hpp."""
        return int((self.lib.krylab_tile_grid_f32 if f32 else self.lib.krylab_tile_grid)(n, k))

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
    assert lib.maxgrid == MAXGRID and (lib.kmax, lib.guard, lib.tile) == (KMAX, GUARD, TILE)
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


# ---- the orthogonalisation passes A, B, C: single (both basis types) and batched
# Bounds (the rule at the top), per output:
#   h1[j] of pass A, h2[j] of pass B     m = n          terms V_ij w_i (pass B: the w the launcher returned)
#   a stage-one partial                  m = its rows   the rows of the tiles b, b + grid, ... (grid: the product's own
#                                                       kry_tile_grid[_f32](n, k), or kry_row_grid(n) in pass C)
#   stage two                            m = grid       against the extended-precision sum of the returned partials
#   a row of w (pass B) or dst (pass C)  m = k + 1      terms w_i and V_ij h_j
#   out[k + 1] of pass C                 m = n          against the sum of squares of the returned dst
# Exact: out[j] = h1[j] + h2[j] of the returned h2 (one add), out[k] = sqrt(out[k + 1]) (one ulp allowed, the distance is
# recorded in SQRT_ULPS), every input keeps its bits, n = 0 gives +0.0 everywhere.
KMAX, GUARD, TILE = 256, 1024, 64       # KRY_KMAX, the harness's guard words, KRY_TILE; run_case() asserts that the library agrees
PASS_MODES = ("dst", "w", "basis")      # pass C: a separate destination, dst = w, dst = column k of the same basis array
SQRT_ULPS = {}                          # case (and column) -> |out[k] - sqrt(out[k + 1])| in ulps, filled by the checks


def strided_cols(V, n, k, ld):
    """The k columns of a flat basis as a (k, n) view."""
    if k == 0:
        return np.zeros((0, n), V.dtype)
    return np.lib.stride_tricks.as_strided(V, shape=(k, n), strides=(ld * V.itemsize, V.itemsize), writeable=False)


def group_sums(terms, rows_per, grid, dtype=LD):
    """terms (c, n) -> (c, grid): entry b sums the rows of the blocks b, b + grid, b + 2 grid, ... of rows_per rows each."""
    c, n = terms.shape
    nblk = -(-n // rows_per)
    trips = max(1, -(-nblk // grid))
    pad = np.zeros((c, trips * grid * rows_per), dtype)
    pad[:, :n] = terms
    return pad.reshape(c, trips, grid, rows_per).sum(axis=(1, 3))


def plus_zero(name, a, fails):
    if np.any(a != 0.0) or np.any(np.signbit(a)):
        fails.append("%s: n = 0 must give +0.0" % name)


def chk_grouped(name, terms, rows_per, grid, part, total, fails):
    """The dots of one pass: total[j] against the sum of terms[j] (m = n), the partials part[b, j] against their rows, and
    total[j] against the returned partials (stage two, m = grid).  terms: a function (j0, j1) -> (j1 - j0, n) longdouble."""
    k, worst = len(total), 0.0
    n = terms(0, 1).shape[1]
    rows = group_sums(np.ones((1, n)), rows_per, grid, np.float64)[0]
    part = part.reshape(grid, k)
    for j0 in range(0, k, 16):
        j1 = min(k, j0 + 16)
        t = terms(j0, j1)
        ta = np.abs(t)
        worst = max(worst, _bounded(name, total[j0:j1], t.sum(axis=1), 2 * n * EPS * ta.sum(axis=1).astype(np.float64), fails))
        worst = max(worst, _bounded(name + " (a partial against its rows)", part[:, j0:j1].T, group_sums(t, rows_per, grid),
                                    2 * rows * EPS * group_sums(ta, rows_per, grid).astype(np.float64), fails))
    if np.all(np.isfinite(part)):
        pl = part.astype(LD)
        worst = max(worst, _bounded(name + " (stage two over its partials)", total, pl.sum(axis=0),
                                    2 * grid * EPS * np.abs(pl).sum(axis=0).astype(np.float64), fails))
    if n == 0:
        plus_zero(name, total, fails)
        plus_zero(name + " (partials)", part, fails)
    return worst


def chk_rows(name, cols, h, w0, got, fails):
    """got = w0 - V h row by row, m = k + 1."""
    k, n = cols.shape
    s, sa = np.zeros(n, LD), np.zeros(n, LD)
    for j0 in range(0, k, 16):
        t = cols[j0:j0 + 16].astype(LD) * h[j0:j0 + 16].astype(LD)[:, None]
        s += t.sum(axis=0)
        sa += np.abs(t).sum(axis=0)
    return _bounded(name, got, w0.astype(LD) - s, 2 * (k + 1) * EPS * (np.abs(w0) + sa.astype(np.float64)), fails)


def ulps(a, b):
    """The distance of two finite non-negative doubles in units of the last place."""
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def chk_pass_column(which, name, n, k, ld, col, got, grid, fails):
    """The reference checks of one column of one pass.  col: its inputs V, w, h1, h2; got: the payloads part, h1, h2, out, w,
    dst the launcher returned."""
    cols = strided_cols(col["V"], n, k, ld)
    dots = lambda w: (lambda j0, j1: cols[j0:j1].astype(LD) * w.astype(LD))
    if which == "a":
        return chk_grouped(name + " h1", dots(col["w"]), TILE, grid, got["part"], got["h1"], fails)
    if which == "b":
        worst = chk_rows(name + " w", cols, col["h1"], col["w"], got["w"], fails)
        if np.all(np.isfinite(got["w"])):
            worst = max(worst, chk_grouped(name + " h2", dots(got["w"]), TILE, grid, got["part"], got["h2"], fails))
        _exact(name + " out = h1 + h2", got["out"][:k], col["h1"] + got["h2"], fails)
        return worst
    worst = chk_rows(name + " dst", cols, col["h2"], col["w"], got["dst"], fails)
    if np.all(np.isfinite(got["dst"])):
        sq = lambda j0, j1: got["dst"].astype(LD)[None, :] ** 2
        worst = max(worst, chk_grouped(name + " norm^2", sq, 256, grid, got["part"], got["out"][k + 1:k + 2], fails))
    nrm, ss = got["out"][k], got["out"][k + 1]
    if not (np.isfinite(nrm) and np.isfinite(ss) and ss >= 0.0 and nrm >= 0.0):
        fails.append("%s: norm %r of norm^2 %r" % (name, nrm, ss))
    else:
        SQRT_ULPS[name] = ulps(nrm, np.sqrt(ss))
        if SQRT_ULPS[name] > 1:
            fails.append("%s: out[k] is %d ulps from the restatement sqrt(out[k + 1])" % (name, SQRT_ULPS[name]))
        if n == 0 and np.signbit(nrm):
            fails.append("%s: n = 0 must give +0.0" % name)
    return worst


def orth_params(case):
    """(pass, batched, f32, n, ld, mode, the k of every column, nb as given)."""
    p, batched = case.p, case.family.endswith("_mv")
    ks = tuple(p["ks"]) if batched else (p["k"],)
    return case.family[5], batched, bool(p["f32"]), p["n"], p["ld"], p.get("mode", 0), ks, p["nb"] if batched else 1


def orth_inputs(case):
    which, batched, f32, n, ld, mode, ks, nb = orth_params(case)
    rng, inp = case.rng(), {}
    for c, k in enumerate(ks):
        V = vec(rng, (k - 1) * ld + n if k > 0 else 0)
        inp["V%d" % c] = V.astype(np.float32) if f32 else V
        inp["w%d" % c], inp["h1%d" % c], inp["h2%d" % c] = vec(rng, n), vec(rng, min(k, KMAX)), vec(rng, min(k, KMAX))
    return inp


def orth_column(inp, c):
    return {key: inp["%s%d" % (key, c)] for key in ("V", "w", "h1", "h2")}


def orth_valid(ks, nb, batched):
    return all(1 <= k <= KMAX for k in ks) and (not batched or 1 <= nb <= 4)


def spread(lengths, start):
    """Element offsets of regions of the given lengths in one flat array: the first at `start`, the gap behind region c is
    1 + c elements, so odd and even starts both occur.  Returns (offsets, total length)."""
    off, pos = [], start
    for c, L in enumerate(lengths):
        off.append(pos)
        pos += L + 1 + c
    return off, (off[-1] + lengths[-1] if lengths else 0)


def orth_layout(which, batched, n, ld, mode, ks, grids):
    """The offset table (7 kinds x 4 columns) and the payload length of every kind.  The scratch of a column is as long as
    its own defined set (tighter than the solver's allocation), so a partial too many lands on the canary."""
    start = 1 if batched else 0
    vlen = [(k * ld + n if mode == 2 else ((k - 1) * ld + n if k > 0 else 0)) for k in ks]
    plen = [(g * k if which in "ab" else g) if 1 <= k <= KMAX else 8 for k, g in zip(ks, grids)]
    tab, tot = np.zeros((7, 4), np.int64), np.zeros(7, np.int64)
    for kind, lens in enumerate((vlen, [n] * len(ks), [n] * len(ks), plen, [KMAX] * len(ks), [KMAX] * len(ks), [KMAX + 2] * len(ks))):
        off, tot[kind] = spread(lens, start)
        tab[kind, :len(off)] = off
    return tab, tot


def canary_buffer(n_words):
    return np.full(n_words, CANARY, dtype=np.uint64).view(np.float64)


def orth_initial(which, batched, f32, n, ld, mode, ks, inp, tab, tot):
    """The buffers as the launcher finds them: canary everywhere except the caller's content (the basis columns, w, h1, h2)."""
    buf = {key: canary_buffer(int(tot[kind]) + GUARD) for kind, key in ((1, "W"), (3, "P"), (4, "H1"), (5, "H2"), (6, "O"))}
    if which == "c" and mode == 0:
        buf["DST"] = canary_buffer(int(tot[2]) + GUARD)
    if mode == 2:
        buf["V"] = canary_buffer(int(tot[0]) + GUARD)
    else:
        buf["V"] = np.full(int(tot[0]), np.nan, dtype=np.float32 if f32 else np.float64)    # a read of a gap is a NaN in the result
    for c, k in enumerate(ks):
        V = inp["V%d" % c]
        if mode == 2:
            for j in range(k):
                buf["V"][tab[0, c] + j * ld:tab[0, c] + j * ld + n] = V[j * ld:j * ld + n]
        else:
            buf["V"][tab[0, c]:tab[0, c] + len(V)] = V
        buf["W"][tab[1, c]:tab[1, c] + n] = inp["w%d" % c]
        if which != "a":                                   # pass A finds the canary in h1: it must write all of h1[0:k)
            buf["H1"][tab[4, c]:tab[4, c] + len(inp["h1%d" % c])] = inp["h1%d" % c]
        if which != "b":
            buf["H2"][tab[5, c]:tab[5, c] + len(inp["h2%d" % c])] = inp["h2%d" % c]
    return buf


def orth_call(lib, which, batched, f32, n, ld, mode, ks, nb, inp):
    """One launch.  Returns the whole buffers, the error code, the own grid of every column and the layout."""
    grids = [(lib.tile_grid(n, k, f32) if which in "ab" else lib.row_grid(n)) if 1 <= k <= KMAX else 1 for k in ks]
    tab, tot = orth_layout(which, batched, n, ld, mode, ks, grids)
    buf = orth_initial(which, batched, f32, n, ld, mode, ks, inp, tab, tot)
    K = np.zeros(4, np.int32)
    K[:len(ks)] = ks
    init = lambda kind: int(tot[kind]) * 8
    dst = buf.get("DST")
    name = "pass_%s_mv" % which if batched else "pass_%s_%s" % (which, "f32" if f32 else "f64")
    code, msg = lib.call(name, *((n, ld) + ((nb, int(f32)) if batched else ()) + (
        mode, K, buf["V"], int(tot[0]), words(buf["V"]) if mode == 2 else 0, buf["W"], init(1), words(buf["W"]), dst,
        words(dst) if dst is not None else 0, buf["P"], words(buf["P"]), buf["H1"], init(4), words(buf["H1"]), buf["H2"], init(5),
        words(buf["H2"]), buf["O"], words(buf["O"]), np.ascontiguousarray(tab.ravel()))))
    res = {key: v for key, v in buf.items() if key != "V" or mode == 2}
    res.update(code=np.array([code]), grid=i64(grids), tab=tab, tot=tot)
    return res


def orth_payloads(which, n, ld, mode, ks, res):
    """Per column, what the pass defines: its slices of the returned buffers."""
    tab, cols = res["tab"], []
    for c, k in enumerate(ks):
        g = int(res["grid"][c])
        got = {"part": res["P"][tab[3, c]:tab[3, c] + (g * k if which in "ab" else g)], "h1": res["H1"][tab[4, c]:tab[4, c] + k],
               "h2": res["H2"][tab[5, c]:tab[5, c] + k], "out": res["O"][tab[6, c]:tab[6, c] + k + 2], "w": res["W"][tab[1, c]:tab[1, c] + n]}
        if which == "c":
            got["dst"] = (res["DST"][tab[2, c]:tab[2, c] + n] if mode == 0 else got["w"] if mode == 1
                          else res["V"][tab[0, c] + k * ld:tab[0, c] + k * ld + n])
        cols.append(got)
    return cols


ORTH_DEFINED = {"a": ("part", "h1"), "b": ("part", "h2", "out", "w"), "c": ("part", "out", "dst")}    # compared with the single launch


def orth_outputs(which, k, got):
    """The defined outputs of a column, out cut to its defined part."""
    res = {key: got[key] for key in ORTH_DEFINED[which]}
    if "out" in res:
        res["out"] = got["out"][:k] if which == "b" else got["out"][k:k + 2]
    return res


def orth_run(lib, case, inp):
    which, batched, f32, n, ld, mode, ks, nb = orth_params(case)
    res = orth_call(lib, which, batched, f32, n, ld, mode, ks, nb, inp)
    if int(res["code"][0]) != 0:
        return res
    if not batched and which == "c":                       # two calls: the same bits
        again = orth_call(lib, which, batched, f32, n, ld, mode, ks, nb, inp)
        res["same_again"] = np.array([all(same_bits(res[key], again[key]) for key in again)])
    if batched:                                            # the single launcher of the same library on the operands of column c
        got = orth_payloads(which, n, ld, mode, ks, res)
        for c, k in enumerate(ks):
            one_inp = {"%s0" % key: v for key, v in orth_column(inp, c).items()}
            one = orth_call(lib, which, False, f32, n, ld, mode, (k,), 1, one_inp)
            if int(one["code"][0]) != 0:
                raise RuntimeError("single launch of column %d: error %d" % (c, int(one["code"][0])))
            single = orth_outputs(which, k, orth_payloads(which, n, ld, mode, (k,), one)[0])
            res["same_as_single%d" % c] = np.array([same_bits(digest(single[key]), digest(v))
                                                    for key, v in orth_outputs(which, k, got[c]).items()])
    return res


def unchanged(buf, init, defined, what, fails):
    """Every word of buf outside the defined elements has the bits the launcher found there."""
    raw = np.uint64 if buf.dtype.itemsize == 8 else np.uint32
    mask = np.zeros(buf.size, bool)
    for a, b in defined:
        mask[a:b] = True
    bad = np.flatnonzero((buf.view(raw) != init.view(raw)) & ~mask)
    if bad.size:
        fails.append("%s: written outside its output set at %s (%d words)" % (what, bad[:3], bad.size))


def orth_check(case, inp, out):
    which, batched, f32, n, ld, mode, ks, nb = orth_params(case)
    fails, worst, code = [], 0.0, int(out["code"][0])
    tab, tot = out["tab"], out["tot"]
    init = orth_initial(which, batched, f32, n, ld, mode, ks, inp, tab, tot)
    valid = orth_valid(ks, nb, batched)
    sets = {key: [] for key in ("W", "DST", "V", "P", "H1", "H2", "O")}
    if valid:
        for c, k in enumerate(ks):
            g = int(out["grid"][c])
            sets["P"].append((tab[3, c], tab[3, c] + (g * k if which in "ab" else g)))
            if which == "a":
                sets["H1"].append((tab[4, c], tab[4, c] + k))
            elif which == "b":
                sets["H2"].append((tab[5, c], tab[5, c] + k))
                sets["O"].append((tab[6, c], tab[6, c] + k))
                sets["W"].append((tab[1, c], tab[1, c] + n))
            else:
                sets["O"].append((tab[6, c] + k, tab[6, c] + k + 2))
                sets[("DST", "W", "V")[mode]].append((tab[(2, 1, 0)[mode], c] + (k * ld if mode == 2 else 0),
                                                      tab[(2, 1, 0)[mode], c] + (k * ld if mode == 2 else 0) + n))
    for key in sets:
        if key in out:
            unchanged(out[key], init[key], sets[key], {"W": "w", "DST": "dst", "V": "the basis", "P": "part", "H1": "h1", "H2": "h2",
                                                       "O": "out"}[key], fails)
    if not valid:
        if code != -2:
            fails.append("k = %s, nb = %d: error %d instead of -2" % (ks, nb, code))
        return fails, 0.0
    if code != 0:
        return fails + ["error %d" % code], 0.0
    got = orth_payloads(which, n, ld, mode, ks, out)
    for c, k in enumerate(ks):
        name = "%s column %d" % (case.name, c) if batched else case.name
        worst = max(worst, chk_pass_column(which, name, n, k, ld, orth_column(inp, c), got[c], int(out["grid"][c]), fails))
        if batched:
            for key, same in zip(orth_outputs(which, k, got[c]), out["same_as_single%d" % c]):
                if not same:
                    fails.append("column %d: %s differs from the single launch" % (c, key))
    if "same_again" in out and not bool(out["same_again"][0]):
        fails.append("two calls differ")
    return fails, worst


# ---- projection vectors and the border product
# proj_coeffs: d = G (Q' x) in ws.h1.  Without G d_j is a sum of n terms; with G the bound E_j = (n + m + 1) u (|G| a)_j,
# a_l = sum_i |Q_il x_i|, derived in check_oblique_project of tests/native_projected_cases.py, and so is the row bound of
# oblique_project, (m + 2) u (|x_i| + sum_j |P_ij| (|d_j| + E_j)) + sum_j |P_ij| E_j.  A partial is checked against its rows
# (256 per workgroup, kry_row_grid(n) workgroups); stage two: d_j = sum_l G_jl sum_b part[b, l], where every term passes
# through at most grid + m + 1 roundings.  proj_update: m + 1 terms per row.  border_product: m + 1 terms per row, n + m per
# entry of the tail.
def flat_cols(rng, n, m, ld):
    """An n x m column-major array with leading dimension ld, exactly (m - 1) ld + n entries; the padding holds NaN."""
    a = np.full(max(0, (m - 1) * ld + n) if m > 0 else 0, np.nan)
    for j in range(m):
        a[j * ld:j * ld + n] = vec(rng, n)
    return a


def proj_refused(case):
    p = case.p
    return p["n"] < 1 or p["m"] < 1 or p["m"] > 32 or p["ld"] < p["n"]


def proj_inputs(case):
    rng, n, m, ld = case.rng(), case.p["n"], case.p["m"], case.p["ld"]
    inp = {"Q": flat_cols(rng, n, m, ld), "P": flat_cols(rng, n, m, ld), "x": vec(rng, n), "G": vec(rng, m * m), "d": vec(rng, min(m, 32))}
    if case.family == "border_product":
        inp["z"], inp["y"] = vec(rng, n + m), vec(rng, n)
    return inp


def proj_run(lib, case, inp):
    n, m, ld, F, res = case.p["n"], case.p["m"], case.p["ld"], case.family, {}
    grid = lib.row_grid(n)
    res["grid"] = i64([grid])
    npart = grid * m if not proj_refused(case) else 8
    for v in (0, 1):                                       # proj_coeffs, oblique_project: without and with G; proj_update: out of
        part, h1 = lib.out(npart), lib.out(KMAX)           # place and in place; border_product: without and with C
        G = inp["G"] if v else None
        if F == "proj_coeffs":
            code, _ = lib.call("proj_coeffs", n, m, inp["Q"], len(inp["Q"]), ld, G, m * m, inp["x"], n, part, words(part), h1, 0, words(h1))
            res.update({"P%d" % v: part, "H%d" % v: h1})
        elif F == "proj_update":
            h1[:len(inp["d"])] = inp["d"]
            y = lib.out(n, init=inp["x"] if v else None)
            code, _ = lib.call("proj_update", n, m, inp["P"], len(inp["P"]), ld, None if v else inp["x"], n, y, n * 8 if v else 0, words(y),
                               h1, len(inp["d"]) * 8, words(h1))
            res.update({"Y%d" % v: y, "H%d" % v: h1})
        elif F == "oblique_project":
            ys = []
            for inplace in (0, 1):
                part, h1 = lib.out(npart), lib.out(KMAX)
                y = lib.out(n, init=inp["x"] if inplace else None)
                code, _ = lib.call("oblique_project", n, m, inp["Q"], len(inp["Q"]), ld, G, m * m, inp["P"], len(inp["P"]), ld,
                                   None if inplace else inp["x"], n, y, n * 8 if inplace else 0, words(y), part, words(part), h1, 0, words(h1))
                ys.append((y, part, h1))
            res.update({"Y%d" % v: ys[0][0], "P%d" % v: ys[0][1], "H%d" % v: ys[0][2],
                        "inplace_same%d" % v: np.array([all(same_bits(a, b) for a, b in zip(ys[0], ys[1]))])})
        else:
            y, z = lib.out(n + m, init=inp["y"]), lib.out(n + m, init=inp["z"])
            code, _ = lib.call("border_product", n, m, inp["Q"], len(inp["Q"]), ld, inp["P"], len(inp["P"]), ld, G, m * m, z, (n + m) * 8,
                               words(z), y, n * 8, words(y), part, words(part))
            res.update({"Y%d" % v: y, "Z%d" % v: z, "P%d" % v: part})
        res["code%d" % v] = np.array([code])
    return res


def proj_cols(a, n, m, ld):
    return strided_cols(a, n, m, ld)


def proj_check(case, inp, out):
    n, m, ld, F = case.p["n"], case.p["m"], case.p["ld"], case.family
    fails, worst, grid = [], 0.0, int(out["grid"][0])
    for v in (0, 1):
        code, nm = int(out["code%d" % v][0]), "%s (%s)" % (case.name, ("plain", "second form")[v])
        start = {"H": canary_buffer(KMAX + GUARD)}
        if F == "proj_update":
            start["H"][:len(inp["d"])] = inp["d"]
        if F == "border_product":
            start["Z"], start["Y"] = canary_buffer(n + m + GUARD), canary_buffer(n + m + GUARD)
            start["Z"][:n + m], start["Y"][:n] = inp["z"], inp["y"]
        else:
            start["Y"] = canary_buffer(n + GUARD)
            if F == "proj_update" and v:
                start["Y"][:n] = inp["x"]
        if "P%d" % v in out:
            start["P"] = canary_buffer(words(out["P%d" % v]))
        ok = not proj_refused(case) and code == 0
        sets = {"H": [(0, m)] if ok and F in ("proj_coeffs", "oblique_project") else [], "P": [(0, grid * m)] if ok else [], "Z": [],
                "Y": [(0, n + m if F == "border_product" else n)] if ok else []}
        for key in ("H", "P", "Z", "Y"):
            if "%s%d" % (key, v) in out:
                unchanged(out["%s%d" % (key, v)], start[key], sets[key], {"H": "h1", "P": "part", "Z": "z", "Y": "y"}[key], fails)
        if proj_refused(case):
            if code != -2:
                fails.append("%s: error %d instead of -2" % (nm, code))
            continue
        if code != 0:
            fails.append("%s: error %d" % (nm, code))
            continue
        Q, P, xl = proj_cols(inp["Q"], n, m, ld).astype(LD), proj_cols(inp["P"], n, m, ld).astype(LD), inp["x"].astype(LD)
        G = inp["G"].reshape(m, m).T if v else None        # column-major: G[j, l] = flat[j + m l]
        if F == "proj_update":
            t = P * inp["d"].astype(LD)[:, None]
            worst = max(worst, _bounded(nm + " y", out["Y%d" % v][:n], xl - t.sum(axis=0),
                                        2 * (m + 1) * EPS * (np.abs(inp["x"]) + np.abs(t).sum(axis=0).astype(np.float64)), fails))
            continue
        if F == "border_product":
            z, zl = out["Z%d" % v][:n + m], inp["z"].astype(LD)
            t = Q * zl[n:][:, None]                        # V s
            worst = max(worst, _bounded(nm + " rows", out["Y%d" % v][:n], inp["y"].astype(LD) + t.sum(axis=0),
                                        2 * (m + 1) * EPS * (np.abs(inp["y"]) + np.abs(t).sum(axis=0).astype(np.float64)), fails))
            wx = P * zl[:n]                                # W' x
            cs = (G.astype(LD) * zl[n:][None, :]) if v else np.zeros((m, m), LD)
            worst = max(worst, _bounded(nm + " tail", out["Y%d" % v][n:n + m], wx.sum(axis=1) + cs.sum(axis=1),
                                        2 * (n + m) * EPS * (np.abs(wx).sum(axis=1) + np.abs(cs).sum(axis=1)).astype(np.float64), fails))
            part = out["P%d" % v][:grid * m].reshape(grid, m)
            rows = group_sums(np.ones((1, n)), 256, grid, np.float64)[0]
            worst = max(worst, _bounded(nm + " (a partial against its rows)", part.T, group_sums(wx, 256, grid),
                                        2 * rows * EPS * group_sums(np.abs(wx), 256, grid).astype(np.float64), fails))
            continue
        # the coefficients
        t = Q * xl
        a = np.abs(t).sum(axis=1).astype(np.float64)
        c = t.sum(axis=1)
        d = G.astype(LD) @ c if v else c
        E = (n + m + 1) * EPS * ((np.abs(G) if v else np.eye(m)) @ a)
        got_d = out["H%d" % v][:m]
        worst = max(worst, _bounded(nm + " d", got_d, d, E if v else 2 * n * EPS * a, fails))
        part = out["P%d" % v][:grid * m].reshape(grid, m)
        rows = group_sums(np.ones((1, n)), 256, grid, np.float64)[0]
        worst = max(worst, _bounded(nm + " (a partial against its rows)", part.T, group_sums(t, 256, grid),
                                    2 * rows * EPS * group_sums(np.abs(t), 256, grid).astype(np.float64), fails))
        if np.all(np.isfinite(part)):
            pl = part.astype(LD)
            Gl, Ga = (G.astype(LD), np.abs(G)) if v else (np.eye(m).astype(LD), np.eye(m))
            worst = max(worst, _bounded(nm + " (stage two over its partials)", got_d, Gl @ pl.sum(axis=0),
                                        2 * (grid + m + 1) * EPS * (Ga @ np.abs(pl).sum(axis=0).astype(np.float64)), fails))
        if F == "oblique_project":
            s, sa, se = np.zeros(n, LD), np.zeros(n), np.zeros(n)
            for j in range(m):
                s += P[j] * d[j]
                sa += np.abs(P[j]).astype(np.float64) * (float(abs(d[j])) + E[j])
                se += np.abs(P[j]).astype(np.float64) * E[j]
            worst = max(worst, _bounded(nm + " y", out["Y%d" % v][:n], xl - s, (m + 2) * EPS * (np.abs(inp["x"]) + sa) + se, fails))
            if not bool(out["inplace_same%d" % v][0]):
                fails.append("%s: y = x gives other bits than the out-of-place call" % nm)
    return fails, worst


EXACT_OPS = ("sub", "add", "div", "scale_by", "widen", "round_div", "round_scale_by")
FAMILIES = {op: (ev_inputs, ev_run, ev_check) for op in EXACT_OPS}
FAMILIES.update({"dot": (dot_inputs, dot_run, dot_check), "cg_xr": (cg_inputs, cg_run, cg_check), "cg_p": (cg_inputs, cg_run, cg_check),
                 "update": (upd_inputs, upd_run, upd_check), "spmv_mv": (spmv_inputs, spmv_run, spmv_check)})
FAMILIES.update({op: (mv_inputs, mv_run, mv_check) for op in MV_OPS})
PASS_OPS = ("pass_a", "pass_b", "pass_c")
PASS_MV_OPS = ("pass_a_mv", "pass_b_mv", "pass_c_mv")
PROJ_OPS = ("proj_coeffs", "proj_update", "oblique_project", "border_product")
FAMILIES.update({op: (orth_inputs, orth_run, orth_check) for op in PASS_OPS + PASS_MV_OPS})
FAMILIES.update({op: (proj_inputs, proj_run, proj_check) for op in PROJ_OPS})
BOUNDED_FAMILIES = ("dot", "cg_xr", "cg_p", "update", "dot_mv", "cg_xr_mv", "cg_p_mv", "spmv_mv") + PASS_OPS + PASS_MV_OPS + PROJ_OPS
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

# ---- the orthogonalisation passes, the projection and the border product.  The shapes are the smallest that reach each
# branch; coverage() checks them against the product's own grid functions
PROJ_M = (1, 2, 7, 8, 9, 16, 17, 32)
PROJ_N = (1, 255, 257, 4099)
MV_KS = (5, 256, 3, 31)                                    # the k of the columns of a batched launch: the largest is not column 0


def _pad(i):
    return 5 if i % 2 else 0


def _ty(f32):
    return "f32" if f32 else "f64"


def tile_shapes(f32):
    """(n, k) of passes A and B.  The k where the workgroups per CU change: 30 | 31 and 148 | 149 (FP64 basis), 61 | 62 (FP32)."""
    edge = (61, 62) if f32 else (30, 31, 148, 149)
    return ([(0, 5)] + [(n, k) for n in (1, 63, 64, 65) for k in (1, 2, 3, 4, 5)] + [(4099, k) for k in (1, 3) + edge + (255, 256)] +
            [(65, 255), (65, 256), (131072, 2), (131073, 2), (16449, 2), (32769, 256) if f32 else (16385, 256)])


def pass_c_shapes(f32):
    """(n, k, mode): every k and every n with every destination mode the basis type has."""
    shapes = [(n, k, (a * 5 + b) % (2 if f32 else 3)) for a, n in enumerate((1, 255, 256, 257, 4099)) for b, k in enumerate((1, 7, 8, 9, 256))]
    return shapes + [(0, 7, 0), (524289, 3, 1 if f32 else 2)]


def _pass_c_case(f32, i, n, k, mode):
    return Case("pass_c_%s_n%d_k%d_%s" % (_ty(f32), n, k, PASS_MODES[mode]), "pass_c", n=n, k=k, mode=mode, f32=f32,
                ld=n + (5 if mode == 2 else _pad(i)))


def _mv_case(op, f32, n, nb, ks, tag=""):
    return Case("%s_%s_n%d_nb%d%s" % (op, _ty(f32), n, nb, tag), op, n=n, nb=nb, ks=ks, f32=f32, ld=n + _pad(nb), mode=nb % 2 if op == "pass_c_mv" else 0)


CASES += (
    [Case("%s_%s_n%d_k%d" % (op, _ty(f32), n, k), op, n=n, k=k, f32=f32, ld=n + _pad(i))
     for op in ("pass_a", "pass_b") for f32 in (False, True) for i, (n, k) in enumerate(tile_shapes(f32))] +
    [_pass_c_case(f32, i, n, k, mode) for f32 in (False, True) for i, (n, k, mode) in enumerate(pass_c_shapes(f32))] +
    [Case("%s_%s_n65_k%d" % (op, _ty(f32), k), op, n=65, k=k, f32=f32, ld=70, mode=0) for op in PASS_OPS for f32 in (False, True) for k in (0, 257)] +
    [_mv_case(op, f32, n, nb, MV_KS[:nb]) for op in PASS_MV_OPS for f32 in (False, True) for n in (1, 65, 4099) for nb in (1, 2, 3, 4)] +
    # one launch whose columns have own grids 256 / 258 / 256 / 258 (FP32: 512 / 514 / 512 / 514): the columns with the smaller
    # grid take a second trip, and the last two workgroups of those columns leave before the barrier
    [_mv_case(op, False, 16449, 4, (256, 1, 149, 31)) for op in ("pass_a_mv", "pass_b_mv")] +
    [_mv_case(op, True, 32833, 4, (256, 1, 193, 2)) for op in ("pass_a_mv", "pass_b_mv")] +
    [_mv_case(op, False, 65, nb, ks, tag) for op in PASS_MV_OPS
     for nb, ks, tag in ((0, (), ""), (5, MV_KS, ""), (4, (5, 0, 3, 31), "_k0"), (4, (5, 3, 257, 31), "_k257"))] +
    [Case("%s_n%d_m%d" % (op, n, m), op, n=n, m=m, ld=n + _pad(a + b)) for op in PROJ_OPS for a, n in enumerate(PROJ_N) for b, m in enumerate(PROJ_M)] +
    [Case("%s_n524289_m9" % op, op, n=524289, m=9, ld=524289) for op in PROJ_OPS] +
    # the chunk tails 3 to 6 (a kernel instance each), which the m above do not reach
    [Case("%s_n257_m%d" % (op, m), op, n=257, m=m, ld=257 + _pad(m)) for op in PROJ_OPS for m in (3, 4, 5, 6)] +
    [Case("%s_refused_n%d_m%d_ld%d" % (op, n, m, ld), op, n=n, m=m, ld=ld) for op in PROJ_OPS
     for n, m, ld in ((257, 0, 257), (257, 33, 257), (0, 2, 0), (257, 2, 256))]
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


def restate_pass(case, out, mutant=None):
    """out of a single pass A, B or C with every defined output replaced by a float64 numpy restatement (sums in numpy's
    order, the partials per workgroup as the grid strides).  Mutants:
      pass A  "ragged"   drops the rows of the ragged last tile
              "grid+1"   credits tile t to workgroup t mod (grid + 1) (what falls to the workgroup that does not exist goes to
                         the last one): h1 stays right and agrees with the partials, only a partial against its own rows
                         shows it
              "w_float"  rounds w to float (a float-basis pass that narrows the vector as well)
      pass B  "old_w"    h2 from the w before the update
              "drop3"    the columns j = 3 mod 4 (the fourth quarter sum) missing from the update
      pass C  "h1"       subtracts V h1 instead of V h2"""
    which, batched, f32, n, ld, mode, ks, nb = orth_params(case)
    assert not batched
    inp, k, tab, grid = inputs(case), ks[0], out["tab"], int(out["grid"][0])
    cols = strided_cols(inp["V0"], n, k, ld).astype(np.float64)
    w, h1, h2 = inp["w0"], inp["h10"], inp["h20"]
    res = {key: v.copy() for key, v in out.items()}

    def put(key, kind, values, shift=0):
        res[key][tab[kind, 0] + shift:tab[kind, 0] + shift + len(values)] = values

    def tile_dots(wv):
        t = cols * wv
        if mutant == "ragged":
            t[:, (n // TILE) * TILE:] = 0.0
        if mutant == "grid+1":
            wide = group_sums(t, TILE, grid + 1, np.float64)
            part = wide[:, :grid].copy()
            part[:, grid - 1] += wide[:, grid]
        else:
            part = group_sums(t, TILE, grid, np.float64)
        return part.T.ravel(), part.sum(axis=1)            # part[b * k + j]

    if which == "a":
        part, h = tile_dots(w.astype(np.float32).astype(np.float64) if mutant == "w_float" else w)
        put("P", 3, part)
        put("H1", 4, h)
    elif which == "b":
        hh = h1.copy()
        if mutant == "drop3":
            hh[3::4] = 0.0
        w_new = w - (cols * hh[:, None]).sum(axis=0)
        part, h = tile_dots(w if mutant == "old_w" else w_new)
        put("W", 1, w_new)
        put("P", 3, part)
        put("H2", 5, h)
        put("O", 6, h1 + h)
    else:
        dst = w - (cols * (h1 if mutant == "h1" else h2)[:, None]).sum(axis=0)
        part = group_sums((dst * dst)[None, :], 256, grid, np.float64)[0]
        put(("DST", "W", "V")[mode], (2, 1, 0)[mode], dst, k * ld if mode == 2 else 0)
        put("P", 3, part)
        put("O", 6, np.array([np.sqrt(part.sum()), part.sum()]), k)
    return res


def restate_proj(case, out, mutant=None):
    """out of proj_coeffs or border_product replaced by a float64 numpy restatement.  Mutants: "G_T" applies G transposed (the
    border product: reads C row-major), "drop_chunk" leaves the columns of the last chunk out of the dots."""
    inp, n, m, ld, F = inputs(case), case.p["n"], case.p["m"], case.p["ld"], case.family
    grid = int(out["grid"][0])
    Q, P, x = proj_cols(inp["Q"], n, m, ld), proj_cols(inp["P"], n, m, ld), inp["x"]
    res = {key: v.copy() for key, v in out.items()}
    for v in (0, 1):
        G = inp["G"].reshape(m, m) if mutant == "G_T" else inp["G"].reshape(m, m).T
        if F == "border_product":
            z = inp["z"]
            part = group_sums(P * z[:n], 256, grid, np.float64)
            res["Y%d" % v][:n] = inp["y"] + (Q * z[n:, None]).sum(axis=0)
            res["Y%d" % v][n:n + m] = part.sum(axis=1) + (G @ z[n:] if v else 0.0)
        else:
            part = group_sums(Q * x, 256, grid, np.float64)
            if mutant == "drop_chunk":
                part[((m - 1) // 8) * 8:] = 0.0
            c = part.sum(axis=1)
            res["H%d" % v][:m] = G @ c if v else c
        res["P%d" % v][:grid * m] = part.T.ravel()
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
        elif F in PASS_OPS + PASS_MV_OPS:
            tags |= orth_coverage(lib, c)
        elif F in PROJ_OPS:
            tags |= proj_coverage(lib, c)
    return tags


def orth_coverage(lib, case):
    """The tags of one case of passes A, B, C or their batched forms, from the product's kry_tile_grid[_f32], kry_row_grid,
    KRY_TILE, KRY_KMAX and KRY_LOCKSTEP_MAX."""
    which, batched, f32, n, ld, mode, ks, nb = orth_params(case)
    F, tags, T, huge = "%s_%s" % (case.family, _ty(f32)), set(), lib.tile, 1 << 40
    add = lambda t: tags.add("%s:%s" % (F, t))
    if batched and not 1 <= nb <= lib.lockstep_max:
        add("nb=%d refused" % nb)
        return tags
    if any(k < 1 for k in ks) or any(k > lib.kmax for k in ks):
        add("k=0 refused" if any(k < 1 for k in ks) else "k>kmax refused")
        return tags
    ntiles = -(-n // T)
    grids = [lib.tile_grid(n, k, f32) if which in "ab" else lib.row_grid(n) for k in ks]
    add("ld>n" if ld > n else "ld=n")
    if batched:
        add("nb=%d" % nb)
        if len(set(grids)) > 1:
            add("different_own_grids")
        if any(g < max(grids) and ntiles > g for g in grids):
            add("early_exit_and_second_trip")
        if int(np.argmax(ks)) != 0:
            add("largest_k_not_first")
        tab = orth_layout(which, batched, n, ld, mode, ks, grids)[0]
        for c in range(nb):
            add("misaligned_column" if tab[1, c] % 2 else "aligned_column")
        if which == "c":
            add("mode=" + PASS_MODES[mode])
        return tags
    k, grid = ks[0], grids[0]
    if which == "c":
        add("n=0" if n == 0 else ("ragged" if n % 256 else "exact"))
        add("k=%d" % k if k in (1, 7, 8, 9, lib.kmax) else "k=other")
        add("mode=" + PASS_MODES[mode])
        if n > 256:
            add("more_workgroups")
        if n > grid * 256:
            add("second_trip")
        if mode == 2 and ld > n:
            add("basis_mode_with_padding")
        return tags
    cap = lib.tile_grid(huge, k, f32)                       # 256 x workgroups per CU
    add("n=0" if n == 0 else ("one_ragged_tile" if ntiles == 1 and n % T else ("exact_tile_edge" if n % T == 0 else "ragged_last_tile")))
    if ntiles == grid == cap:
        add("full_grid_one_trip")
    if ntiles > grid:
        add("second_trip")
        if n % T:
            add("second_trip_ragged_last_tile")
    add("wpc=%d" % (cap // 256))
    if k < lib.kmax and lib.tile_grid(huge, k + 1, f32) < cap:
        add("last_k_of_wpc=%d" % (cap // 256))
    if k > 1 and lib.tile_grid(huge, k - 1, f32) > cap:
        add("first_k_of_wpc=%d" % (cap // 256))
    add("k=%d" % k if k in (1, 2, 3, 4, 5, lib.kmax - 1, lib.kmax) else "k=other")
    add("stage2>256" if grid > 256 else "stage2<=256")
    return tags


def proj_coverage(lib, case):
    """The tags of one projection or border case, from kry_row_grid and the product's chunk widths and limits."""
    F, n, m, ld, tags = case.family, case.p["n"], case.p["m"], case.p["ld"], set()
    add = lambda t: tags.add("%s:%s" % (F, t))
    most, chunk = (lib.border_max, lib.border_chunk) if F == "border_product" else (lib.proj_max, lib.proj_chunk)
    if proj_refused(case):
        add("m=0 refused" if m < 1 else ("m>max refused" if m > most else ("n=0 refused" if n < 1 else "ld<n refused")))
        return tags
    add("m=%d" % m)
    add("chunks=%d" % -(-m // chunk))
    add("chunk_tail=%d" % (m % chunk or chunk))
    add("n=1" if n == 1 else ("ragged" if n % 256 else "exact"))
    add("ld>n" if ld > n else "ld=n")
    if n > lib.row_grid(n) * 256:
        add("second_trip")
    if n > 256:
        add("more_workgroups")
    add("both_forms")         # every case runs without and with G (C of the border product), proj_update out of place and in place
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
     "spmv_mv:repeated_column", "spmv_mv:partial_block"} |
    # passes A and B, each basis type: the tile edges, the grid-stride trips, the workgroups-per-CU classes of the LDS tile
    # (FP64: 8 up to k = 30, 7 from 31, 2 up to 148, 1 from 149; FP32: 8 up to 61, 7 from 62, 2 at 256), the k below and above
    # the four quarter waves, both stage-two loops
    {"%s_%s:%s" % (F, T, t) for F in ("pass_a", "pass_b") for T in ("f64", "f32") for t in (
        "n=0", "one_ragged_tile", "exact_tile_edge", "ragged_last_tile", "full_grid_one_trip", "second_trip", "second_trip_ragged_last_tile",
        "wpc=8", "wpc=7", "wpc=2", "last_k_of_wpc=8", "first_k_of_wpc=7", "k=1", "k=2", "k=3", "k=4", "k=5", "k=255", "k=256",
        "stage2<=256", "stage2>256", "ld=n", "ld>n", "k=0 refused", "k>kmax refused")} |
    {"%s_f64:%s" % (F, t) for F in ("pass_a", "pass_b") for t in ("wpc=1", "last_k_of_wpc=2", "first_k_of_wpc=1")} |
    # pass C
    {"pass_c_%s:%s" % (T, t) for T in ("f64", "f32") for t in (
        "n=0", "ragged", "exact", "more_workgroups", "second_trip", "k=1", "k=7", "k=8", "k=9", "k=256", "mode=dst", "mode=w", "ld=n", "ld>n",
        "k=0 refused", "k>kmax refused")} |
    {"pass_c_f64:mode=basis", "pass_c_f64:basis_mode_with_padding"} |
    # the batched passes
    {"%s_%s:%s" % (F, T, t) for F in PASS_MV_OPS for T in ("f64", "f32") for t in (
        "nb=1", "nb=2", "nb=3", "nb=4", "largest_k_not_first", "misaligned_column", "aligned_column", "ld=n", "ld>n")} |
    {"%s_%s:%s" % (F, T, t) for F in ("pass_a_mv", "pass_b_mv") for T in ("f64", "f32") for t in ("different_own_grids", "early_exit_and_second_trip")} |
    {"pass_c_mv_%s:mode=%s" % (T, t) for T in ("f64", "f32") for t in ("dst", "w")} |
    {"%s_f64:%s" % (F, t) for F in PASS_MV_OPS for t in ("nb=0 refused", "nb=5 refused", "k=0 refused", "k>kmax refused")} |
    # the projection and the border product
    {"%s:%s" % (F, t) for F in PROJ_OPS for t in
     ["m=%d" % m for m in PROJ_M] + ["chunk_tail=%d" % t for t in range(1, 9)] + ["chunks=%d" % c for c in (1, 2, 3, 4)] +
     ["n=1", "ragged", "more_workgroups", "second_trip", "ld=n", "ld>n", "both_forms", "m=0 refused", "m>max refused", "n=0 refused",
      "ld<n refused"]})
