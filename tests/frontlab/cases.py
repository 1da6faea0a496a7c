"""Front-level test cases of the batched multifrontal LU (tests/frontlab/front_harness.cpp).

Pattern generators (dense block, nested / arrowhead, grid subdomain with a separator shell, saddle point), random
nonsymmetric diagonally dominant values (one seed per member), a float64 LAPACK reference of the separator block
S = A22 - A21 A11^{-1} A12 and of A11 x = b, the ctypes driver of the harness and the coverage bookkeeping that reads the
front table the harness returns.  Shared by tests/test_frontlab.py (host simulator) and tests/test_frontlab_gpu.py
(product library, through tests/frontlab/child.py)."""
import ctypes
import os
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"sim": os.path.join(HERE, "libfrontlab_sim.so"), "gpu": os.path.join(HERE, "libfrontlab_gpu.so")}

C_TOL = 8.0                 # the one constant of every error bound below (not tuned per case)
EPS = 2.0 ** -52

# thresholds of the product code the coverage bookkeeping mirrors (device_hip.hip / device.hpp)
PIECE = 128                 # columns of a pivot piece (factor_big_front)
OUTER = 512                 # outer block of the wide factorisation (default of HYMLS_MI_OUTER_BLOCK)
LVL_SMALL_ROWS = 256        # fronts with more rows are cut into 64-row tasks by the merged solve
BIG_PANEL = 1 << 40         # analyse_class default: no panel-size limit


# ------------------------------------------------------------------ patterns
class Pattern:
    """Extended local pattern: nI interior rows first, then nS separator rows; `mask` is the dense n x n structure."""

    def __init__(self, nI, nS, mask, zero_diag, coord):
        self.nI, self.nS = nI, nS
        self.mask = mask
        self.zero_diag = np.asarray(zero_diag, dtype=np.int8)
        self.coord = np.ascontiguousarray(coord, dtype=np.int32).reshape(-1)
        rows, cols = np.nonzero(mask)
        self.rows, self.cols = rows, cols
        self.rowptr = np.zeros(nI + nS + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows, minlength=nI + nS), out=self.rowptr[1:])
        self.col = cols.astype(np.int32)


def _with_diag(mask, zero_diag):
    n = mask.shape[0]
    d = np.ones(n, dtype=bool)
    d[: len(zero_diag)] = ~np.asarray(zero_diag, dtype=bool)
    mask[np.arange(n), np.arange(n)] = d
    return mask


def dense_block(w, nS):
    """nI = w fully coupled unknowns, nS separator rows coupled to all of them and to each other."""
    n = w + nS
    mask = np.ones((n, n), dtype=bool)
    coord = np.zeros((w, 3), dtype=np.int32)
    coord[:, 0] = np.arange(w)
    return Pattern(w, nS, mask, np.zeros(w, np.int8), coord)


def arrowhead(nleaf, a, top, nS):
    """nleaf dense leaf blocks of a unknowns, each coupled to a dense top block of `top` unknowns; the separator rows
    couple to the top block and to the first unknown of every leaf."""
    nI = nleaf * a + top
    n = nI + nS
    mask = np.zeros((n, n), dtype=bool)
    for j in range(nleaf):
        s = slice(j * a, (j + 1) * a)
        mask[s, s] = True
        mask[s, nleaf * a: nI] = True
        mask[nleaf * a: nI, s] = True
    mask[nleaf * a: nI, nleaf * a: nI] = True
    if nS:
        mask[nI:, nleaf * a: nI] = True
        mask[nleaf * a: nI, nI:] = True
        firsts = np.arange(nleaf) * a
        mask[nI:, firsts] = True
        mask[firsts, nI:] = True
        mask[nI:, nI:] = True
    coord = np.zeros((nI, 3), dtype=np.int32)
    coord[:, 0] = np.arange(nI)
    return Pattern(nI, nS, _with_diag(mask, np.zeros(nI)), np.zeros(nI, np.int8), coord)


def grid_box(nx, ny, nz, stencil):
    """7- or 27-point stencil on an nx x ny x nz box of interior cells; the separator is the one-cell shell around it."""
    full = [(i, j, k) for k in range(-1, nz + 1) for j in range(-1, ny + 1) for i in range(-1, nx + 1)]
    inside = [c for c in full if 0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz]
    if stencil == 7:
        offs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    else:
        offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    inside_set = set(inside)
    shell = sorted({(c[0] + o[0], c[1] + o[1], c[2] + o[2]) for c in inside for o in offs} - inside_set,
                   key=lambda c: (c[2], c[1], c[0]))
    nodes = inside + shell
    idx = {c: t for t, c in enumerate(nodes)}
    nI, nS = len(inside), len(shell)
    n = nI + nS
    mask = np.zeros((n, n), dtype=bool)
    for c in nodes:
        t = idx[c]
        for o in offs:
            u = idx.get((c[0] + o[0], c[1] + o[1], c[2] + o[2]))
            if u is not None and (t < nI or u < nI):
                mask[t, u] = mask[u, t] = True
    mask[np.arange(n), np.arange(n)] = True
    coord = np.array(inside, dtype=np.int32) * 2
    return Pattern(nI, nS, mask, np.zeros(nI, np.int8), coord)


def saddle(nc, nS):
    """Staggered velocity / pressure pairs on nc^3 cells: a velocity on every cell face (boundary faces included) couples
    to the velocities of its direction around it and to the one or two pressures beside it; the pressure rows have no
    diagonal.  nS separator rows couple to the velocities of the faces on the x = 0 boundary."""
    vel = []
    for d in range(3):
        for k in range(nc + (d == 2)):
            for j in range(nc + (d == 1)):
                for i in range(nc + (d == 0)):
                    vel.append((d, i, j, k))
    cells = [(i, j, k) for k in range(nc) for j in range(nc) for i in range(nc)]
    nv, npr = len(vel), len(cells)
    nI = nv + npr
    n = nI + nS
    vidx = {v: t for t, v in enumerate(vel)}
    cidx = {c: nv + t for t, c in enumerate(cells)}
    mask = np.zeros((n, n), dtype=bool)
    sign = np.zeros((n, n))   # divergence / gradient signs of the velocity-pressure couplings
    coord = np.zeros((nI, 3), dtype=np.int32)
    for t, (d, i, j, k) in enumerate(vel):
        p = [2 * i, 2 * j, 2 * k]
        p[d] -= 1
        coord[t] = p
        for e in range(3):
            for s in (-1, 1):
                q = [i, j, k]
                q[e] += s
                u = vidx.get((d, q[0], q[1], q[2]))
                if u is not None:
                    mask[t, u] = mask[u, t] = True
        for s in (-1, 0):   # the cells on both sides of the face
            q = [i, j, k]
            q[d] += s
            if all(0 <= q[e] < nc for e in range(3)):
                c = cidx[tuple(q)]
                mask[t, c] = mask[c, t] = True
                sign[t, c] = sign[c, t] = 1.0 if s else -1.0
    for t, c in enumerate(cells):
        coord[nv + t] = [2 * c[0], 2 * c[1], 2 * c[2]]
    zd = np.zeros(nI, dtype=np.int8)
    zd[nv:] = 1
    x0 = [vidx[(0, 0, j, k)] for k in range(nc) for j in range(nc)]
    for s in range(nS):
        for t in x0[s % len(x0):: max(1, nS)] + [x0[(s * 7) % len(x0)]]:
            mask[nI + s, t] = mask[t, nI + s] = True
    mask[nI:, nI:] = True
    pat = Pattern(nI, nS, _with_diag(mask, zd), zd, coord)
    pat.vp_sign = sign
    return pat


PATTERNS = {"dense": dense_block, "arrow": arrowhead, "grid": grid_box, "saddle": saddle}


# ------------------------------------------------------------------ values
def member_values(pat, seed, tweak=None):
    """Dense n x n values on the pattern: off-diagonal entries uniform in (-1, 1), a diagonal 1.5 x the absolute row sum
    + 1 (nonsymmetric, diagonally dominant: cond(A11) stays small); rows without a diagonal keep none.  tweak(V, pat):
    the flag cases overwrite a few entries."""
    rng = np.random.default_rng(seed)
    n = pat.nI + pat.nS
    V = np.where(pat.mask, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    d = np.arange(n)
    V[d, d] = 0.0
    zd = np.zeros(n, dtype=bool)
    zd[: pat.nI] = pat.zero_diag != 0
    if zd.any():   # velocity-pressure couplings of magnitude 1 .. 2: the pressure Schur complement stays well away from zero
        vp = pat.mask & (zd[:, None] != zd[None, :])
        V[vp] = pat.vp_sign[vp] * (1.0 + np.abs(V[vp]))
    diag = 1.5 * np.abs(V).sum(axis=1) + 1.0
    has = pat.mask[d, d]
    V[d[has], d[has]] = diag[has]
    if tweak is not None:
        tweak(V, pat)
    return V


def seed_of(name, b):
    return (zlib.crc32(name.encode()) + 7919 * b) & 0x7fffffff


def zero_pivot(V, pat):
    V[0, 0] = 0.0


def tiny_pivot(V, pat):
    # the first pivot 1e-12 against couplings of 1: u_11 ~ 1e12, growth far above 1e8
    V[0, 0] = 1e-12
    V[0, 1] = V[1, 0] = 1.0


TWEAKS = {None: None, "zero": zero_pivot, "growth": tiny_pivot}


# ------------------------------------------------------------------ the case list
class Case:
    def __init__(self, name, kind, args, nb=1, leaf=None, max_width=256, big_panel=BIG_PANEL, chunk=0, nrhs=1,
                 merged=False, sim=True, tweak=None, repro=False):
        self.name, self.kind, self.args = name, kind, args
        self.nb, self.max_width, self.big_panel, self.chunk = nb, max_width, big_panel, chunk
        self.nrhs, self.merged, self.sim, self.tweak, self.repro = nrhs, merged, sim, tweak, repro
        self.leaf = leaf if leaf is not None else (args[0] if kind == "dense" else 24)

    def pattern(self):
        return PATTERNS[self.kind](*self.args)

    def values(self, pat, b):
        return member_values(pat, seed_of(self.name, b), TWEAKS[self.tweak])

    def rhs(self, pat, b):
        return np.random.default_rng(seed_of(self.name, 1000 + b)).uniform(-1.0, 1.0, (self.nrhs, pat.nI))

    def __repr__(self):
        return self.name


WIDE = 16   # max_width that sends every front wider than 16 columns to the multi-workgroup path


def _dense(w, nS, **kw):
    return Case("dense_w%d_s%d%s" % (w, nS, "_" + kw["tweak"] if kw.get("tweak") else "") + ("_wide" if kw.get("max_width") == WIDE else ""),
                "dense", (w, nS), **kw)


CASES = [
    # one-workgroup fronts (k_factor_level): LDS variants 3072 (w <= 54) / 6144 (55..77), global memory (78..256)
    _dense(1, 3, nb=3),
    _dense(54, 4, nb=3, nrhs=2),
    _dense(55, 0),
    _dense(77, 5, nb=3),
    _dense(78, 5),
    _dense(256, 8, nrhs=3),
    # wide fronts: pivot pieces of both kernels, last pieces of w % 128 columns, outer blocks of 512
    _dense(17, 5, nb=3, max_width=WIDE, repro=True, chunk=2),
    _dense(64, 0, max_width=WIDE),
    _dense(65, 3, max_width=WIDE, nrhs=2),
    _dense(96, 20, max_width=WIDE),
    _dense(97, 7, max_width=WIDE),
    _dense(128, 2, max_width=WIDE, nb=3),
    _dense(129, 33, nb=3, max_width=WIDE, repro=True, chunk=2),
    _dense(511, 12, max_width=WIDE),
    _dense(512, 100, max_width=WIDE),
    _dense(513, 9, max_width=WIDE),
    _dense(640, 64, max_width=WIDE, merged=True, nrhs=4),
    _dense(1100, 40, max_width=WIDE),
    _dense(2287, 50, max_width=WIDE, sim=False),
    _dense(3793, 30, max_width=WIDE, sim=False, merged=True, nrhs=2),
    # trees: a chain of wide fronts (wide into wide), small fronts into a wide root, grid subdomains, saddle point
    Case("chain_w1100", "dense", (1100, 16), leaf=300, max_width=WIDE),
    Case("arrow_6x24_top160", "arrow", (6, 24, 160, 12), nb=3, leaf=24, max_width=128, repro=True, chunk=2),
    Case("grid7_8", "grid", (8, 8, 8, 7), nb=3, nrhs=2, repro=True, chunk=2),
    Case("grid27_6", "grid", (6, 6, 6, 27), leaf=32, merged=True, nrhs=3),
    Case("grid7_12_merged", "grid", (12, 12, 12, 7), leaf=64, merged=True, nrhs=4, sim=False),
    Case("saddle_4", "saddle", (4, 16), nb=3, nrhs=2),
    # flags: an exactly zero pivot (bit 1) and element growth above 1e8 (bit 2), one-workgroup and wide paths
    _dense(20, 2, tweak="zero"),
    _dense(80, 2, tweak="zero"),
    _dense(20, 2, tweak="growth"),
    _dense(80, 2, tweak="growth"),
    _dense(64, 2, tweak="zero", max_width=WIDE),
    _dense(65, 2, tweak="zero", max_width=WIDE),
    _dense(64, 2, tweak="growth", max_width=WIDE),
    _dense(65, 2, tweak="growth", max_width=WIDE),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------ the harness
def build(which):
    subprocess.check_call(["make", "-s", "-C", HERE, which])
    return LIBS[which]


_loaded = {}


def load(which):
    if which not in _loaded:
        lib = ctypes.CDLL(build(which))
        f = lib.frontlab_run
        P = ctypes.c_void_p
        f.argtypes = [ctypes.c_int32, ctypes.c_int32, P, P, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int32,
                      ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P, ctypes.c_int32, P, P, P, P, P, ctypes.c_int32,
                      ctypes.c_char_p, ctypes.c_int32]
        f.restype = ctypes.c_int
        _loaded[which] = f
    return _loaded[which]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(fn, pat, vals, rhs, leaf, max_width, big_panel=BIG_PANEL, chunk=0, merged=False):
    """One call of the harness: vals [nb] dense value matrices, rhs [nb][nrhs][nI] (local order)."""
    nb, nrhs = len(vals), rhs.shape[1]
    nI, nS = pat.nI, pat.nS
    kval = np.ascontiguousarray(np.concatenate([V[pat.rows, pat.cols] for V in vals]))
    rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    sblock = np.zeros((nb, nS * nS))
    x = np.zeros((nb, nrhs, nI))
    info = np.zeros(8, dtype=np.int64)
    growth = np.zeros(1)
    fronts = np.zeros((nI + 1, 7), dtype=np.int32)
    err = ctypes.create_string_buffer(512)
    rc = fn(nI, nS, _p(pat.rowptr), _p(pat.col), _p(pat.zero_diag), _p(pat.coord), nb, _p(kval), leaf, max_width,
            big_panel, chunk, nrhs, _p(rhs), int(merged), _p(sblock), _p(x), _p(info), _p(growth), _p(fronts),
            nI + 1, err, 512)
    if rc != 0:
        raise RuntimeError("frontlab_run failed: " + err.value.decode())
    nf = int(info[0])
    return {"S": sblock.reshape(nb, nS, nS).transpose(0, 2, 1), "x": x, "fronts": fronts[:nf].copy(),
            "chunk": int(info[1]), "merged": int(info[2]), "flag": int(info[3]), "canary": int(info[4]),
            "passes": int(info[6]), "growth": float(growth[0])}


def run_case(fn, case, variant_runs=True):
    """The case itself, and for repro cases also the chunked run and member 1 factored alone."""
    pat = case.pattern()
    vals = [case.values(pat, b) for b in range(case.nb)]
    rhs = np.stack([case.rhs(pat, b) for b in range(case.nb)])
    out = {"main": run(fn, pat, vals, rhs, case.leaf, case.max_width, case.big_panel, 0, case.merged)}
    if case.repro and variant_runs:
        out["chunked"] = run(fn, pat, vals, rhs, case.leaf, case.max_width, case.big_panel, case.chunk, case.merged)
        out["alone"] = run(fn, pat, vals[1:2], rhs[1:2], case.leaf, case.max_width, case.big_panel, 0, case.merged)
    return out


# ------------------------------------------------------------------ reference and error bounds
def reference(case):
    """Per member: (A11, b, x_ref, S_ref, kappa, scale of S) with LAPACK (row pivoting) in float64."""
    pat = case.pattern()
    nI = pat.nI
    out = []
    for b in range(case.nb):
        V = case.values(pat, b)
        A11, A12, A21, A22 = V[:nI, :nI], V[:nI, nI:], V[nI:, :nI], V[nI:, nI:]
        rhs = case.rhs(pat, b)
        X = np.linalg.solve(A11, np.hstack([A12, rhs.T]))
        Y, xr = X[:, : pat.nS], X[:, pat.nS:].T
        upd = A21 @ Y
        kappa = np.linalg.cond(A11, 1)
        scale = (np.abs(A22).max() if pat.nS else 0.0) + (np.abs(upd).max() if pat.nS else 0.0)
        out.append({"A11": A11, "b": rhs, "x": xr, "S": A22 - upd, "kappa": kappa, "scale": scale})
    return out


def accuracy_failures(case, res, ref):
    """Messages of every violated bound (empty: all hold)."""
    bad = []
    nI = case.pattern().nI
    for b, r in enumerate(ref):
        k = r["kappa"]
        if r["S"].size:
            e = np.abs(res["S"][b] - r["S"]).max()
            tol = C_TOL * nI * EPS * k * r["scale"]
            if not e <= tol:
                bad.append("member %d: max|S - S_ref| = %.3e > %.3e" % (b, e, tol))
        A11 = r["A11"]
        anorm = np.abs(A11).sum(axis=1).max()
        for v in range(case.nrhs):
            x, xr, rhs = res["x"][b, v], r["x"][v], r["b"][v]
            fe = np.linalg.norm(x - xr) / np.linalg.norm(xr)
            if not fe <= C_TOL * nI * EPS * k:
                bad.append("member %d rhs %d: forward error %.3e > %.3e" % (b, v, fe, C_TOL * nI * EPS * k))
            be = np.abs(A11 @ x - rhs).max() / (anorm * np.abs(x).max())
            if not be <= C_TOL * nI * EPS:
                bad.append("member %d rhs %d: backward error %.3e > %.3e" % (b, v, be, C_TOL * nI * EPS))
    return bad


CANARY_MSG = {1: "guard tail behind the setup arena written", 2: "factor slab of a member outside the chunk changed",
              4: "non-finite or unwritten panel entry", 8: "slab entry outside every panel written"}


def canary_failures(case, res):
    mask = 1 | 2 | 8 if case.tweak else 1 | 2 | 4 | 8   # (a zero pivot legitimately leaves inf / NaN in the panels)
    return [CANARY_MSG[b] for b in (1, 2, 4, 8) if res["canary"] & mask & b]


def expected_flag(case):
    return {None: 0, "zero": 1, "growth": 2}[case.tweak]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------ coverage (from the returned front tables)
def pivot_blocked(wk):
    """k_big_pivot_blk takes the piece (factor_big_front), else k_big_pivot."""
    Wk = (wk + 31) // 32 * 32
    return wk > 96 or (wk > 16 and Wk - wk < 24)


def wide_pieces(w):
    return [min(PIECE, w - off) for off in range(0, w, PIECE)]


def trailing_updates(w, ri, rs):
    """(M = N, rank) of the trailing updates of a wide front: one per outer block with rows beyond it."""
    m = w + ri + rs
    out = []
    for o0 in range(0, w, OUTER):
        o1 = min(w, o0 + OUTER)
        if m - o1 > 0:
            out.append((m - o1, o1 - o0))
    return out


def gemm_big_tile(M, N, K, batch):
    tiles = ((M + 127) // 128) * ((N + 127) // 128) * batch
    return M > 96 and N > 96 and (K >= 256 or (K >= 64 and tiles >= 768))


def coverage(results):
    """Branches reached by a set of runs: results = [(case, res)]."""
    got = set()
    for case, res in results:
        F = res["fronts"]
        nb = case.nb
        if nb == 1:
            got.add("nb=1")
        if nb == 3:
            got.add("nb=3")
        if res["passes"] > 1:
            got.add("chunked")
        for w, ri, rs, parent, level, big, wide in F:
            got.add("ri>0" if ri > 0 else "ri=0")
            got.add("rs>0" if rs > 0 else "rs=0")
            if not wide:
                if w in (1, 54, 55, 77, 78, 256):
                    got.add("level_w=%d" % w)
                lvl_w = max(int(g[0]) for g in F if not g[6] and g[4] == level)
                ld = 3072 if lvl_w * lvl_w + 2 * lvl_w <= 3072 else 6144
                got.add("lds%d" % ld if w * w + 2 * w <= ld else "global")
                if rs > 0 and parent < 0:
                    got.add("level_root_update")
                continue
            got.add("wide_w=%d" % w)
            for wk in wide_pieces(w):
                got.add("pivot_blk" if pivot_blocked(wk) else "pivot_scalar")
                rk = w + ri + rs - wk
                if rk > 0:
                    got.add("trmm_le64" if wk <= 64 else "trmm_gt64")
            for M, K in trailing_updates(w, ri, rs):
                got.add("rank<64" if K < 64 else ("rank64-255" if K < 256 else "rank>=256"))
                got.add("gemm128" if gemm_big_tile(M, M, K, res["chunk"]) else "gemm64")
            if w > OUTER:
                got.add("outer_blocks")
            if parent < 0 and rs > 0:
                got.add("wide_root_update")
        kids = {}
        for s, row in enumerate(F):
            if row[3] >= 0:
                kids.setdefault(int(row[3]), []).append(s)
        for p, cs in kids.items():
            if F[p][6]:
                for c in cs:
                    got.add("wide_into_wide" if F[c][6] else "small_into_wide")
        if res["merged"] and any(w + ri > LVL_SMALL_ROWS for w, ri, *_ in F):
            got.add("merged_tiled")
    return got


REQUIRED_SIM = ({"level_w=%d" % w for w in (1, 54, 55, 77, 78, 256)} | {"lds3072", "lds6144", "global"}
                | {"wide_w=%d" % w for w in (17, 64, 65, 96, 97, 128, 129, 511, 512, 513, 640, 1100)}
                | {"pivot_blk", "pivot_scalar", "trmm_le64", "trmm_gt64", "rank<64", "rank64-255", "rank>=256",
                   "gemm64", "gemm128", "outer_blocks", "ri=0", "ri>0", "rs=0", "rs>0", "wide_root_update",
                   "level_root_update", "wide_into_wide", "small_into_wide", "nb=1", "nb=3", "chunked", "merged_tiled"})
REQUIRED_GPU = REQUIRED_SIM | {"wide_w=2287", "wide_w=3793"}
