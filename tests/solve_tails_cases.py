"""Cases, runner and fixture layout of tests/test_solve_tails_gpu.py (bitwise equality of the solve kernels with recorded
results) -- shared with tools/record_solve_tails.py, which records the fixtures under tests/golden/solve_tails/.

Inputs come from the seeded generators of tests/fusedlab/cases.py and tests/frontlab/cases.py (imported, nothing added to
them); the shapes those lists lack are built here with the same generators.  The cases are the smallest that reach every
k loop of k_interior_fused / k_interior_fused_io / k_interior_fused_mv, fused_spmv_rows and k_lvl_fwd / k_lvl_bwd with
every leftover count behind the unrolled part."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "solve_tails")


def _load(key, path):
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, path)
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


fc = _load("fusedlab_cases", os.path.join(HERE, "fusedlab", "cases.py"))
fl = fc.fl

# ------------------------------------------------------------------ fused interior solve (tests/fusedlab)
# one dense front of w columns: fw_ni = bw_ni = w, so 64 / 65, 128 / 129 and 255 / 256 sit on both sides of the k-split and
# of the second trip of the item loop; the trees add ri % 4 != 0, levels of more than 256 items and the A12 lane counts
_FROM_LAB = ("dense_w7", "dense_w64", "dense_w65", "dense_w128", "dense_w129", "dense_w203", "arrow_2x5_top3",
             "arrow_3x9_top6", "arrow_4x16_top21", "grid7_8")
_STEPS = ("mv", "f32", "io")
FUSED_CASES = [fc.Case(n, fc.BY_NAME[n].classes, a_lanes=fc.BY_NAME[n].a_lanes, steps=_STEPS) for n in _FROM_LAB] + [
    fc.Case("dense_w255", [fc.ClassSpec("dense", (255, 2), leaf=255)], a_lanes=4, steps=_STEPS),
    fc.Case("dense_w256", [fc.ClassSpec("dense", (256, 1), leaf=256, nb=2)], a_lanes=8, steps=_STEPS),
]
# tags of fusedlab's coverage() the list has to reach
FUSED_TAGS = ({"wide_tail%%4=%d" % t for t in range(4)} | {"ksplit4_tail!=0", "ksplit2_tail!=0", "ri=0", "ri%4!=0", "packed", "unpacked"}
              | {"%s_ni%s" % (d, t) for d in ("fw", "bw") for t in ("<=64", "=64", "=65", "=128", "=129", ">256")})
FUSED_NV = 4            # vectors kept per case (x_single[:4]: _mv with nv 2 and 4 solve the same columns)
FUSED_NV32 = 2


def fused_results(lab, case):
    """(what is compared with the fixture, the whole result of fusedlab's run_case)."""
    R = fc.run_case(lab, case)
    out = {"x": R["x_single"][:FUSED_NV], "x_f32": R["x_f32"][:FUSED_NV32],
           "io_x10": R["io_x10_fused"], "io_user": R["io_user_fused"]}
    return out, R


def fused_failures(case, R, gold):
    """Messages; empty: every solve has the recorded bits."""
    bad = []

    def same(what, a, b):
        if not fc.same_bits(a, b):
            bad.append("%s: %s differs from the recorded result" % (case.name, what))

    same("k_interior_fused<double>", R["x_single"][:FUSED_NV], gold["x"])
    same("k_interior_fused_mv<2>", R["x_mv2"], gold["x"][:2])
    same("k_interior_fused_mv<4>", R["x_mv4"], gold["x"][:4])
    same("k_interior_fused<float>", R["x_f32"][:FUSED_NV32], gold["x_f32"])
    same("k_interior_fused_mv<2, float> (+ single)", R["x_mv3_f32"][:FUSED_NV32], gold["x_f32"])
    same("k_interior_fused_io<1, 0>", R["io_x10_fused"], gold["io_x10"])
    same("k_interior_fused_io<2, 1>", R["io_user_fused"], gold["io_user"])
    return bad


# ------------------------------------------------------------------ merged level solve (tests/frontlab, MergedSolve)
LVL_NRHS = 7            # column groups 4 + 2 + 1: k_lvl_*<4>, <2> and <1> in one solve


def _lvl(name, kind, args, leaf):
    return fl.Case("tails_" + name, kind, args, leaf=leaf, merged=True, nrhs=LVL_NRHS)


LVL_CASES = (
    # whole-front tasks: small fronts of 1 .. 9 columns (backward pivot loops of 1 .. 9 entries) with 1 .. 20 update rows
    # (ri % 4 of every kind) and top fronts with ri = 0
    [_lvl("arrow_a%d" % a, "arrow", (2, a, a + 2, 2), a) for a in range(1, 10)] + [_lvl("dense_w8", "dense", (8, 2), 8)]
    # tile tasks (more than 256 rows): one front of W columns, ri = 0 -- the last wave's column range ends W % 8 = 1 .. 7
    # entries behind its unrolled part in both sweeps
    + [_lvl("dense_w%d" % w, "dense", (w, 2), w) for w in range(257, 264)]
    # tile tasks with ri % 4 != 0: leaves of 21 columns and 243 update rows (pivot part 16 + 5, U-side part 51 = 48 + 3 in
    # the first wave), and a whole-front top of 243 columns
    # (top = 241 and 247: the first leaf's last wave ends 3 and 1 entries behind its unrolled U-side part)
    + [_lvl("arrow_21_top%d" % t, "arrow", (2, 21, t, 4), 21) for t in (243, 241, 247)]
)


def lvl_results(fn, case):
    pat = case.pattern()
    vals = [case.values(pat, b) for b in range(case.nb)]
    rhs = np.stack([case.rhs(pat, b) for b in range(case.nb)])
    return fl.run(fn, pat, vals, rhs, case.leaf, case.max_width, case.big_panel, 0, True)


def lvl_failures(case, res, gold):
    bad = []
    if not res["merged"]:
        bad.append("%s: not solved by MergedSolve" % case.name)
    if res["flag"] or res["canary"]:
        bad.append("%s: flag %d canary %d" % (case.name, res["flag"], res["canary"]))
    if not fc.same_bits(res["x"], gold["x"]):
        bad.append("%s: k_lvl_fwd / k_lvl_bwd differ from the recorded result" % case.name)
    return bad


def lvl_shapes(results):
    """What the front tables say the k_lvl_* kernels ran: {(kind, w, ri)} with kind 'whole' or 'tile'."""
    got = set()
    for res in results:
        for w, ri in res["fronts"][:, :2]:
            got.add(("whole" if w + ri <= fl.LVL_SMALL_ROWS else "tile", int(w), int(ri)))
    return got


def lvl_tile_tails(w, ri):
    """Leftover entries behind the unrolled-by-eight part of every wave of every tile task of a front, by the index
    arithmetic of k_lvl_fwd / k_lvl_bwd restated: {(loop, leftover)} with loop 'fwd', 'bwd_pivot' or 'bwd_uside'."""
    got, rows = set(), w + ri
    for r0 in range(0, rows, 64):
        kneed = min(w, r0 + 63)
        chunk = (kneed + 31) // 32 * 8
        for g in range(4):
            kb, ke = g * chunk, min(g * chunk + chunk, kneed)
            if ke > kb:
                got.add(("fwd", (ke - kb) % 8))
    for r0 in range(0, w, 64):
        nU = w - r0
        total = nU + ri
        chunk = (total + 31) // 32 * 8
        for g in range(4):
            kb, ke = g * chunk, min(g * chunk + chunk, total)
            e = min(ke, nU)
            if e > kb:
                got.add(("bwd_pivot", (e - kb) % 8))
            if ke > max(kb, nU):
                got.add(("bwd_uside", (ke - max(kb, nU)) % 8))
    return got


# ------------------------------------------------------------------ fixtures
def golden_path(family, case):
    return os.path.join(GOLDEN, "%s_%s.npz" % (family, case.name))


def load_golden(family, case):
    with np.load(golden_path(family, case)) as z:
        return {k: z[k] for k in z.files}


def run_all(out_dir, which="gpu", full=True):
    """Every case through the harnesses; writes <out_dir>/<family>_<case>.npz (the fixture layout) and, with full,
    <out_dir>/full_<case>.npz (all of fusedlab's run_case: the multi-vector and FP32 results, the plan tables)."""
    import time
    os.makedirs(out_dir, exist_ok=True)
    lab = fc.load(which)
    for case in FUSED_CASES:
        t0 = time.time()
        out, R = fused_results(lab, case)
        np.savez(os.path.join(out_dir, "fused_%s.npz" % case.name), **out)
        if full:
            np.savez(os.path.join(out_dir, "full_%s.npz" % case.name), **R)
        print("solve_tails: fused %-20s %.2f s" % (case.name, time.time() - t0), flush=True)
    fn = fl.load(which)
    for case in LVL_CASES:
        t0 = time.time()
        res = lvl_results(fn, case)
        np.savez(os.path.join(out_dir, "lvl_%s.npz" % case.name), x=res["x"], fronts=res["fronts"],
                 info=np.array([res["merged"], res["flag"], res["canary"]], dtype=np.int64))
        print("solve_tails: lvl   %-20s merged %d  %.2f s" % (case.name, res["merged"], time.time() - t0), flush=True)


if __name__ == "__main__":      # the child process of tests/test_solve_tails_gpu.py: python solve_tails_cases.py OUT_DIR [sim]
    run_all(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "gpu")
