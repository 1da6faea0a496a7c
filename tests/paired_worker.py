"""Child process of tests/test_paired_panels_gpu.py: every case twice through the product library (tests/fusedlab), once with
packed panels and once with the panels of the wide levels in column pairs (HYMLS_MI_FORCE_PAIRED_PANELS, read by
BatchedLU::upload when the class is planned), same values, same right-hand sides.  Writes <out>/<case>.npz.

usage: python paired_worker.py OUT_DIR"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import paired_cases as pc  # noqa: E402

fc = pc.fc
SWITCH = "HYMLS_MI_FORCE_PAIRED_PANELS"
NV = (2, 3, 5)


def run_case(lab, case):
    lab.reset()
    R = {}
    pats = [c.pattern() for c in case.classes]
    xoffs, off = [], 0
    for c, pat in zip(case.classes, pats):
        xoffs.append([off + b * (pat.nI + fc.GAP) for b in range(c.nb)])
        off += c.nb * (pat.nI + fc.GAP)
    n = off
    os.environ.pop(SWITCH, None)
    tabs = {"packed": [lab.plan(pat, xo, c.leaf, c.max_width, True) for c, pat, xo in zip(case.classes, pats, xoffs)]}
    os.environ[SWITCH] = "1"
    tabs["paired"] = [lab.plan(pat, xo, c.leaf, c.max_width, True) for c, pat, xo in zip(case.classes, pats, xoffs)]
    os.environ.pop(SWITCH, None)
    inside = np.zeros(n, dtype=bool)
    for T in tabs["packed"]:
        for o in T["xoff"]:
            inside[o: o + T["nI"]] = True
    B = fc.canary_vector((max(NV), n))
    B[:, inside] = fc.rng_of(case, "rhs").uniform(-1.0, 1.0, (max(NV), int(inside.sum())))
    R["n"], R["rhs"] = np.array(n), B
    flags = []
    for layout in ("packed", "paired"):
        subs = []
        for ci, (c, pat, T) in enumerate(zip(case.classes, pats, tabs[layout])):
            assert T["fits"], "%s: class %d outside fused_solve_fits" % (case.name, ci)
            for key in ("fronts", "fw_ptr", "bw_ptr"):
                R["c%d_%s" % (ci, key)] = T[key]
            kval = np.concatenate([fc.class_values(case, ci, pat, b)[pat.rows, pat.cols] for b in range(c.nb)])
            U, flag, guard = lab.factor(T, kval)
            flags += [flag, int(not guard)]
            P, guard = lab.repack(T, 0, c.nb)
            flags.append(int(not guard))
            R["c%d_slab" % ci], R["c%d_%s" % (ci, layout)] = U, P
            subs += [(T["id"], b, int(o)) for b, o in enumerate(T["xoff"])]

        def solve(kind, x, storage=0):
            y, guard, _ = lab.solve(kind, subs, x, n, storage)
            flags.append(int(not guard))
            return y

        R["x_%s" % layout] = solve(0, B[0])[0]
        for nv in NV:
            R["x_mv%d_%s" % (nv, layout)] = solve(2, B[:nv])
        for ci, T in enumerate(tabs[layout]):
            _, fl32, guard = lab.storage(T, 1)
            flags += [fl32, int(not guard)]
        R["x_f32_%s" % layout] = solve(1, B[0])[0]
        R["x_mv3_f32_%s" % layout] = solve(3, B[:3])
        io = fc.io_run(lab, case, subs, tabs[layout])
        flags += [int(not g) for g in io["guards"]]
        R["io10_%s" % layout], R["io21_%s" % layout] = io["x10_fused"], io["user_fused"]
        xt = B[0].copy()
        for T in tabs[layout]:
            xt, guard = lab.transposed(T, xt)
            flags.append(int(not guard))
        R["x_transposed_%s" % layout] = xt
    R["flags"] = np.array(flags, dtype=np.int64)     # factor flags and guards written: all zero when all is well
    lab.reset()
    return R


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    lab = fc.load("gpu")
    for case in pc.CASES:
        t0 = time.time()
        np.savez(os.path.join(out, case.name + ".npz"), **run_case(lab, case))
        print("paired panels: %-24s %.2f s" % (case.name, time.time() - t0), flush=True)


def load(out, case):
    with np.load(os.path.join(out, case.name + ".npz")) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    main()
