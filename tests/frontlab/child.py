"""One process per environment variant of tests/test_frontlab_gpu.py: runs every case through the product library
(libfrontlab_gpu.so) and writes the results to <out>/<case>.npz.  The switches of the library (HYMLS_MI_GEMM_TILE, ...) are
read once per process, which is why every variant is a process of its own.

usage: python child.py OUT_DIR [sim]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases as fl  # noqa: E402


def main():
    out, which = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "gpu")
    os.makedirs(out, exist_ok=True)
    fn = fl.load(which)
    for case in fl.CASES:
        if which == "sim" and not case.sim:
            continue
        t0 = time.time()
        res = fl.run_case(fn, case)
        arrays = {}
        for run, r in res.items():
            for key in ("S", "x", "fronts"):
                arrays[run + "_" + key] = r[key]
            arrays[run + "_info"] = np.array([r["chunk"], r["merged"], r["flag"], r["canary"], r["passes"]], dtype=np.int64)
            arrays[run + "_growth"] = np.array([r["growth"]])
        np.savez(os.path.join(out, case.name + ".npz"), **arrays)
        print("frontlab: %-28s flag %d canary %d  %.2f s" % (case.name, res["main"]["flag"], res["main"]["canary"],
                                                             time.time() - t0), flush=True)


def load(out, case):
    """The runs of one case as written by main() (the dicts of cases.run)."""
    z = np.load(os.path.join(out, case.name + ".npz"))
    res = {}
    for run in ("main", "chunked", "alone"):
        if run + "_info" not in z:
            continue
        info = z[run + "_info"]
        res[run] = {"S": z[run + "_S"], "x": z[run + "_x"], "fronts": z[run + "_fronts"], "chunk": int(info[0]),
                    "merged": int(info[1]), "flag": int(info[2]), "canary": int(info[3]), "passes": int(info[4]),
                    "growth": float(z[run + "_growth"][0])}
    return res


if __name__ == "__main__":
    main()
