"""One process per environment variant of tests/test_fusedlab_gpu.py: runs the demote / round shapes and every case through
the product library (libfusedlab_gpu.so) and writes the results to <out>/<case>.npz and <out>/demote.txt.  The switches of
the library are read per process, which is why every variant is a process of its own.

usage: python child.py OUT_DIR [sim]"""
import importlib.util
import os
import sys
import time

import numpy as np

LAB = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    """tests/fusedlab/<name>.py as module fusedlab_<name> (the other labs have modules of the same file names)."""
    key = "fusedlab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


def main():
    fc = _load("cases")
    out, which = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "gpu")
    os.makedirs(out, exist_ok=True)
    lab = fc.load(which)
    with open(os.path.join(out, "demote.txt"), "w") as f:
        f.write("\n".join(fc.demote_failures(lab)))
    for case in fc.CASES:
        if which == "sim" and not case.sim:
            continue
        t0 = time.time()
        R = fc.run_case(lab, case)
        np.savez(os.path.join(out, case.name + ".npz"), **R)
        print("fusedlab: %-24s LDS %6d doubles  %.2f s" % (case.name, int(R["lds"][0]), time.time() - t0), flush=True)


def load(out, case):
    """The results of one case as written by main() (the dict of cases.run_case)."""
    with np.load(os.path.join(out, case.name + ".npz")) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    main()
