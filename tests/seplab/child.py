"""One process per environment variant of tests/test_seplab_gpu.py: runs every case of the variant through the product
library (libseplab_gpu.so) and writes the whole output buffers to <out>/<case>.npz.  The switches of the library
(HYMLS_MI_INVERT_BLOCKED_MIN, HYMLS_MI_MV_GROUP_BLK) are read once per process, which is why every variant is a process of
its own.

usage: python child.py OUT_DIR VARIANT [sim]"""
import importlib.util
import os
import sys
import time

import numpy as np

LAB = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    """tests/seplab/<name>.py as module seplab_<name> (tests/frontlab has modules of the same file names)."""
    key = "seplab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


sl = _load("cases")


def main():
    out, variant, which = sys.argv[1], sys.argv[2], (sys.argv[3] if len(sys.argv) > 3 else "gpu")
    os.makedirs(out, exist_ok=True)
    lib = sl.load(which)
    for case in sl.cases_of(variant):
        if which == "sim" and not case.sim:
            continue
        sl.inputs(case)
        t0 = time.time()
        res = sl.run_case(lib, case)
        dt = time.time() - t0
        np.savez(os.path.join(out, case.name + ".npz"), **res)
        print("seplab: %-28s %.3f s" % (case.name, dt), flush=True)
    tags = sorted(sl.coverage(lib, [c for c in sl.cases_of(variant) if which != "sim" or c.sim]))
    with open(os.path.join(out, "coverage.txt"), "w") as f:
        f.write("\n".join(tags) + "\n")


def load(out, case):
    """The output buffers of one case as written by main()."""
    with np.load(os.path.join(out, case.name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def load_coverage(out):
    with open(os.path.join(out, "coverage.txt")) as f:
        return set(f.read().split("\n")) - {""}


if __name__ == "__main__":
    main()
