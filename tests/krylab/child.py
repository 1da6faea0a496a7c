"""The run of every case of tests/krylab/cases.py in one process: through the product library (libkrylab_gpu.so) for
tests/test_krylab_gpu.py, which starts it with a time limit, or through the simulator build.  Writes the whole output
buffers of every case to <out>/<case>.npz and the coverage tags to <out>/coverage.txt.  The kernels read no environment
switches, so one process serves all cases.  A batched case also runs the single launcher on every column's operands and
stores whether the digests agree, so that both launches come from this one process.

usage: python child.py OUT_DIR [sim]"""
import importlib.util
import os
import sys
import time

import numpy as np

LAB = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    """tests/krylab/<name>.py as module krylab_<name> (the other labs have modules of the same file names)."""
    key = "krylab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


kl = _load("cases")


def main():
    out, which = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "gpu")
    os.makedirs(out, exist_ok=True)
    lib = kl.load(which)
    t_all = time.time()
    for case in kl.CASES:
        inp = kl.inputs(case, keep=False)
        t0 = time.time()
        res = kl.FAMILIES[case.family][1](lib, case, inp)
        dt = time.time() - t0
        np.savez(os.path.join(out, case.name + ".npz"), **res)
        print("krylab: %-34s %.3f s" % (case.name, dt), flush=True)
    tags = sorted(kl.coverage(lib, kl.CASES))
    with open(os.path.join(out, "coverage.txt"), "w") as f:
        f.write("\n".join(tags) + "\n")
    print("krylab: all %d cases in %.1f s" % (len(kl.CASES), time.time() - t_all), flush=True)


def load(out, case):
    """The output buffers of one case as written by main()."""
    with np.load(os.path.join(out, case.name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def load_coverage(out):
    with open(os.path.join(out, "coverage.txt")) as f:
        return set(f.read().split("\n")) - {""}


if __name__ == "__main__":
    main()
