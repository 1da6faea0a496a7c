"""The GPU run of the level-solve lab in a process of its own (tests/test_lvllab_gpu.py starts it with a time limit):
every case of tests/lvllab/cases.py on the product library.
  python tests/lvllab/child.py OUT.json
Writes {case: {"failures": [...], "kinds": [...], "lds_bytes_nv4": n}} after every case; exit status 0 when it ran to its end."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import cases as lc  # noqa: E402


def main():
    out = sys.argv[1]
    lab = lc.load("gpu")
    rec = {}
    for case in lc.CASES:
        R = lc.run_case(lab, case, groups=(None, 1, 2))
        rec[case.name] = {"failures": lc.exact_failures(case, R) + lc.bound_failures(case, R), "kinds": sorted(lc.task_kinds(R)),
                          "lds_bytes_nv4": 32 * R["T"]["lds"]}
        with open(out + ".tmp", "w") as f:
            json.dump(rec, f)
        os.replace(out + ".tmp", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
