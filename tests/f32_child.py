"""One group of GPU checks of the FP32 panel storage in a process of its own (tests/test_f32_panels_gpu.py starts it with
a time limit): runs the check of tests/f32_cases.py on the product library and writes a JSON record.
  python tests/f32_child.py GROUP OUT.json
Exit status 0 whenever the check ran to its end, passed or not; anything else means the process itself failed."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hymls_amd  # noqa: E402
import f32_cases as fc  # noqa: E402
from common import problem, xml_params  # noqa: E402


def check_memory(lib, dev):
    """case 5 on the device: Stokes-C 64^3 three-level, free device memory (hipMemGetInfo through torch) after Compute with
    FP32 storage exceeds the FP64 figure of the same handle by at least 90 % of half the demoted panel bytes (the 10 %
    is room for allocator granularity).  One handle, 64 -> 32 -> 64."""
    A, tv = problem("Stokes-C", 64)
    prm = xml_params("Stokes-C", 64, 8, 2, partitioner="Skew Cartesian")
    P = hymls_amd.Preconditioner(A, prm, testVector=tv, lib=lib)
    free, b1, b4, r9 = {}, {}, {}, {}
    for step, storage in enumerate(("double", "single", "double")):
        P.SetFactorStorage(storage)
        P.Compute()
        torch.cuda.synchronize()
        free[step] = torch.cuda.mem_get_info()[0]
        b1[step], b4[step], r9[step] = P.apply_bytes(1), P.apply_bytes(4), P.apply_bytes(9)
    saved = ((b1[0] - b1[1]) + (b4[0] - b4[1])) / 2
    print("f32 panels memory Stokes-C 64^3: resident panel bytes %.0f (FP64) %.0f (FP32), model saving %.0f; free device memory "
          "%d / %d / %d bytes" % (r9[0], r9[1], saved, free[0], free[1], free[2]), flush=True)
    assert saved > 0 and r9[1] == r9[0] - saved and r9[2] == r9[0]
    assert free[1] - free[0] >= 0.9 * saved, (free, saved)
    assert free[1] - free[2] >= 0.9 * saved, (free, saved)
    return {"resident_fp64": r9[0], "resident_fp32": r9[1], "free": [free[0], free[1], free[2]]}


def main():
    group, out = sys.argv[1], sys.argv[2]
    lib = hymls_amd.load_library()
    dev = "cuda"
    rec = {"group": group, "ok": False, "message": "", "figures": None}
    try:
        if group.startswith("case:"):
            rec["figures"] = fc.check_case(lib, dev, fc.CASES[fc.CASE_IDS.index(group[5:])])
        elif group == "defaults_lifecycle":
            fc.check_defaults(lib, dev)
            fc.check_lifecycle(lib, dev)
        elif group == "python_xml":
            fc.check_python_and_xml(lib, dev, os.path.dirname(os.path.abspath(out)))
        elif group == "solver32":
            rec["figures"] = fc.check_solver(lib, dev, 32)
        elif group == "solver64":
            rec["figures"] = fc.check_solver(lib, dev, 64)
        elif group == "memory64":
            rec["figures"] = check_memory(lib, dev)
        else:
            raise SystemExit("unknown group " + group)
        rec["ok"] = True
    except (AssertionError, hymls_amd.HymlsError, RuntimeError):
        rec["message"] = traceback.format_exc()[-3000:]
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(rec, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
