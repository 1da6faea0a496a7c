"""One group of GPU checks of the FP32 storage of the merged level-solve panels in a process of its own
(tests/test_merged_f32_gpu.py starts it with a time limit): runs the check of tests/merged_f32_cases.py on the product
library and writes a JSON record.
  python tests/merged_f32_child.py GROUP OUT.json
Exit status 0 whenever the check ran to its end, passed or not; anything else means the process itself failed."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import hymls_amd  # noqa: E402
import merged_f32_cases as mc  # noqa: E402


def main():
    group, out = sys.argv[1], sys.argv[2]
    lib = hymls_amd.load_library()
    dev = "cuda"
    rec = {"group": group, "ok": False, "message": "", "figures": None}
    try:
        if group.startswith("run:"):
            rec["figures"] = mc.check_run(lib, dev, mc.RUNS[mc.RUN_IDS.index(group[4:])])
        elif group == "defaults_lifecycle":
            mc.check_defaults(lib, dev)
            mc.check_lifecycle(lib, dev)
            mc.check_overflow(lib, dev)
        elif group == "python_xml":
            mc.check_python_and_xml(lib, dev, os.path.dirname(os.path.abspath(out)))
        elif group == "solver":
            rec["figures"] = mc.check_solver(lib, dev)
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
