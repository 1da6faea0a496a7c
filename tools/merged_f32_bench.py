"""ApplyInverse with FP64 and with FP32 storage of the merged level-solve panels ("MI Merged Factor Storage"), measured
in alternation on ONE handle per configuration in one process on one GPU.

  python tools/merged_f32_bench.py [--n 256] [--configs a,b] [--runs 3] [--warmup 10] [--steps 20]
                                   [--out profiles/merged_f32_bench_256.json]

Stokes3D n^3, Skew Cartesian.  Configurations:
  a   separator length 8, 3-level, "MI Factor Storage" = "single": the benchmark's setup with the fused panels in FP32;
      the merged route solves the classes of levels >= 1
  b   separator length 16, 3-level: the finest level does not fit the fused kernel, the whole interior solve of every
      level runs on the merged route
Per run: merged storage 64, Compute, warm-up and timed ApplyInverse calls on device vectors with the per-phase event
timers of the library (hymls_mi_last_apply_seconds); merged storage 32, Compute, the same.  The FP64 run executes the code
path the library had before the option existed.  Every run is reported.

Byte model of the level kernels per ApplyInverse: hymls_mi_apply_bytes(h, 10), every stored panel entry of the merged
classes once per sweep and solve, 8 B or 4 B.  In a the level kernels run inside phase 4 (coarse), in b they are phase 1
(the two interior solves) plus their share of phase 4; the model TB/s divides the bytes by the sum of the two phases in b
and by phase 4 in a, so it is a lower bound on what the kernels reach.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import hymls_amd

CONFIGS = {"a": {"sx": 8, "levels": 2, "fused": "single"}, "b": {"sx": 16, "levels": 2, "fused": "double"}}


def measure(name, n, args, lib, dev):
    cfg = CONFIGS[name]
    rp, ci, va = hymls_amd.generate_problem("Stokes", n, n, n, lib=lib)
    tv = hymls_amd.generate_testvector(rp, ci, va, lib=lib)
    prm = {"Problem": {"Equations": "Stokes-C", "Dimension": 3, "nx": n, "ny": n, "nz": n},
           "Preconditioner": {"Separator Length": cfg["sx"], "Number of Levels": cfg["levels"], "Partitioner": "Skew Cartesian",
                              "MI Factor Storage": cfg["fused"]}}
    P = hymls_amd.Preconditioner((rp, ci, va), prm, testVector=tv, lib=lib)
    N = rp.size - 1
    del rp, ci, va, tv
    t0 = time.time()
    P.Initialize()
    out = {"config": name, "problem": "Stokes3D %d^3 (%d DoF), Number of Levels %d, Skew Cartesian sx %d, fused storage %s"
           % (n, N, cfg["levels"], cfg["sx"], cfg["fused"]), "initialize_s": time.time() - t0, "runs": []}
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    v = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
    y = torch.empty_like(v)
    for run in range(args.runs):
        for storage in ("double", "single"):
            P.SetMergedFactorStorage(storage)
            torch.cuda.synchronize(); t = time.perf_counter()
            P.Compute()
            torch.cuda.synchronize()
            t_comp = time.perf_counter() - t
            for _ in range(args.warmup):
                P.ApplyInverse(v, y)
            torch.cuda.synchronize()
            P.set_profiling(True)
            for _ in range(args.steps):
                P.ApplyInverse(v, y)
            torch.cuda.synchronize()
            ph = [P.last_apply_seconds(i) for i in range(5)]
            P.set_profiling(False)
            level_bytes = P.apply_bytes(10)
            level_s = ph[4] + (ph[1] if name == "b" else 0.0)
            out["runs"].append({
                "run": run, "merged_storage": storage, "compute_s": t_comp, "apply_ms": 1e3 * ph[0],
                "phase_ms": {"interior_two_launches": 1e3 * ph[1], "spmv": 1e3 * ph[2], "schur": 1e3 * ph[3], "coarse": 1e3 * ph[4]},
                "level_kernel_model_bytes": level_bytes, "level_kernel_phase_ms": 1e3 * level_s,
                "level_kernel_model_tb_per_s": level_bytes / level_s / 1e12 if level_s > 0 else None,
                "apply_bytes_total": P.apply_bytes(0), "resident_panel_bytes": P.apply_bytes(9),
                "free_device_bytes": torch.cuda.mem_get_info()[0], "y_norm": float(torch.linalg.norm(y))})
            print("merged_f32_bench %s: run %d merged storage %s: %.3f ms per ApplyInverse, coarse %.3f ms, interior %.3f ms"
                  % (name, run, storage, 1e3 * ph[0], 1e3 * ph[4], 1e3 * ph[1]), file=sys.stderr, flush=True)
    out["levels"] = P.level_sizes()
    pairs = [(out["runs"][2 * r]["apply_ms"], out["runs"][2 * r + 1]["apply_ms"]) for r in range(args.runs)]
    out["fp32_not_slower_in_every_run"] = all(s <= d for d, s in pairs)
    del P, v, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--configs", default="a,b")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = hymls_amd.load_library()
    out = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps,
           "lvl_f32_cols": os.environ.get("HYMLS_MI_LVL_F32_COLS", "default"), "configs": []}
    for name in args.configs.split(","):
        out["configs"].append(measure(name, args.n, args, lib, dev))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
