"""ApplyInverse with FP64 and with FP32 storage of the interior factor panels ("MI Factor Storage"), measured in
alternation on ONE handle in one process on one GPU (two 256^3 handles and a Krylov basis do not fit into 288 GB).

  python tools/f32_apply_bench.py [--n 256] [--levels 2] [--sx 8] [--alternations 3] [--warmup 10] [--steps 20]
                                  [--no-solve] [--out profiles/<name>.json]

Stokes3D n^3, Skew Cartesian.  Per alternation: storage 64, Compute, warm-up and timed ApplyInverse calls on device
vectors with the per-phase event timers of the library (hymls_mi_last_apply_seconds); storage 32, Compute, the same.
Every run is reported.  Then right-preconditioned GMRES(100) to 1e-8 through the native solver in each storage
(b = K x_ex, zero start), with the true FP64 residual ||b - K x|| / ||b||.

Byte model of one k_interior_fused launch (an ApplyInverse has two): every stored panel entry once, 8 B or 4 B, plus
16 B per interior unknown (the vector in and out).  hymls_mi_apply_bytes(h, 1) counts the panel bytes of both launches.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--sx", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--restart", type=int, default=100)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dev = args.n, torch.device("cuda", 0)
    lib = hymls_amd.load_library()
    rp, ci, va = hymls_amd.generate_problem("Stokes", n, n, n, lib=lib)
    tv = hymls_amd.generate_testvector(rp, ci, va, lib=lib)
    prm = {"Problem": {"Equations": "Stokes-C", "Dimension": 3, "nx": n, "ny": n, "nz": n},
           "Preconditioner": {"Separator Length": args.sx, "Number of Levels": args.levels, "Partitioner": "Skew Cartesian"}}
    P = hymls_amd.Preconditioner((rp, ci, va), prm, testVector=tv, lib=lib)
    N = rp.size - 1
    del rp, ci, va, tv
    t0 = time.time()
    P.Initialize()
    out = {"problem": "Stokes3D %d^3 (%d DoF), Number of Levels %d, Skew Cartesian sx %d" % (n, N, args.levels, args.sx),
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps,
           "initialize_s": time.time() - t0, "runs": []}
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    x_ex = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
    v = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
    y = torch.empty_like(v)
    lv = P.level_sizes()
    n1 = lv[0][1] - lv[0][2]                    # interior unknowns of the finest level
    out["levels"] = lv

    def compute(storage):
        P.SetFactorStorage(storage)
        torch.cuda.synchronize(); t = time.perf_counter()
        P.Compute()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for alt in range(args.alternations):
        for storage in ("double", "single"):
            t_comp = compute(storage)
            for _ in range(args.warmup):
                P.ApplyInverse(v, y)
            torch.cuda.synchronize()
            P.set_profiling(True)
            t = time.perf_counter()
            for _ in range(args.steps):
                P.ApplyInverse(v, y)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t) / args.steps
            ph = [P.last_apply_seconds(i) for i in range(5)]
            P.set_profiling(False)
            launch_bytes = P.apply_bytes(1) / 2 + 16.0 * n1
            launch_s = ph[1] / 2
            out["runs"].append({
                "alternation": alt, "storage": storage, "compute_s": t_comp,
                "apply_ms_wall": 1e3 * wall, "apply_ms_events": 1e3 * ph[0],
                "phase_ms": {"interior_two_launches": 1e3 * ph[1], "spmv": 1e3 * ph[2], "schur": 1e3 * ph[3], "coarse": 1e3 * ph[4]},
                "fused_launch_ms": 1e3 * launch_s, "fused_launch_model_bytes": launch_bytes,
                "fused_launch_tb_per_s": launch_bytes / launch_s / 1e12 if launch_s > 0 else None,
                "apply_bytes_total": P.apply_bytes(0), "apply_bytes_panels": P.apply_bytes(1),
                "resident_panel_bytes": P.apply_bytes(9), "free_device_bytes": torch.cuda.mem_get_info()[0]})
            print("f32_apply_bench: alternation %d %s: %.3f ms per ApplyInverse, %.3f ms per fused launch" %
                  (alt, storage, 1e3 * ph[0], 1e3 * launch_s), file=sys.stderr, flush=True)
    out["levels"] = P.level_sizes()
    if not args.no_solve:
        b = P.MatVec(x_ex).clone()
        del x_ex
        bb = float(torch.dot(b, b))
        sprm = {"Solver": {"Krylov Method": "GMRES", "Iterative Solver": {
            "Convergence Tolerance": 1e-8, "Maximum Iterations": 2000, "Num Blocks": args.restart, "Maximum Restarts": 40}}}
        out["gmres"] = {}
        for storage in ("double", "single"):
            compute(storage)
            S = hymls_amd.NativeSolver(P, sprm)
            torch.cuda.synchronize(); t = time.perf_counter()
            x = S.ApplyInverse(b)
            torch.cuda.synchronize(); t = time.perf_counter() - t
            r = b - P.MatVec(x)
            out["gmres"][storage] = {"iterations": S.getNumIter(), "seconds": t,
                                     "true_relative_residual": float(torch.dot(r, r) / bb) ** 0.5}
            S.close()
            del x, r, S
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
