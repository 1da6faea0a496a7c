"""Four right-hand sides through hymls_amd.NativeSolver at lock-step widths 1, 2 and 4 ("MI Lockstep Columns"), in
alternation in one process on one GPU, on ONE preconditioner and ONE solver object, for the FP64 and the FP32 basis.
Prints one JSON line per solve and writes all of them to --out.

  python tools/lockstep_bench.py [--n 128] [--levels 2] [--sx 8] [--restart 100] [--rounds 3] [--out FILE]

Stokes3D n^3, Skew Cartesian, b_v = K x_v with four seeded x_v, GMRES(restart), right preconditioned, tolerance 1e-8, zero
start.  The yardstick of a width is width 1 of the same build on the same handle in the same process.  A warm-up solve
(width 4, then width 1) comes first, so that no timed solve allocates the per-column buffers of its width for the first
time on a cold allocator; every change of the width or of the basis storage still reallocates inside the timed solve, for
every width alike.

Per solve: seconds, ms per iteration and column (seconds over the sum of the columns' iterations), the three phase times
of the solver (ApplyInverse, K x, orthogonalisation and updates; a batched call counts once), the per-column iterations
and the true relative residuals |b_v - K x_v| / |b_v|.
"""
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
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--levels", type=int, default=2, help="XML 'Number of Levels' (2 = the 3-level method)")
    ap.add_argument("--sx", type=int, default=8)
    ap.add_argument("--restart", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nvec", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_bench_128.json"))
    args = ap.parse_args()
    n, dev = args.n, torch.device("cuda", 0)
    lib = hymls_amd.load_library()
    t0 = time.time()
    rp, ci, va = hymls_amd.generate_problem("Stokes", n, n, n, lib=lib)
    tv = hymls_amd.generate_testvector(rp, ci, va, lib=lib)
    prm = {"Problem": {"Equations": "Stokes-C", "Dimension": 3, "nx": n, "ny": n, "nz": n},
           "Preconditioner": {"Separator Length": args.sx, "Number of Levels": args.levels, "Partitioner": "Skew Cartesian"}}
    P = hymls_amd.Preconditioner((rp, ci, va), prm, testVector=tv, lib=lib)
    P.Initialize()
    P.Compute()
    N = rp.size - 1
    del rp, ci, va, tv
    t_setup = time.time() - t0
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    B = torch.empty((args.nvec, N), dtype=torch.float64, device=dev)
    for v in range(args.nvec):
        x_ex = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
        P.MatVec(x_ex, B[v])
    del x_ex
    bb = [float(torch.dot(B[v], B[v])) for v in range(args.nvec)]

    def sprm(storage, width):
        return {"Solver": {"Krylov Method": "GMRES", "MI Basis Storage": storage, "MI Lockstep Columns": width, "Iterative Solver": {
            "Convergence Tolerance": 1e-8, "Maximum Iterations": 2000, "Num Blocks": args.restart, "Maximum Restarts": 40}}}

    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)

    emit({"problem": "Stokes3D %d^3 (%d DoF), Number of Levels %d, Skew Cartesian sx %d, GMRES(%d), tol 1e-8, %d right-hand sides"
                     % (n, N, args.levels, args.sx, args.restart, args.nvec), "setup_s": t_setup})
    S = hymls_amd.NativeSolver(P, sprm("double", 4))
    X = torch.empty_like(B)
    S.ApplyInverse(B, X)                                 # warm-up
    S.setParameterList(sprm("double", 1))
    S.ApplyInverse(B, X)
    for rnd in range(args.rounds):
        for storage in ("double", "single"):
            for width in (1, 2, 4):
                S.setParameterList(sprm(storage, width))
                S.set_profiling(True)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                S.ApplyInverse(B, X)
                torch.cuda.synchronize(); t = time.perf_counter() - t0
                ph = [S.seconds(i) for i in range(4)]
                S.set_profiling(False)
                cols = S.getColumnResults()
                its = sum(c["iterations"] for c in cols)
                res = []
                for v in range(args.nvec):
                    r = B[v] - P.MatVec(X[v].contiguous())
                    res.append(float(torch.dot(r, r) / bb[v]) ** 0.5)
                emit({"round": rnd, "basis_storage": storage, "lockstep_columns": width, "seconds": t,
                      "iterations": [c["iterations"] for c in cols], "restarts": [c["restarts"] for c in cols],
                      "ms_per_iteration_and_column": 1e3 * t / its,
                      "phase_seconds": {"solve": ph[0], "apply_inverse": ph[1], "matvec": ph[2], "orthogonalisation_and_updates": ph[3]},
                      "phase_ms_per_iteration_and_column": {"apply_inverse": 1e3 * ph[1] / its, "matvec": 1e3 * ph[2] / its,
                                                            "orthogonalisation_and_updates": 1e3 * ph[3] / its},
                      "achieved_tol": [c["achieved_tol"] for c in cols], "true_relative_residual": res,
                      "device_free_bytes_after_solve": torch.cuda.mem_get_info(dev)[0]})
    S.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
