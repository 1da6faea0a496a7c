"""GMRES solve of the bench configuration with hymls_amd.NativeSolver in double and in single basis storage
("MI Basis Storage"), in alternation in one process on one GPU, on ONE preconditioner and ONE solver object.
Prints one JSON line per solve.

  python tools/basis_f32_bench.py [--n 256] [--levels 2] [--sx 8] [--restart 100] [--rounds 2] [--out FILE]

The problem of tools/krylov_bench.py: Stokes3D n^3, Skew Cartesian, b = K x_ex with a seeded x_ex, GMRES(restart), right
preconditioned, tolerance 1e-8, at most 2000 iterations and 40 restarts, zero start.  The storage is switched with
setParameterList, so every solve after the first reallocates the basis (inside the timed solve, as the first does).

Algorithmic bytes of phase 3 (orthogonalisation and vector updates), N rows, an iteration with k basis columns:
  double:  3 k N 8 (the three passes read the basis) + 7 N 8 (w: read by pass A, read and written by pass B, read by
           pass C, the new column written by pass C, read and written by the normalisation)
  single:  3 k N 4 (the passes) + N 4 (column k read by the widening copy) + N 4 (the rounded store of column k + 1)
           + 7 N 8 (w: read by pass A, read and written by pass B, read and written by pass C, read by the rounding
           store; the FP64 copy of column k written into t)  =  (12 k + 64) N
  solution update of a cycle that used k columns:  double (k + 2) N 8,  single k N 4 + 2 N 8.
So the single figure is not the double figure halved: only basis entries are counted at 4 B.  TB/s divides these bytes
by the seconds of phase 3 of the solver (every vector update of the solve included): a lower bound of the passes' rate.
The cycle lengths are reconstructed from the iteration and restart counts for full cycles; a cycle that the FP32 scheme
ended early is counted with its real length only in the total of iterations (the model then assumes the early cycle
came last, which changes the figure by well under one percent).
basis_bytes = (restart + 1) * ld * bytes per entry, ld = N rounded up to 16: what the solver allocates.
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


def orth_bytes(its, m, n, single):
    """algorithmic bytes of phase 3 of `its` GMRES(m) iterations (see the module docstring)"""
    eb = 4.0 if single else 8.0
    total, k_used = 0.0, 0
    for i in range(its):
        k = i % m + 1
        total += 3 * k * n * eb + 7 * n * 8.0 + (2 * n * 4.0 if single else 0.0)
        k_used = k
        if k == m:
            total += m * n * eb + 2 * n * 8.0
    if its % m:
        total += k_used * n * eb + 2 * n * 8.0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--sx", type=int, default=8)
    ap.add_argument("--restart", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append every JSON line to this file")
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
    x_ex = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
    b = P.MatVec(x_ex).clone()
    del x_ex
    bb = float(torch.dot(b, b))

    def sprm(storage):
        return {"Solver": {"Krylov Method": "GMRES", "MI Basis Storage": storage, "Iterative Solver": {
            "Convergence Tolerance": 1e-8, "Maximum Iterations": 2000, "Num Blocks": args.restart, "Maximum Restarts": 40}}}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    emit({"problem": "Stokes3D %d^3 (%d DoF), Number of Levels %d, Skew Cartesian sx %d, GMRES(%d), tol 1e-8"
                     % (n, N, args.levels, args.sx, args.restart), "setup_s": t_setup})
    S = hymls_amd.NativeSolver(P, sprm("double"))
    ld = (N + 15) // 16 * 16
    for rnd in range(args.rounds):
        for storage in ("double", "single"):
            S.setParameterList(sprm(storage))
            S.set_profiling(True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            x = S.ApplyInverse(b)
            torch.cuda.synchronize(); t = time.perf_counter() - t0
            its = S.getNumIter()
            ph = [S.seconds(i) for i in range(4)]
            S.set_profiling(False)
            r = b - P.MatVec(x)
            res = float(torch.dot(r, r) / bb) ** 0.5
            del x, r
            single = storage == "single"
            ob = orth_bytes(its, args.restart, N, single)
            emit({"round": rnd, "basis_storage": storage, "iterations": its, "restarts": S.getNumRestarts(), "seconds": t,
                  "ms_per_iteration": 1e3 * t / its, "achieved_tol": S.achievedTol(), "true_relative_residual": res,
                  "phase_seconds": {"solve": ph[0], "apply_inverse": ph[1], "matvec": ph[2], "orthogonalisation_and_updates": ph[3]},
                  "orth_ms_per_iteration": 1e3 * ph[3] / its, "orth_algorithmic_bytes": ob,
                  "orth_tb_per_s": ob / ph[3] / 1e12 if ph[3] > 0 else None,
                  "basis_bytes": (args.restart + 1) * ld * (4 if single else 8),
                  "device_free_bytes_after_solve": torch.cuda.mem_get_info(dev)[0]})
    S.close()


if __name__ == "__main__":
    main()
