"""GMRES solve of the bench configuration with hymls_amd.Solver (torch loop) and with hymls_amd.NativeSolver (the
library's solver, include/hymls_mi_solver.h), one after the other in one process on one GPU.  Prints one JSON line.

  python tools/krylov_bench.py [--n 256] [--levels 2] [--sx 8] [--restart 100] [--native-only]

Stokes3D n^3, Skew Cartesian, b = K x_ex with a seeded x_ex, GMRES(restart), right preconditioned, tolerance 1e-8,
at most 2000 iterations and 40 restarts, zero start.  Orthogonalisation bytes are algorithmic: per iteration with k
basis columns the three passes read the basis 3 k n 8 B, plus 7 n 8 B of w traffic and the normalisation; the solution
update of every cycle adds (k + 2) n 8 B.  The native TB/s divides them by the time of phase 3 of the solver
(orthogonalisation and every vector update of the solve), so it is a lower bound of the orthogonalisation's own rate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import hymls_amd


def orth_bytes(its, m, n):
    """algorithmic bytes of the orthogonalisation and the solution updates of `its` GMRES(m) iterations"""
    total, k_used = 0.0, 0
    for i in range(its):
        k = i % m + 1
        total += (3 * k + 7) * n * 8.0
        k_used = k
        if k == m:
            total += (m + 2) * n * 8.0
    if its % m:
        total += (k_used + 2) * n * 8.0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--sx", type=int, default=8)
    ap.add_argument("--restart", type=int, default=100)
    ap.add_argument("--native-only", action="store_true")
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
    sprm = {"Solver": {"Krylov Method": "GMRES", "Iterative Solver": {
        "Convergence Tolerance": 1e-8, "Maximum Iterations": 2000, "Num Blocks": args.restart, "Maximum Restarts": 40}}}
    bb = float(torch.dot(b, b))

    def true_res(x):
        r = b - P.MatVec(x)
        return float(torch.dot(r, r) / bb) ** 0.5

    out = {"problem": "Stokes3D %d^3 (%d DoF), Number of Levels %d, Skew Cartesian sx %d, GMRES(%d), tol 1e-8"
                      % (n, N, args.levels, args.sx, args.restart), "setup_s": t_setup}
    if not args.native_only:
        S = hymls_amd.Solver(P, P, sprm)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x = S.ApplyInverse(b)
        torch.cuda.synchronize(); t = time.perf_counter() - t0
        its = S.getNumIter()
        out["torch"] = {"iterations": its, "seconds": t, "ms_per_iteration": 1e3 * t / its, "true_relative_residual": true_res(x),
                        "orth_algorithmic_bytes_four_passes": orth_bytes(its, args.restart, N) * 4 / 3}
        del S, x
        torch.cuda.empty_cache()
    S = hymls_amd.NativeSolver(P, sprm)
    S.set_profiling(True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    x = S.ApplyInverse(b)
    torch.cuda.synchronize(); t = time.perf_counter() - t0
    its = S.getNumIter()
    ph = [S.seconds(i) for i in range(4)]
    ob = orth_bytes(its, args.restart, N)
    out["native"] = {"iterations": its, "seconds": t, "ms_per_iteration": 1e3 * t / its, "true_relative_residual": true_res(x),
                     "phase_seconds": {"solve": ph[0], "apply_inverse": ph[1], "matvec": ph[2], "orthogonalisation_and_updates": ph[3]},
                     "orth_algorithmic_bytes": ob, "orth_tb_per_s": ob / ph[3] / 1e12 if ph[3] > 0 else None,
                     "orth_ms_per_iteration": 1e3 * ph[3] / its}
    S.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
