"""A solve with projection vectors (NativeSolver.setProjectionVectors) in the folded and in the literal form of the projected
preconditioner ("MI Projection Form"), in alternation in one process on one GPU, on ONE preconditioner and ONE solver
object, for m = 1, 4 and 8 projection vectors.  Prints one JSON line per solve and writes all of them to --out.

  python tools/projected_bench.py [--n 128] [--levels 2] [--sx 8] [--restart 100] [--rounds 3] [--m 1,4,8] [--out FILE]

Stokes3D n^3, Skew Cartesian, V = m seeded random orthonormal columns (Gram-Schmidt on the device), BV = V, the right-hand side
b = (I - V V') K (I - V V') x_ex with a seeded x_ex, GMRES(restart), right preconditioned, tolerance 1e-8, zero start.
The yardstick of the folded form is the literal form -- the reference's arithmetic, two ApplyInverse per application -- of
the same build on the same handle in the same process; one warm-up solve per form comes first.

Per solve: seconds, iterations, the phase times of the solver per iteration (ApplyInverse with the preconditioner's
projector, K x with its two projectors, orthogonalisation and updates), the achieved tolerance and the projected true
residual |(I - V V')(b - K x)| / |b|.  The last record holds, per m, the median over the rounds of the ApplyInverse phase per
iteration of both forms, their ratio, and the spread (max - min) of each form over the rounds.
"""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--m", default="1,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projected_bench_128.json"))
    args = ap.parse_args()
    n, dev = args.n, torch.device("cuda", 0)
    ms = [int(v) for v in args.m.split(",")]
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
    Vall = torch.rand((max(ms), N), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    for j in range(max(ms)):                                  # Gram-Schmidt, twice: orthonormal to rounding
        for _ in range(2):
            if j:
                Vall[j] -= Vall[:j].t() @ (Vall[:j] @ Vall[j])
        Vall[j] /= torch.linalg.norm(Vall[j])

    def sprm(form):
        return {"Solver": {"Krylov Method": "GMRES", "MI Projection Form": form, "Iterative Solver": {
            "Convergence Tolerance": 1e-8, "Maximum Iterations": 2000, "Num Blocks": args.restart, "Maximum Restarts": 40}}}

    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)

    emit({"problem": "Stokes3D %d^3 (%d DoF), Number of Levels %d, Skew Cartesian sx %d, GMRES(%d), tol 1e-8, m in %s random "
                     "orthonormal projection vectors" % (n, N, args.levels, args.sx, args.restart, ms), "setup_s": t_setup})
    S = hymls_amd.NativeSolver(P, sprm("folded"))
    summary = {}
    for m in ms:
        V = Vall[:m].t()                                      # (N, m), its columns contiguous
        proj = lambda r: r - V @ (V.t() @ r)
        b = proj(P.MatVec(proj(x_ex).contiguous())).contiguous()
        bb = float(torch.dot(b, b))
        S.setProjectionVectors(V)
        x = torch.empty_like(b)
        for form in ("folded", "literal"):                  # warm-up; the first one forms Z and H
            S.setParameterList(sprm(form))
            S.ApplyInverse(b, x)
        per_it = {"folded": [], "literal": []}
        for rnd in range(args.rounds):
            for form in ("folded", "literal"):
                S.setParameterList(sprm(form))
                S.set_profiling(True)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                S.ApplyInverse(b, x)
                torch.cuda.synchronize(); t = time.perf_counter() - t0
                ph = [S.seconds(i) for i in range(4)]
                S.set_profiling(False)
                its = S.getNumIter()
                r = proj(b - P.MatVec(x))
                per_it[form].append(1e3 * ph[1] / its)
                emit({"m": m, "round": rnd, "form": form, "seconds": t, "iterations": its, "restarts": S.getNumRestarts(),
                      "ms_per_iteration": 1e3 * t / its,
                      "phase_seconds": {"solve": ph[0], "apply_inverse": ph[1], "matvec": ph[2], "orthogonalisation_and_updates": ph[3]},
                      "phase_ms_per_iteration": {"apply_inverse": 1e3 * ph[1] / its, "matvec": 1e3 * ph[2] / its,
                                                 "orthogonalisation_and_updates": 1e3 * ph[3] / its},
                      "achieved_tol": S.achievedTol(), "projected_true_relative_residual": float(torch.dot(r, r) / bb) ** 0.5})
        med = {f: statistics.median(v) for f, v in per_it.items()}
        summary[str(m)] = {"apply_inverse_ms_per_iteration_median": med,
                           "folded_over_literal": med["folded"] / med["literal"],
                           "spread_over_rounds_ms": {f: max(v) - min(v) for f, v in per_it.items()}}
    emit({"summary": summary})
    S.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
