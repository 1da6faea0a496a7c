"""The shifted operator product y = a K x + b B x (hymls_mi_shifted_product, the kernel k_kry_shifted) next to K x alone
(hymls_mi_matvec), in alternation in one process on one GPU and ONE preconditioner handle.  Prints one JSON line per
measurement and writes all of them to --out.

  python tools/shifted_bench.py [--n 128] [--levels 2] [--sx 8] [--reps 50] [--rounds 5] [--out FILE]

Stokes3D n^3, B = diag(1, 1, 1, 0) per node (the mass matrix of the velocities), x seeded random, (a, b) = (1, 0.5).  Three
variants, in this order in every round:
    matvec          hymls_mi_matvec on the handle: K x alone, the yardstick
    shift_identity  the shifted product with B = NULL (the identity): a K x + b x
    shift_diagonal  the shifted product with the diagonal B
The shifted product reads a device copy of the generated K (the arrays the handle was given); the bench first checks that
(1, 0) through it agrees with hymls_mi_matvec.  No speed target is set: the figure next to each time is the time of K x on
the same handle in the same run.

Method: a warm-up call per variant, then per round and variant `reps` calls, each ending in a device synchronise (the
building block synchronises itself, so K x is given the same), inside one host clock window; ms is the window over reps.
GB/s is over the algorithmic bytes: the CSR arrays of every matrix read once (12 nnz + 4 (n + 1)), x read once and y written
once (16 n).  two_pass_bytes is what dev::spmv twice would move for the same result: a second gather of x and y written, read
back and written again, 24 n more.  The last record holds the medians over the rounds, their ratios to K x and the spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import hymls_amd
from hymls_amd.native_solver import shifted_product


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--levels", type=int, default=2, help="XML 'Number of Levels' (2 = the 3-level method)")
    ap.add_argument("--sx", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shifted_bench_128.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shifted_bench needs a GPU: it measures, and does not fall back")
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
    N, nnz = rp.size - 1, int(rp[-1])
    t_setup = time.time() - t0
    Kd = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64)))
    del rp, ci, va, tv
    diag = (torch.arange(N, device=dev) % 4 != 3).to(torch.float64)
    Bd = (torch.arange(N + 1, dtype=torch.int32, device=dev), torch.arange(N, dtype=torch.int32, device=dev), diag)
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    x = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
    y = torch.empty_like(x)
    a, b = 1.0, 0.5

    # the same numbers first: (1, 0) through the building block against the handle's K x, then both shifted forms against it
    y0 = P.MatVec(x).clone()
    shifted_product(P, N, 1.0, Kd, 0.0, None, x, N, y, N, 1)
    agree = float((y - y0).abs().max() / y0.abs().max())
    shifted_product(P, N, a, Kd, b, None, x, N, y, N, 1)
    err_i = float((y - (a * y0 + b * x)).abs().max() / y0.abs().max())
    shifted_product(P, N, a, Kd, b, Bd, x, N, y, N, 1)
    err_d = float((y - (a * y0 + b * diag * x)).abs().max() / y0.abs().max())

    csr = lambda entries: 12 * entries + 4 * (N + 1)
    variants = {
        "matvec": (lambda: (P.MatVec(x, y), torch.cuda.synchronize()), csr(nnz) + 16 * N, None),
        "shift_identity": (lambda: shifted_product(P, N, a, Kd, b, None, x, N, y, N, 1), csr(nnz) + 16 * N, csr(nnz) + 16 * N + 24 * N),
        "shift_diagonal": (lambda: shifted_product(P, N, a, Kd, b, Bd, x, N, y, N, 1), csr(nnz) + csr(N) + 16 * N,
                           csr(nnz) + csr(N) + 16 * N + 24 * N),
    }
    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)

    emit({"problem": "Stokes3D %d^3 (%d DoF, %d entries of K), B = diag(1, 1, 1, 0) per node, (a, b) = (%g, %g), %d calls per "
                     "window, each ending in a device synchronise" % (n, N, nnz, a, b, args.reps), "setup_s": t_setup,
          "max_relative_difference": {"shifted_product_1_0_vs_matvec": agree, "shift_identity_vs_torch": err_i,
                                      "shift_diagonal_vs_torch": err_d}})
    for call, _, _ in variants.values():                           # warm-up
        call()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for rnd in range(args.rounds):
        for name, (call, nbytes, two_pass) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / args.reps
            ms[name].append(1e3 * t)
            emit({"round": rnd, "variant": name, "ms": 1e3 * t, "algorithmic_bytes": nbytes, "gb_per_s": nbytes / t / 1e9,
                  "two_pass_bytes": two_pass})
    med = {name: statistics.median(v) for name, v in ms.items()}
    emit({"summary": {"ms_median": med, "ms_over_matvec": {name: med[name] / med["matvec"] for name in med},
                      "gb_per_s_median": {name: variants[name][1] / (med[name] * 1e-3) / 1e9 for name in med},
                      "spread_over_rounds_ms": {name: max(v) - min(v) for name, v in ms.items()},
                      "yardstick": "matvec: K x alone on the same handle in the same run"}})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
