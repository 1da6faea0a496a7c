"""Worker of the sharded FP32-basis test (launched through torch.distributed.run, one process per rank): every rank
solves K x = b with hymls_amd.NativeSolver and "MI Basis Storage" = "single" on its owned rows of a sharded
preconditioner (Stokes-C 16^3, Skew Cartesian, sx 4, one level, GMRES(100)); rank 0 solves the same system on one rank
and prints the iteration counts.
  python -m torch.distributed.run --nproc-per-node W tests/basis_f32_worker.py MODE
MODE = sim (the TEST-ONLY simulator library named by HYMLS_KRYLOV_SIM_LIB, gloo) | gpu (all ranks share cuda:0)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

import hymls_amd
from hymls_amd.dist import TorchComm, rank_grid


def main():
    mode = sys.argv[1]
    eq, n, sx, levels, part = "Stokes-C", 16, 4, 1, "Skew Cartesian"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if mode == "sim":
        lib, device = hymls_amd.load_library(os.environ["HYMLS_KRYLOV_SIM_LIB"]), "cpu"
    else:
        lib, device = hymls_amd.load_library(), "cuda:0"
    prm = {"Problem": {"Equations": eq, "Dimension": 3, "nx": n, "ny": n, "nz": n},
           "Preconditioner": {"Separator Length": sx, "Number of Levels": levels, "Partitioner": part}}
    sprm = {"Krylov Method": "GMRES", "MI Basis Storage": "single",
            "Iterative Solver": {"Convergence Tolerance": 1e-8, "Maximum Iterations": 300, "Num Blocks": 100}}
    a = float(n * n)
    P = hymls_amd.Preconditioner(None, prm, lib=lib, comm=TorchComm(device), rank_grid=rank_grid(world))
    req = P.RequiredRows()
    rows = hymls_amd.generate_rows(eq, n, n, n, req, a=a, lib=lib)
    P.SetMatrixRows(req, rows)
    P.SetTestVector(hymls_amd.generate_testvector_rows(req, *rows))
    P.Initialize()
    P.Compute()
    owned = P.OwnedRows()
    N = n ** 3 * 4
    x_ex = np.random.default_rng(9).uniform(-1, 1, N)
    rhs = torch.from_numpy(P.MatVec(x_ex[owned]).copy()).to(device)
    S = hymls_amd.NativeSolver(P, {"Solver": sprm})
    x_loc = S.ApplyInverse(rhs).cpu().numpy()
    parts = [None] * world
    dist.all_gather_object(parts, (owned, x_loc, S.getNumIter(), S.getBasisStorage()))
    if rank == 0:
        x = np.full(N, np.nan)
        for o, xl, _, _ in parts:
            x[o] = xl
        K = hymls_amd.generate_matrix(eq, n, n, n, a=a, lib=lib)
        P0 = hymls_amd.Preconditioner(K, prm, testVector=hymls_amd.generate_testvector(*K, lib=lib), lib=lib)
        P0.Compute()
        import scipy.sparse as sp
        Ks = sp.csr_matrix((K[2], K[1], K[0]), shape=(N, N))
        b = Ks @ x_ex
        S0 = hymls_amd.NativeSolver(P0, {"Solver": sprm})
        S0.ApplyInverse(torch.from_numpy(b).to(device))
        res = {"world": world, "its_sharded": [p[2] for p in parts], "storage": [p[3] for p in parts],
               "its_one_rank": S0.getNumIter(), "residual": float(np.linalg.norm(b - Ks @ x) / np.linalg.norm(b))}
        print("BASISF32_RESULT " + json.dumps(res), flush=True)
        del S0, P0
    del S, P
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
