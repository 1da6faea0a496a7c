"""Worker of tests/test_native_bordered.py (launched through torch.distributed.run, one process per rank, like
tests/dist_worker.py): a sharded handle is refused by hymls_mi_solver_solve_bordered with -99, without and with a border,
and the plain sharded solve still works.  The library is the TEST-ONLY simulator named by HYMLS_KRYLOV_SIM_LIB (gloo)."""
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
from hymls_amd.native_solver import bind_bordered


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    lib = hymls_amd.load_library(os.environ["HYMLS_KRYLOV_SIM_LIB"])
    eq, n = "Laplace", 8
    prm = {"Problem": {"Equations": eq, "Dimension": 3, "nx": n, "ny": n, "nz": n},
           "Preconditioner": {"Separator Length": 4, "Number of Levels": 1, "Partitioner": "Cartesian"}}
    P = hymls_amd.Preconditioner(None, prm, lib=lib, comm=TorchComm("cpu"), rank_grid=rank_grid(world))
    req = P.RequiredRows()
    rows = hymls_amd.generate_rows(eq, n, n, n, req, a=float(n * n), lib=lib)
    P.SetMatrixRows(req, rows)
    P.SetTestVector(hymls_amd.generate_testvector_rows(req, *rows))
    P.Initialize()
    P.Compute()
    owned = P.OwnedRows()
    S = hymls_amd.NativeSolver(P, {"Krylov Method": "CG"})
    bind_bordered(lib)
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n ** 3)[owned].copy())
    x = torch.empty_like(b)
    sb = np.zeros(2)
    code = lib.hymls_mi_solver_solve_bordered(S._s, b.data_ptr(), None, x.data_ptr(), None, 1)
    rng = np.random.default_rng(17)
    Vg = rng.uniform(-1, 1, (n ** 3, 2))
    P.SetBorder(Vg[owned], None, np.eye(2))
    P.Compute()
    code_b = lib.hymls_mi_solver_solve_bordered(S._s, b.data_ptr(), None, x.data_ptr(), sb.ctypes.data, 1)
    P.SetBorder(None)
    P.Compute()
    S.ApplyInverse(b)                    # the plain sharded solve is untouched
    plain_ok = S.getNumIter() > 0
    parts = [None] * world
    dist.all_gather_object(parts, (code, code_b, plain_ok))
    if rank == 0:
        print("NBORDER_RESULT " + json.dumps({"codes": [p[0] for p in parts], "codes_bordered": [p[1] for p in parts],
                                              "plain_ok": all(p[2] for p in parts)}), flush=True)
    del S, P
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
