"""Worker of tests/test_native_shifted.py (launched through torch.distributed.run, one process per rank, like
tests/dist_worker.py): on a sharded handle a solve with a shift other than (1, 0) is refused with -99 on every rank, and the
plain sharded solve works again after setShift(1, 0).  The library is the TEST-ONLY simulator named by HYMLS_KRYLOV_SIM_LIB
(gloo)."""
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
from hymls_amd.native_solver import bind_shifted


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
    bind_shifted(lib)
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n ** 3)[owned].copy())
    x = torch.empty_like(b)
    nloc = len(owned)
    code_set = lib.hymls_mi_solver_set_shift(S._s, 1.0, 0.5)
    code = lib.hymls_mi_solver_solve(S._s, b.data_ptr(), nloc, x.data_ptr(), nloc, 1, 1)
    S.setShift(1.0, 0.0)
    S.ApplyInverse(b)                    # the plain sharded solve is untouched
    plain_ok = S.getNumIter() > 0
    parts = [None] * world
    dist.all_gather_object(parts, (code_set, code, plain_ok))
    if rank == 0:
        print("NSHIFT_RESULT " + json.dumps({"set": [p[0] for p in parts], "codes": [p[1] for p in parts],
                                             "plain_ok": all(p[2] for p in parts)}), flush=True)
    del S, P
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
