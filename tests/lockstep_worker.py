"""Worker of tests/test_lockstep.py (launched through torch.distributed.run, one process per rank, like
tests/native_bordered_worker.py): on a sharded handle a solve with lock-step columns and the three building blocks
(hymls_mi_matvec_mv, hymls_mi_orthogonalize_mv, hymls_mi_orthogonalize_mv_f32) return -99, and the plain width-1 solve
still works.  The library is the TEST-ONLY simulator named by HYMLS_KRYLOV_SIM_LIB (gloo)."""
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
from hymls_amd.native_solver import bind_lockstep


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    lib = bind_lockstep(hymls_amd.load_library(os.environ["HYMLS_KRYLOV_SIM_LIB"]))
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
    no = len(owned)
    S = hymls_amd.NativeSolver(P, {"Krylov Method": "CG", "MI Lockstep Columns": 2})
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, n ** 3))[:, owned].copy())
    x = torch.empty_like(b)
    solve = lib.hymls_mi_solver_solve(S._s, b.data_ptr(), no, x.data_ptr(), no, 2, 1)
    k = np.array([1, 1], dtype=np.int32)
    h, nrm = np.zeros(2), np.zeros(2)
    blocks = [lib.hymls_mi_matvec_mv(P._h, b.data_ptr(), no, x.data_ptr(), no, 2, 1),
              lib.hymls_mi_orthogonalize_mv(P._h, no, 2, k.ctypes.data, b.data_ptr(), no, no, x.data_ptr(), no, h.ctypes.data, 1,
                                            nrm.ctypes.data),
              lib.hymls_mi_orthogonalize_mv_f32(P._h, no, 2, k.ctypes.data, b.float().data_ptr(), no, no, x.data_ptr(), no, None, 0,
                                                h.ctypes.data, 1, nrm.ctypes.data)]
    S.setParameterList({"Krylov Method": "CG", "MI Lockstep Columns": 1})
    S.ApplyInverse(b[0].contiguous())       # the plain sharded solve is untouched
    plain_ok = S.getNumIter() > 0
    parts = [None] * world
    dist.all_gather_object(parts, (solve, blocks, plain_ok))
    if rank == 0:
        print("LOCKSTEP_RESULT " + json.dumps({"solve": [p[0] for p in parts], "blocks": [p[1] for p in parts],
                                               "plain_ok": all(p[2] for p in parts)}), flush=True)
    del S, P
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
