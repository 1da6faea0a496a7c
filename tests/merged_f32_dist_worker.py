"""Worker of tests/test_merged_f32.py::test_sharded_sim (torch.distributed.run, gloo, one process per rank): the sharded
preconditioner with FP32 storage of the merged level-solve panels on every rank against one rank with the same storage,
Stokes-C 16^3, every class on the merged route (the test sets HYMLS_MI_NO_FUSED_SOLVE=1).
  python -m torch.distributed.run --nproc-per-node 2 tests/merged_f32_dist_worker.py LIBRARY"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch.distributed as dist

import hymls_amd
from hymls_amd.dist import TorchComm, rank_grid


def main():
    lib = hymls_amd.load_library(sys.argv[1])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eq, n, sx = "Stokes-C", 16, 4
    prm = {"Problem": {"Equations": eq, "Dimension": 3, "nx": n, "ny": n, "nz": n},
           "Preconditioner": {"Separator Length": sx, "Number of Levels": 1, "Partitioner": "Skew Cartesian",
                              "MI Merged Factor Storage": "single"}}
    P = hymls_amd.Preconditioner(None, prm, lib=lib, comm=TorchComm("cpu"), rank_grid=rank_grid(world))
    req = P.RequiredRows()
    rows = hymls_amd.generate_rows(eq, n, n, n, req, a=float(n * n), lib=lib)
    P.SetMatrixRows(req, rows)
    P.SetTestVector(hymls_amd.generate_testvector_rows(req, *rows))
    P.Compute()
    owned = P.OwnedRows()
    N = n * n * n * 4
    b = np.random.default_rng(5).uniform(-1, 1, N)
    parts = [None] * world
    dist.all_gather_object(parts, (owned, P.ApplyInverse(b[owned]), P.MergedFactorStorage()))
    if rank == 0:
        x = np.full(N, np.nan)
        cover = np.zeros(N, np.int64)
        for o, xl, _ in parts:
            x[o] = xl
            cover[o] += 1
        K = hymls_amd.generate_matrix(eq, n, n, n, a=float(n * n), lib=lib)
        tv = hymls_amd.generate_testvector(*K, lib=lib)
        P32 = hymls_amd.Preconditioner(K, prm, testVector=tv, lib=lib)
        P32.Compute()
        x32 = P32.ApplyInverse(b)
        prm64 = {"Problem": prm["Problem"], "Preconditioner": dict(prm["Preconditioner"], **{"MI Merged Factor Storage": "double"})}
        P64 = hymls_amd.Preconditioner(K, prm64, testVector=tv, lib=lib)
        P64.Compute()
        x64 = P64.ApplyInverse(b)
        res = {"cover_ok": bool((cover == 1).all()), "storage": [p[2] for p in parts],
               "rel_err": float(np.linalg.norm(x - x32) / np.linalg.norm(x32)),
               "rel_to_double": float(np.linalg.norm(x - x64) / np.linalg.norm(x64)),
               "bytes10_64": P64.apply_bytes(10), "bytes10_ratio": P32.apply_bytes(10) / max(P64.apply_bytes(10), 1.0)}
        print("MERGED_F32_DIST_RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
