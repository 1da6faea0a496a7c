"""Worker of the sharded case of tests/test_fused_io.py and tests/test_fused_io_gpu.py (torch.distributed.run, one process
per rank): every rank builds the sharded preconditioner twice, with the vector passes fused into the interior solve and
with HYMLS_MI_NO_FUSED_IO=1, applies both to its part of a seeded vector and counts the entries that differ.  Rank 0
also compares the assembled result with the one-rank preconditioner.
  python -m torch.distributed.run --nproc-per-node W tests/fused_io_worker.py EQ N SX LEVELS CX PART MODE [LIBRARY]
MODE = hostsim (TEST-ONLY CPU simulator; LIBRARY: another simulator build) | gpu (all ranks share cuda:0, gloo staging)."""
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
    eq, n, sx, levels, cx, part, mode = sys.argv[1:8]
    n, sx, levels, cx = int(n), int(sx), int(levels), int(cx)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if mode == "hostsim":
        lib = hymls_amd.load_library(sys.argv[8] if len(sys.argv) > 8 else os.path.join(ROOT, "tests", "hostsim", "libhymls_mi_hostsim.so"))
        device = "cpu"
    else:
        lib = hymls_amd.load_library()
        device = "cuda:0"
    prec = {"Separator Length": sx, "Number of Levels": levels, "Partitioner": part}
    if cx > 0:
        prec["Coarsening Factor"] = cx
    prm = {"Problem": {"Equations": eq, "Dimension": 3, "nx": n, "ny": n, "nz": n}, "Preconditioner": prec}
    a = float(n * n)
    N = n * n * n * (1 if eq == "Laplace" else 4)
    b = np.random.default_rng(5).uniform(-1, 1, N)

    def sharded(fused_io):
        assert "HYMLS_MI_NO_FUSED_IO" not in os.environ
        if not fused_io:
            os.environ["HYMLS_MI_NO_FUSED_IO"] = "1"
        try:
            P = hymls_amd.Preconditioner(None, prm, lib=lib, comm=TorchComm(device), rank_grid=rank_grid(world))
            req = P.RequiredRows()
            rows = hymls_amd.generate_rows(eq, n, n, n, req, a=a, lib=lib)
            P.SetMatrixRows(req, rows)
            P.SetTestVector(hymls_amd.generate_testvector_rows(req, *rows))
            P.Initialize()
            P.Compute()
        finally:
            os.environ.pop("HYMLS_MI_NO_FUSED_IO", None)
        return P

    Pon, Poff = sharded(True), sharded(False)
    owned = Pon.OwnedRows()
    assert np.array_equal(owned, Poff.OwnedRows())
    x_on, x_off = Pon.ApplyInverse(b[owned]), Poff.ApplyInverse(b[owned])
    x_on2 = Pon.ApplyInverse(b[owned])
    parts = [None] * world
    dist.all_gather_object(parts, (owned, x_on, int(np.count_nonzero(x_on != x_off)), int(np.count_nonzero(x_on != x_on2)),
                                   Poff.apply_bytes(0) - Pon.apply_bytes(0)))
    ok = True
    if rank == 0:
        x = np.full(N, np.nan)
        for o, xl, _, _, _ in parts:
            x[o] = xl
        K = hymls_amd.generate_matrix(eq, n, n, n, a=a, lib=lib)
        P0 = hymls_amd.Preconditioner(K, prm, testVector=hymls_amd.generate_testvector(*K, lib=lib), lib=lib)
        P0.Compute()
        x0 = P0.ApplyInverse(b)
        res = {"world": world, "differ": sum(p[2] for p in parts), "repeat_differ": sum(p[3] for p in parts),
               "bytes_saved": [p[4] for p in parts], "rel_err": float(np.linalg.norm(x - x0) / np.linalg.norm(x0))}
        print("FUSED_IO_RESULT " + json.dumps(res), flush=True)
        ok = res["differ"] == 0 and res["repeat_differ"] == 0 and all(s > 0 for s in res["bytes_saved"]) and res["rel_err"] < 1e-9
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
