"""Checks of the vector passes fused into the interior solve of a single-vector ApplyInverse ("Vector passes inside the interior solve"): the
entry gather of b1, y1 = A12 x2, x1 -= A11 \\ y1 and the exit scatter of x1 ride inside the two launches of the fused
kernel when every interior row of a level is solved by it.  HYMLS_MI_NO_FUSED_IO=1 (read by Initialize) keeps the
separate kernels.  Both sequences do the same operations in the same order, so the results are compared with
np.array_equal; nothing here has a tolerance except the comparison with the oracle.

Shared by tests/test_fused_io.py (TEST-ONLY host simulators, CPU) and tests/test_fused_io_gpu.py (the HIP library)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

import hymls_amd
from common import problem, xml_params

# eq, n, sx, "Number of Levels", cx, partitioner
STOKES16 = ("Stokes-C", 16, 8, 1, -1, "Skew Cartesian")
STOKES32 = ("Stokes-C", 32, 4, 2, 2, "Skew Cartesian")     # two levels with a fused interior solve
LAPLACE16 = ("Laplace", 16, 4, 1, -1, "Cartesian")
CASES = [STOKES16, STOKES32, LAPLACE16]
CASE_IDS = ["stokes16_sx8_levels1", "stokes32_sx4_levels2", "laplace16_sx4_levels1"]
SWITCH = "HYMLS_MI_NO_FUSED_IO"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(case, lib, fused_io, env=None, storage=None):
    """a computed handle; the development switches are read by Initialize / Compute, so they are set around them only"""
    eq, n, sx, levels, cx, part = case
    A, tv = problem(eq, n)
    extra = dict(env or {})
    if not fused_io:
        extra[SWITCH] = "1"
    assert not any(k in os.environ for k in list(extra) + [SWITCH])
    os.environ.update(extra)
    try:
        P = hymls_amd.Preconditioner(A, xml_params(eq, n, sx, levels, cx=cx, partitioner=part), testVector=tv, lib=lib)
        if storage is not None:
            P.SetFactorStorage(storage)
        assert P.Initialize() == 0 and P.Compute() == 0
    finally:
        for k in extra:
            os.environ.pop(k, None)
    return A, P


def apply(P, b, dev, inplace=False):
    """ApplyInverse through device pointers (host pointers on the simulators); inplace: the same array as b and x"""
    t = torch.from_numpy(np.ascontiguousarray(b.T if b.ndim == 2 else b).copy()).to(dev)
    x = P.ApplyInverse(t, t) if inplace else P.ApplyInverse(t)
    x = x.cpu().numpy()
    return x.T if b.ndim == 2 else x


def interior_rows(P):
    """sum of n1 over the levels that have a Schur complement (level_sizes: level, rows, separator rows, ...)"""
    return sum(s[1] - s[2] for s in P.level_sizes() if s[2] > 0)


def check_equal(lib, dev, case, env=None, storage=None, expect_fused=True):
    """fusion on against HYMLS_MI_NO_FUSED_IO=1 on the same problem: equal bits; and the byte model tells which sequence
    a handle takes -- the vector bytes of apply_bytes(0) count 7 n1-sized passes of 8 B per level less with the fusion"""
    A, Pon = make(case, lib, True, env, storage)
    _, Poff = make(case, lib, False, env, storage)
    saved = Poff.apply_bytes(0) - Pon.apply_bytes(0)
    n1 = interior_rows(Pon)
    print("fused io %s: vector bytes saved per apply %.0f, 56 B x interior rows of all levels %d" % (case, saved, 56 * n1), flush=True)
    assert n1 > 0 and saved == (56.0 * n1 if expect_fused else 0.0), (saved, n1)
    rng = np.random.default_rng(11)
    for rep in range(2):
        b = rng.uniform(-1, 1, A.shape[0])
        x_on, x_off = apply(Pon, b, dev), apply(Poff, b, dev)
        nbad = int(np.count_nonzero(x_on != x_off))
        print("  vector %d: entries that differ between the two sequences: %d of %d" % (rep, nbad, b.size), flush=True)
        assert np.isfinite(x_on).all() and np.abs(x_on).max() > 0
        assert nbad == 0 and np.array_equal(x_on, x_off)
        assert np.array_equal(apply(Pon, b, dev), x_on)                       # buffers reused: same bits again
    assert np.array_equal(apply(Pon, b, dev, inplace=True), x_on)            # b and x are the same array
    assert np.array_equal(apply(Poff, b, dev, inplace=True), x_on)
    assert np.array_equal(Pon.ApplyInverse(b), x_on)                          # vectors in host memory
    # several right-hand sides keep the separate kernels on both handles
    B = rng.uniform(-1, 1, (A.shape[0], 2))
    assert np.array_equal(apply(Pon, B, dev), apply(Poff, B, dev))
    return A, Pon, Poff


def run_worker(world, case, mode, port, library=None, timeout=900):
    """tests/fused_io_worker.py on world ranks; returns what rank 0 reports"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "fused_io_worker.py")] + [str(a) for a in case] + [mode]
    if library:
        cmd.append(library)
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("FUSED_IO_RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(lines[-1][len("FUSED_IO_RESULT "):])
    print(res)
    return res
