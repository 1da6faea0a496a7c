"""The bitwise comparison of tests/test_solve_tails_gpu.py is sharp for the mistakes a batched leftover loop invites --
shown on a numpy restatement of one k loop of the fused solve (four accumulators over an unrolled-by-four main part, the
leftover entries into the first one, (a0 + a1) + (a2 + a3) at the end): another accumulator, another order, or a zero
multiplied in for an absent entry all change the bits that np.array_equal / same_bits compares.  Also: the fixtures exist
for every case, within the size limit, and the case list reaches every changed loop on the host simulator."""
import os

import numpy as np
import pytest

import solve_tails_cases as st

fc, fl = st.fc, st.fl


def row_sum(l, f, tail="a0", beyond=None):
    """sum_k l[k] f[k] as the wide path adds it.  tail: 'a0' the kernel's order; 'a_u' leftover entry u into accumulator u;
    'reversed' leftover entries last to first; 'zero_fill': a batch of three in which an absent entry is not skipped but
    read (beyond = what lies behind the row's entries) and multiplied by 0."""
    a = np.zeros(4)
    n, k = len(l), 0
    while k + 3 < n:
        for u in range(4):
            a[u] += l[k + u] * f[k + u]
        k += 4
    left = list(range(k, n))
    if tail == "reversed":
        left = left[::-1]
    for u, kk in enumerate(left):
        a[(kk - k) if tail == "a_u" else 0] += l[kk] * f[kk]
    if tail == "zero_fill":
        for u in range(len(left), 3):
            a[0] += beyond[u - len(left)] * 0.0
    return (a[0] + a[1]) + (a[2] + a[3])


def solve_rows(L, f, **kw):
    """x_r = f_r + sum_{k < r} L[r, k] f[k]: the forward step of one front."""
    return np.array([f[r] + row_sum(L[r, :r], f[:r], **kw) for r in range(len(f))])


@pytest.fixture(scope="module")
def front():
    rng = np.random.default_rng(fl.seed_of("solve_tails/sharpness", 0))
    w = 23
    return np.tril(rng.uniform(-1.0, 1.0, (w, w)), -1), rng.uniform(-1.0, 1.0, w)


def test_another_accumulator_changes_bits(front):
    L, f = front
    ref = solve_rows(L, f)
    assert fc.same_bits(ref, solve_rows(L, f))
    other = solve_rows(L, f, tail="a_u")
    assert not fc.same_bits(ref, other) and not np.array_equal(ref, other)
    assert np.allclose(ref, other, rtol=0, atol=1e-13)          # the same sum: only a bitwise comparison sees it


def test_reversed_leftover_order_changes_bits(front):
    L, f = front
    ref, other = solve_rows(L, f), solve_rows(L, f, tail="reversed")
    assert not fc.same_bits(ref, other) and not np.array_equal(ref, other)
    assert np.allclose(ref, other, rtol=0, atol=1e-13)


def test_zero_times_an_infinite_neighbour_is_not_a_skip(front):
    L, f = front
    beyond = np.array([np.inf, 1.0, 1.0])
    ref = solve_rows(L, f)
    with np.errstate(invalid="ignore"):
        other = solve_rows(L, f, tail="zero_fill", beyond=beyond)
    assert np.isfinite(ref).all()
    assert np.isnan(other).any() and not np.array_equal(ref, other)
    # with finite neighbours the zero is invisible (the accumulators start at +0.0), which is why finite fixtures alone
    # would not catch it and the kernels' leftover batches are read for it: load and multiply-add under one predicate
    assert fc.same_bits(ref, solve_rows(L, f, tail="zero_fill", beyond=np.ones(3)))


def test_fixtures_are_there_and_small():
    total = 0
    for family, cases in (("fused", st.FUSED_CASES), ("lvl", st.LVL_CASES)):
        for c in cases:
            p = st.golden_path(family, c)
            assert os.path.isfile(p), p
            g = st.load_golden(family, c)
            assert all(v.dtype == np.float64 for k, v in g.items() if k.startswith(("x", "io_")))
            total += os.path.getsize(p)
    assert total < 1 << 20
