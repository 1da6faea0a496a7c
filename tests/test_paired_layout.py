"""The paired panel layout (device.hpp: paired_lower / paired_l21 / paired_q, restated in tests/paired_layout.py): every slot
of each region is written exactly once and no region changes its size; and the classes of tests/paired_cases.py, planned
by the host simulator, reach every branch of the paired loops."""
import numpy as np
import pytest

import paired_cases as pc
import paired_layout as pl

WIDTHS = list(range(1, 10)) + [40]
UPDATE_ROWS = (0, 1, 3, 4, 5, 37)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("ri", UPDATE_ROWS)
def test_every_slot_is_hit_exactly_once(w, ri):
    ld, low = w + ri, w * (w - 1) // 2
    i, k = np.meshgrid(np.arange(ld), np.arange(w), indexing="ij")
    i, k = i.T.reshape(-1), k.T.reshape(-1)          # t = i + ld k
    dst, packed = pl.lside_index(w, ri, True), pl.lside_index(w, ri, False)
    regions = {"lower": ((i > k) & (i < w), 0, low), "l21": (i >= w, low, low + ri * w), "upper": (i <= k, low + ri * w, ld * w)}
    for name, (mask, begin, end) in regions.items():
        assert mask.sum() == end - begin, name
        assert sorted(dst[mask].tolist()) == list(range(begin, end)), "%s: not a permutation of its region" % name
        assert sorted(packed[mask].tolist()) == list(range(begin, end)), "%s (packed)" % name
    assert np.array_equal(dst[regions["upper"][0]], packed[regions["upper"][0]]), "the upper triangle stays as it is"
    assert sorted(pl.q_index(w, ri).tolist()) == list(range(w * ri)), "Q: not a permutation of its region"


@pytest.mark.parametrize("w", WIDTHS)
def test_a_pair_is_two_neighbouring_entries(w):
    """What the kernel relies on: entries (r, 2j) and (r, 2j + 1) of a row sit side by side wherever it reads a pair."""
    ri = 5
    for r in range(w + ri):
        kmax = min(r, w)
        for j in range(kmax // 2):
            a = (pl.paired_lower(w, r, 2 * j), pl.paired_lower(w, r, 2 * j + 1)) if r < w else \
                (pl.paired_cols(ri, w, r - w, 2 * j), pl.paired_cols(ri, w, r - w, 2 * j + 1))
            assert a[1] == a[0] + 1, (w, r, j)
    for i in range(w):
        for j in range(ri // 2):
            assert pl.paired_cols(w, ri, i, 2 * j + 1) == pl.paired_cols(w, ri, i, 2 * j) + 1


def test_cases_reach_every_branch():
    lab = pc.fc.load("sim")
    reached = set()
    for case in pc.CASES:
        lab.reset()
        for c in case.classes:
            reached |= pc.tags_of(lab.plan(c.pattern(), [0], c.leaf, c.max_width, True))
    lab.reset()
    assert pc.REQUIRED - reached == set()
