"""The paired panel layout of the wide levels of the fused interior solve (hymls_amd/csrc/device.hpp: FrontD::pair, paired_lower /
paired_l21 / paired_q), restated in numpy for tests/test_paired_layout.py and tests/test_paired_panels_gpu.py, with the coverage
tags of a class computed from its plan tables (tests/fusedlab: Lab.plan)."""
import numpy as np

PAIR_L, PAIR_Q = 1, 2
WIDE = 128      # a level with more items than this is solved one thread per row: its panels are paired


def paired_cols(ld, ncol, i, k):
    """ld x ncol panel, rows on lanes: columns 2j, 2j + 1 interleaved row by row, a last odd column plain behind the pairs."""
    return np.where(k < (ncol & ~1), 2 * (ld * (k >> 1) + i) + (k & 1), ld * k + i)


def paired_lower(w, i, k):
    """Strictly lower triangle (i > k): pair-column j = k >> 1 holds the rows i >= 2j + 2, both entries; the entries
    (2j + 1, 2j) without a partner form a strip behind the pair-columns."""
    j = k >> 1
    return np.where(i >= 2 * j + 2, 2 * j * (w - 1 - j) + 2 * (i - 2 * j - 2) + (k & 1), w * (w - 1) // 2 - w // 2 + j)


def lside_index(w, ri, paired):
    """Where entry t = i + (w + ri) k of the column-major (w + ri) x w panel goes: [strictly lower triangle | L21 | upper
    triangle by columns], the first two paired or packed by columns (cases.py: packed_index)."""
    ld = w + ri
    i, k = np.meshgrid(np.arange(ld, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    low = w * (w - 1) // 2
    if paired:
        lower = paired_lower(w, i, k)
        l21 = low + paired_cols(ri, w, i - w, k)
    else:
        lower = k * (2 * w - k - 1) // 2 + (i - k - 1)
        l21 = low + (i - w) + ri * k
    upper = low + ri * w + k * (k + 1) // 2 + i
    dst = np.where(i >= w, l21, np.where(i > k, lower, upper))
    return dst.T.reshape(-1)


def q_index(w, ri):
    """Where entry t = i + w k of the w x ri panel Q goes in a front with PAIR_Q."""
    i, k = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(ri, dtype=np.int64), indexing="ij")
    return paired_cols(w, ri, i, k).T.reshape(-1)


def front_pairs(T):
    """FrontD::pair of every front of a class whose panels are paired: the L side iff the forward level of the front has
    more than 128 items, Q iff its backward level has."""
    fw, bw = np.diff(T["fw_ptr"]), np.diff(T["bw_ptr"])
    lev = T["fronts"][:, 4].astype(np.int64)
    return PAIR_L * (fw[lev] > WIDE) + PAIR_Q * (bw[lev] > WIDE)


def paired_reference(T, slab, members, swap=None):
    """The unpacked slab of a class with the panels of `members` in the paired layout.  swap = (front, t0, t1): exchange
    two targets of that front's L-side permutation (the mutant of the sharpness test)."""
    out = slab.copy()
    pairs = front_pairs(T)
    for s, (w, ri, rs, parent, level, c0, idx_off, lp_off, q_off, big) in enumerate(T["fronts"]):
        w, ri = int(w), int(ri)
        dst = lside_index(w, ri, bool(pairs[s] & PAIR_L))
        if swap is not None and swap[0] == s:
            dst[swap[1]], dst[swap[2]] = dst[swap[2]], dst[swap[1]]
        n = (w + ri) * w
        for b in members:
            out[b, lp_off + dst] = slab[b, lp_off: lp_off + n]
            if pairs[s] & PAIR_Q:
                out[b, q_off + q_index(w, ri)] = slab[b, q_off: q_off + w * ri]
    return out


TAGS = ({"pair_w_odd", "pair_w_even", "pair_r_odd", "pair_r_even", "pair_single_only", "pair_mixed_class", "pair_q_ri_odd",
         "pair_q_ri_even"} | {"pair_tail=%d" % t for t in range(4)} | {"pair_q_tail=%d" % t for t in range(4)})


def tags_of(T):
    """Which branches of the paired loops the class reaches.  A row of the L side of a front adds kmax = min(r, w) entries:
    kmax // 4 trips of two pair loads, then a leftover of kmax % 4 (pair_tail: one pair for 2 and 3, one single entry for 1
    and 3); a pivot row of Q adds ri."""
    tags = set()
    pairs = front_pairs(T)
    if np.any(pairs != 0) and np.any((pairs & PAIR_L) == 0):
        tags.add("pair_mixed_class")
    for (w, ri), pr in zip(T["fronts"][:, :2].astype(np.int64), pairs):
        if pr & PAIR_L:
            tags.add("pair_w_odd" if w & 1 else "pair_w_even")
            for r in range(1, int(w + ri)):
                kmax = min(r, int(w))
                if r < w:
                    tags.add("pair_r_odd" if r & 1 else "pair_r_even")
                if kmax == 1:
                    tags.add("pair_single_only")
                if kmax >= 4 or kmax % 4:
                    tags.add("pair_tail=%d" % (kmax % 4))
        if pr & PAIR_Q and ri > 0:
            tags.add("pair_q_ri_odd" if ri & 1 else "pair_q_ri_even")
            if ri >= 4 or ri % 4:
                tags.add("pair_q_tail=%d" % (ri % 4))
    return tags
