"""Dependent panel round trips on the critical path of one workgroup of the fused interior solve, counted from the plan
tables of a class (front table, fw_ptr / bw_ptr; the items of a level are its fronts in table order, rows in order, as
symbolic.cpp writes them) -- no GPU needed, the plan comes from the host simulator through tests/fusedlab.

A trip is one "loads, wait, multiply-adds" step of a k loop of k_interior_fused.  Per level and loop (forward L-side,
backward U11^-1, backward U-side panel) the workgroup pays the largest count among its waves, and a wave pays the largest
count among its lanes: unrolled-by-four main iterations, plus
  today    one trip per leftover entry (up to three),
  batched  one trip if any lane has a leftover entry.
A level of more than 256 items pays once per pass of the item loop.

usage: python tools/count_panel_trips.py [case ...]      (cases of tests/fusedlab/cases.py; default: the grid and saddle cases)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import solve_tails_cases as st  # noqa: E402

fc = st.fc
DEFAULT = ("grid7_8", "grid27_6", "saddle_4", "grid7_12_leaf4", "grid7_14")


def level_items(T, lev):
    """[(w, ri, row)] of the forward items and [(w, ri, pivot row)] of the backward items of one level."""
    fw, bw = [], []
    for w, ri, rs, parent, level in T["fronts"][:, :5]:
        if level == lev:
            fw += [(int(w), int(ri), r) for r in range(int(w + ri))]
            bw += [(int(w), int(ri), r) for r in range(int(w))]
    return fw, bw


def trips(lengths_per_thread):
    """lengths_per_thread[tid] = entries thread tid adds in this loop (256 threads; idle ones 0).  (today, batched)"""
    n = np.asarray(lengths_per_thread).reshape(4, 64)        # wave, lane
    main, rem = n // 4, n % 4
    today = (main.max(axis=1) + rem.max(axis=1)).max()
    batched = (main.max(axis=1) + (rem.max(axis=1) > 0)).max()
    return int(today), int(batched)


def loop_trips(lengths):
    """One k loop over the items of a level (lengths[it]); the split of the kernel: > 128 items one thread per item and
    passes of 256, else 2 (65 .. 128 items) or 4 thread groups share the k range of an item."""
    ni = len(lengths)
    today = batched = 0
    if ni > 128:
        for p0 in range(0, ni, 256):
            per = np.zeros(256, dtype=np.int64)
            part = lengths[p0: p0 + 256]
            per[: len(part)] = part
            t, b = trips(per)
            today, batched = today + t, batched + b
        return today, batched
    RT = 128 if ni > 64 else 64
    KG = 256 // RT
    per = np.zeros(256, dtype=np.int64)
    for tid in range(256):
        it, kg = tid % RT, tid // RT
        if it < ni:
            per[tid] = max(0, (lengths[it] - kg + KG - 1) // KG)
    return trips(per)


def count(T):
    """{loop: (today, batched)} summed over the levels of the class, and the number of level steps."""
    out = {"forward L": [0, 0], "backward U11^-1": [0, 0], "backward U-side": [0, 0]}
    for lev in range(T["nlev"]):
        fw, bw = level_items(T, lev)
        assert len(fw) == T["fw_ptr"][lev + 1] - T["fw_ptr"][lev] and len(bw) == T["bw_ptr"][lev + 1] - T["bw_ptr"][lev], \
            "the items of a level are not its fronts in table order"
        for key, lengths in (("forward L", [min(r, w) for w, ri, r in fw]), ("backward U11^-1", [w - i for w, ri, i in bw]),
                             ("backward U-side", [ri for w, ri, i in bw])):
            t, b = loop_trips(np.array(lengths, dtype=np.int64))
            out[key][0] += t
            out[key][1] += b
    return out


def main():
    names = sys.argv[1:] or DEFAULT
    lab = fc.load("sim")
    print("| class | nI | levels | loop | trips today | trips batched | ratio |")
    print("|---|---|---|---|---|---|---|")
    for name in names:
        case = fc.BY_NAME[name]
        lab.reset()
        for c in case.classes:
            pat = c.pattern()
            T = lab.plan(pat, [0], c.leaf, c.max_width, c.packed)
            res = count(T)
            tot = [sum(v[0] for v in res.values()), sum(v[1] for v in res.values())]
            for key, (t, b) in list(res.items()) + [("all", tot)]:
                print("| %s | %d | %d | %s | %d | %d | %.2f |" % (name, T["nI"], T["nlev"], key, t, b, b / max(t, 1)))
        lab.reset()


if __name__ == "__main__":
    main()
