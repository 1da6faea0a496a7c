"""Wave-level panel load instructions of one workgroup of the fused interior solve, counted from the plan tables of a class
(as tools/count_panel_trips.py counts round trips; the plan comes from the host simulator through tests/fusedlab, no GPU
needed): per sweep (forward L side, backward U11^-1, backward U-side panel Q)
  today   one load per column: 4 per trip of the unrolled k loop and wave, up to 3 predicated ones for the leftover
  paired  the panels the wide levels (more than 128 items) read in column pairs (device.hpp: FrontD::pair): 2 per trip,
          one pair and one single entry for the leftover; U11^-1 and the k-split levels as today
with the mean number of active lanes per instruction (of 64; a vector-memory instruction costs its issue slot whatever
that number is) and the share of the panel entries that lie in the wide levels, paired or not.  An instruction is counted
when at least one lane of the wave executes it.

usage: python tools/count_panel_loads.py [case ...]      (cases of tests/fusedlab/cases.py; default: the grid and saddle cases)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import solve_tails_cases as st  # noqa: E402
from count_panel_trips import DEFAULT, level_items  # noqa: E402

fc = st.fc


def wave_loads(n, paired):
    """n[wave][lane] = entries a thread adds in this loop.  (instructions, active lanes summed over them)"""
    ins = act = 0
    for lanes in n:
        main, rem = lanes // 4, lanes % 4
        per_trip = 2 if paired else 4
        for t in range(int(main.max(initial=0))):
            ins += per_trip
            act += per_trip * int((main > t).sum())
        tails = [rem >= 2, (rem & 1) == 1] if paired else [rem > u for u in range(3)]
        for m in tails:
            if m.any():
                ins += 1
                act += int(m.sum())
    return ins, act


def loop_loads(lengths, pairable):
    """One k loop over the items of a level.  {"today": (ins, act), "paired": (ins, act)}, entries, wide?"""
    ni = len(lengths)
    out = {"today": [0, 0], "paired": [0, 0]}
    if ni > 128:
        for p0 in range(0, ni, 256):
            per = np.zeros(256, dtype=np.int64)
            part = lengths[p0: p0 + 256]
            per[: len(part)] = part
            per = per.reshape(4, 64)
            per = per[per.max(axis=1) > 0] if per.max() > 0 else per[:0]
            for key, pr in (("today", False), ("paired", pairable)):
                i, a = wave_loads(per, pr)
                out[key][0] += i
                out[key][1] += a
        return out, int(lengths.sum()), True
    RT = 128 if ni > 64 else 64
    KG = 256 // RT
    per = np.zeros(256, dtype=np.int64)
    for tid in range(256):
        it, kg = tid % RT, tid // RT
        if it < ni:
            per[tid] = max(0, (lengths[it] - kg + KG - 1) // KG)
    i, a = wave_loads(per.reshape(4, 64), False)
    return {"today": [i, a], "paired": [i, a]}, int(lengths.sum()), False


def count(T):
    """{sweep: {"today": [ins, act], "paired": [ins, act], "entries": e, "wide": entries in wide levels}}"""
    out = {k: {"today": [0, 0], "paired": [0, 0], "entries": 0, "wide": 0} for k in ("forward L", "backward U11^-1", "backward Q")}
    for lev in range(T["nlev"]):
        fw, bw = level_items(T, lev)
        for key, lengths, pairable in (("forward L", [min(r, w) for w, ri, r in fw], True),
                                       ("backward U11^-1", [w - i for w, ri, i in bw], False),
                                       ("backward Q", [ri for w, ri, i in bw], True)):
            res, entries, wide = loop_loads(np.array(lengths, dtype=np.int64), pairable)
            for k in ("today", "paired"):
                out[key][k][0] += res[k][0]
                out[key][k][1] += res[k][1]
            out[key]["entries"] += entries
            out[key]["wide"] += entries if wide else 0
    return out


def main():
    names = sys.argv[1:] or DEFAULT
    lab = fc.load("sim")
    print("| class | nI | sweep | entries | in wide levels | loads today | lanes / load | loads paired | lanes / load | ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in names:
        case = fc.BY_NAME[name]
        lab.reset()
        for c in case.classes:
            T = lab.plan(c.pattern(), [0], c.leaf, c.max_width, c.packed)
            res = count(T)
            tot = {"today": [0, 0], "paired": [0, 0], "entries": 0, "wide": 0}
            for v in res.values():
                for k in ("today", "paired"):
                    tot[k][0] += v[k][0]
                    tot[k][1] += v[k][1]
                tot["entries"] += v["entries"]
                tot["wide"] += v["wide"]
            for key, v in list(res.items()) + [("all", tot)]:
                t, p = v["today"], v["paired"]
                print("| %s | %d | %s | %d | %.0f %% | %d | %.1f | %d | %.1f | %.2f |" % (
                    name, T["nI"], key, v["entries"], 100.0 * v["wide"] / max(v["entries"], 1), t[0], t[1] / max(t[0], 1),
                    p[0], p[1] / max(p[0], 1), p[0] / max(t[0], 1)))
            pairable = res["forward L"]["wide"] + res["backward Q"]["wide"]
            print("| %s | %d | entries in paired panels | %d | %.0f %% of all | | | | | |" % (name, T["nI"], pairable, 100.0 * pairable / max(tot["entries"], 1)))
        lab.reset()


if __name__ == "__main__":
    main()
