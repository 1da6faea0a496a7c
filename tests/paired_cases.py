"""Cases of tests/test_paired_layout.py and tests/test_paired_panels_gpu.py: classes of tests/fusedlab/cases.py (imported,
nothing added to it), every class with packed panels, and the one shape that list lacks."""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import paired_layout as pl  # noqa: E402


def _load(key, path):
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, path)
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


fc = _load("fusedlab_cases", os.path.join(HERE, "fusedlab", "cases.py"))

_FROM_LAB = ("dense_w1", "saddle_4", "grid27_6", "grid7_8", "arrow_7x24_top37", "two_dense40_grid12")
CASES = [fc.Case(n, fc.BY_NAME[n].classes, a_lanes=fc.BY_NAME[n].a_lanes) for n in _FROM_LAB] + [
    # 40 leaves of one pivot row and three update rows each: a forward level of 160 items whose paired fronts have w = 1
    # (no pair at all, the single entry alone), a backward level of 40 (Q stays as it is)
    fc.Case("arrow_40x1_top3", [fc.ClassSpec("arrow", (40, 1, 3, 2), leaf=1, nb=2)], a_lanes=2),
]
REQUIRED = pl.TAGS | {"pair_w=1", "pair_l_only"}


def tags_of(T):
    """paired_layout.tags_of and the two tags of the added case."""
    tags = pl.tags_of(T)
    pairs = pl.front_pairs(T)
    if any(p & pl.PAIR_L and w == 1 and ri > 0 for (w, ri), p in zip(T["fronts"][:, :2], pairs)):
        tags.add("pair_w=1")
    if any(p == pl.PAIR_L for p in pairs):
        tags.add("pair_l_only")
    return tags
