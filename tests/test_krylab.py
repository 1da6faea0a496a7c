"""-m "not gpu": the vector, reduction and update launchers of the native Krylov solver, their batched forms and spmv_mv one
by one (tests/krylab) on the test-only simulators, against the numpy references of the lab.  On the simulator a batched
launcher is a loop over the single one, so this run proves the harness, the references, the canaries, the bounds and the
coverage bookkeeping on a machine without a GPU, and that every check bites (perturbations, numpy mutants, stray writes);
tests/test_krylab_gpu.py runs the same cases through the product library and pins the kernels."""
import importlib.util
import os
import sys

import numpy as np
import pytest

LAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "krylab")


def _load(name):
    """tests/krylab/<name>.py as module krylab_<name> (the other labs have modules of the same file names)."""
    key = "krylab_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(LAB, name + ".py"))
        sys.modules[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[key])
    return sys.modules[key]


kl = _load("cases")

_results = {}


@pytest.fixture(scope="module")
def sim():
    return kl.load("sim")


def result(sim, case):
    """The simulator's output buffers of one case (kept only where they are small)."""
    if case.name in _results:
        return _results[case.name]
    res = kl.run_case(sim, case)
    if sum(v.nbytes for v in res.values()) < (1 << 20):
        _results[case.name] = res
    return res


def copy_of(res):
    return {k: v.copy() for k, v in res.items()}


@pytest.mark.parametrize("case", kl.CASES, ids=[c.name for c in kl.CASES])
def test_case_matches_reference(sim, case):
    fails, ratio = kl.check_case(case, result(sim, case))
    print("krylab sim: %-34s error / bound %.3g" % (case.name, ratio))
    assert fails == []


def test_case_list_covers_every_branch(sim):
    assert sorted(kl.REQUIRED - kl.coverage(sim, kl.CASES)) == []


def test_coverage_notices_a_missing_case(sim):
    """The coverage check itself: each of these cases is the only one that reaches its branch."""
    for names, tag in ((["dot_524288"], "dot:full_grid_one_trip"), (["update_f64_n257_k0", "update_f32_n257_k0"], "update:k=0"),
                       (["cg_xr_mv_n257_nb5"], "cg_xr_mv:nb=5 refused")):
        got = kl.coverage(sim, [c for c in kl.CASES if c.name not in names])
        assert kl.REQUIRED - got == {tag}
    got = kl.coverage(sim, [c for c in kl.CASES if not (c.family == "spmv_mv" and c.p["nv"] in (2, 6))])
    assert kl.REQUIRED - got == {"spmv_mv:group=2"}
    got = kl.coverage(sim, [c for c in kl.CASES if not (c.family == "dot" and c.p["n"] >= 524289)])
    assert kl.REQUIRED - got == {"dot:second_trip"}


# ---- sharpness of the bounds: a relative perturbation of 1e-9 in one output entry fails the check
SHARP = [("dot_257", "out", 0), ("dot_65537", "out", 0), ("cg_xr_257", "x1", 200), ("cg_xr_257", "r0", 256), ("cg_xr_257", "out1", 0),
         ("cg_p_257", "p0", 256), ("cg_p_65537", "p1", 65536), ("update_f64_n257_k9_ld5", "x", 256), ("update_f32_n4099_k256_ld0", "x", 4098),
         ("dot_mv_n257_nb3", "O", 2 * kl.MV_OUT_STRIDE), ("cg_xr_mv_n257_nb4", "Y", None), ("cg_xr_mv_n257_nb4", "R", None),
         ("cg_xr_mv_n257_nb4", "O", 3 * kl.MV_OUT_STRIDE), ("cg_p_mv_n65537_nb2", "Y", None), ("spmv_mv_65_L4_nv7", "y2", None),
         ("spmv_mv_257_L1_nv6", "y0", None)]


def last_written(buf):
    """Index of the last element of buf that does not hold the canary bits."""
    raw = np.uint64 if buf.dtype.itemsize == 8 else np.uint32
    want = np.full(buf.nbytes // 8, kl.CANARY, dtype=np.uint64).view(raw)
    return int(np.flatnonzero(buf.view(raw) != want)[-1])


@pytest.mark.parametrize("name,key,pos", SHARP, ids=["%s-%s" % (n, k) for n, k, _ in SHARP])
def test_bound_catches_a_perturbed_entry(sim, name, key, pos):
    case = kl.BY_NAME[name]
    assert case.family in kl.BOUNDED_FAMILIES
    res = result(sim, case)
    assert kl.check_case(case, res)[0] == []
    bad = copy_of(res)
    if pos is None:     # the last entry the launcher wrote: the last row of the last column
        pos = last_written(bad[key])
    assert bad[key][pos] != 0.0 and np.isfinite(bad[key][pos])
    bad[key][pos] *= 1 + 1e-9
    fails = kl.check_case(case, bad)[0]
    assert any("above the bound" in f for f in fails), fails


def test_every_bounded_family_has_a_perturbation():
    assert {kl.BY_NAME[n].family for n, _, _ in SHARP} == set(kl.BOUNDED_FAMILIES)


# ---- the bitwise families: the lowest mantissa bit of one entry
FLIP = [("sub_257", "o", 256), ("add_255", "o", 254), ("div_65537", "o", 65536), ("scale_by_257_pos", "o", 0), ("scale_by_257_neg", "o", 256),
        ("widen_257", "o", 3), ("round_div_257", "o", 256), ("round_div_crafted_s2", "o", 11), ("round_scale_by_257_nan", "o", 100),
        ("round_scale_by_crafted_s1", "o", 0), ("scale_by_mv_n257_nb3", "Y", None), ("round_scale_by_mv_n257_nb4", "Y", None),
        ("widen_mv_n65537_nb2", "Y", None)]


@pytest.mark.parametrize("name,key,pos", FLIP, ids=["%s-%s" % (n, k) for n, k, _ in FLIP])
def test_exact_check_catches_a_flipped_bit(sim, name, key, pos):
    case = kl.BY_NAME[name]
    assert case.family in kl.BITWISE_FAMILIES
    res = result(sim, case)
    assert kl.check_case(case, res)[0] == []
    bad = copy_of(res)
    raw = bad[key].view(np.uint64 if bad[key].dtype.itemsize == 8 else np.uint32)
    if pos is None:
        pos = last_written(bad[key])
    raw[pos] ^= raw.dtype.type(1)
    fails = kl.check_case(case, bad)[0]
    assert any("restatement" in f for f in fails), fails


def test_every_bitwise_family_has_a_flipped_bit():
    assert {kl.BY_NAME[n].family for n, _, _ in FLIP} == set(kl.BITWISE_FAMILIES)


# ---- numpy mutants: a float64 restatement with one defect substituted for the output fails the reference check, the
# restatement without the defect passes it
def reference_fails(case, res):
    """The failures of the reference checks alone (not the comparison with the single launch, not the canaries)."""
    return [f for f in kl.check_case(case, res)[0] if "above the bound" in f or "restatement" in f or "above any bound" in f]


@pytest.mark.parametrize("mutant,names", [
    ("ragged", ["dot_1", "dot_255", "dot_257", "dot_65281", "dot_65537", "dot_524289", "dot_1048579"]),
    ("first256", ["dot_65537", "dot_524288", "dot_524289", "dot_1048579"])])
def test_dot_check_catches_a_mutant(sim, mutant, names):
    for name in names:
        case = kl.BY_NAME[name]
        res = result(sim, case)
        assert kl.check_case(case, kl.restate_dot(case, res))[0] == [], name
        assert reference_fails(case, kl.restate_dot(case, res, mutant)), (mutant, name)


@pytest.mark.parametrize("mutant,names", [
    ("swap12", ["%s_n%d_nb%d" % (op, n, nb) for op in kl.MV_OPS if op != "dot_mv" for n in (1, 257, 65537) for nb in (3, 4)]),
    ("alpha0", ["cg_xr_mv_n%d_nb%d" % (n, nb) for n in (1, 257, 65537) for nb in (2, 3, 4)])])
def test_batched_check_catches_a_mutant(sim, mutant, names):
    """Columns 1 and 2 exchanged; column 0's alpha used for every column."""
    for name in names:
        case = kl.BY_NAME[name]
        res = result(sim, case)
        assert kl.check_case(case, kl.restate_mv(case, res))[0] == [], name
        assert reference_fails(case, kl.restate_mv(case, res, mutant)), (mutant, name)


def test_scale_by_check_catches_a_division_by_a_negative_scalar(sim):
    for name in ("scale_by_257_neg", "scale_by_65537_neg"):
        case = kl.BY_NAME[name]
        res, inp = result(sim, case), kl.inputs(case)
        good, bad = copy_of(res), copy_of(res)
        good["o"][:case.p["n"]] = inp["a"]
        bad["o"][:case.p["n"]] = inp["a"] / inp["s"][0]
        assert kl.check_case(case, good)[0] == []
        assert reference_fails(case, bad), name


def test_round_div_check_catches_a_quotient_of_rounded_operands(sim):
    """float32(x) / float32(s) instead of float32(x / s): random entries with a divisor that is no power of two, and the
    crafted entry whose quotient by 2 is a float subnormal."""
    for name in ["round_div_%d" % n for n in kl.N_LIST if n >= 255] + ["round_div_crafted_s2"]:
        case = kl.BY_NAME[name]
        res, inp = result(sim, case), kl.inputs(case)
        n, s = case.p["n"], inp["s"][0]
        good, bad = copy_of(res), copy_of(res)
        good["o"][:n] = (inp["a"] / s).astype(np.float32)
        bad["o"][:n] = inp["a"].astype(np.float32) / np.float32(s)
        assert kl.check_case(case, good)[0] == []
        assert reference_fails(case, bad), name
    case = kl.BY_NAME["round_div_crafted_s2"]
    x = kl.inputs(case)["a"][11:12]
    assert (x / 2.0).astype(np.float32) != x.astype(np.float32) / np.float32(2.0)


@pytest.mark.parametrize("mutant,names", [
    ("ldy", ["spmv_mv_%d_L%d_nv%d" % (n, L, nv) for n in (1, 63, 257) for L in (1, 8) for nv in (2, 3, 4, 6, 9)]),
    ("beta_nan", ["spmv_mv_%d_L%d_nv%d" % (n, L, nv) for n in (1, 65) for L in (2, 4) for nv in (1, 5, 7)])])
def test_spmv_mv_check_catches_a_mutant(sim, mutant, names):
    """X read with ldy instead of ldx; beta y formed where beta = 0 and y holds NaN."""
    for name in names:
        case = kl.BY_NAME[name]
        res = result(sim, case)
        assert reference_fails(case, kl.restate_spmv(case, res)) == [], name
        assert reference_fails(case, kl.restate_spmv(case, res, mutant)), (mutant, name)


# ---- canaries
def test_canary_check_notices_a_stray_write(sim):
    """One word behind an output, one word inside the gap between two columns, a partial too many, out[1]."""
    case = kl.BY_NAME["sub_257"]
    bad = copy_of(result(sim, case))
    bad["o"][257] = 0.0
    assert kl.check_case(case, bad)[0] != []
    case = kl.BY_NAME["cg_p_mv_n257_nb3"]
    off = kl.mv_layout(case)[0]
    bad = copy_of(result(sim, case))
    assert bad["Y"].view(np.uint64)[off[0] + 257] == np.uint64(kl.CANARY) and off[1] > off[0] + 257
    bad["Y"][off[0] + 257] = 0.0
    assert kl.check_case(case, bad)[0] != []
    case = kl.BY_NAME["spmv_mv_63_L2_nv3"]
    bad = copy_of(result(sim, case))
    bad["y1"][63] = 1.0                                  # the first word of the gap behind column 0 (ldy = nrows + 5)
    assert kl.check_case(case, bad)[0] != []
    case = kl.BY_NAME["dot_257"]
    for key, pos in (("part", 2), ("out", 1)):
        bad = copy_of(result(sim, case))
        bad[key][pos] = 0.0
        assert kl.check_case(case, bad)[0] != []
    res = result(sim, case)
    assert int((res["part"].view(np.uint64) != np.uint64(kl.CANARY)).sum()) == 2     # exactly vec_grid(257) partials
