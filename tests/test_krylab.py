"""-m "not gpu": the vector, reduction and update launchers of the native Krylov solver, the orthogonalisation passes A, B
and C pass by pass, the projection and border-product launchers, their batched forms and spmv_mv one by one (tests/krylab)
on the test-only simulators, against the numpy references of the lab.  On the simulator a batched
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
    assert all(u == 0 for u in kl.SQRT_ULPS.values())    # out[k] of pass C: the host's sqrt is numpy's, bit for bit


def test_case_list_covers_every_branch(sim):
    assert sorted(kl.REQUIRED - kl.coverage(sim, kl.CASES)) == []


def test_coverage_notices_a_missing_case(sim):
    """The coverage check itself: each of these cases is the only one that reaches its branch."""
    for names, tag in ((["dot_524288"], "dot:full_grid_one_trip"), (["update_f64_n257_k0", "update_f32_n257_k0"], "update:k=0"),
                       (["cg_xr_mv_n257_nb5"], "cg_xr_mv:nb=5 refused"), (["pass_b_f32_n131072_k2"], "pass_b_f32:full_grid_one_trip"),
                       (["pass_c_f64_n524289_k3_basis"], "pass_c_f64:second_trip"), (["pass_c_mv_f64_n65_nb4_k0"], "pass_c_mv_f64:k=0 refused"),
                       (["proj_coeffs_n524289_m9"], "proj_coeffs:second_trip"), (["border_product_n257_m5"], "border_product:chunk_tail=5")):
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
         ("spmv_mv_257_L1_nv6", "y0", None),
         # a coefficient, a partial (the one of the ragged last tile), a row of w / dst, the squared norm, a d_j, a row of y
         ("pass_a_f64_n4099_k255", "H1", 254), ("pass_a_f64_n4099_k255", "P", 64 * 255 + 254), ("pass_a_f32_n4099_k62", "H1", 61),
         ("pass_a_f32_n65_k256", "P", 256 + 255), ("pass_b_f64_n4099_k149", "W", 4098), ("pass_b_f64_n4099_k149", "H2", 148),
         ("pass_b_f64_n65_k3", "P", 3 + 2), ("pass_b_f32_n4099_k61", "W", 0), ("pass_c_f64_n4099_k256_dst", "DST", 4098),
         ("pass_c_f64_n4099_k8_w", "W", 4098), ("pass_c_f64_n4099_k9_basis", "V", None), ("pass_c_f64_n4099_k256_dst", "O", 257),
         ("pass_c_f32_n4099_k256_dst", "P", 16), ("pass_a_mv_f64_n4099_nb4", "H1", None), ("pass_a_mv_f32_n65_nb2", "P", None),
         ("pass_b_mv_f32_n65_nb3", "W", None), ("pass_b_mv_f64_n4099_nb2", "P", None), ("pass_b_mv_f64_n4099_nb2", "H2", None),
         ("pass_c_mv_f64_n4099_nb2", "DST", None), ("pass_c_mv_f32_n65_nb3", "O", None), ("proj_coeffs_n257_m32", "H1", 31),
         ("proj_coeffs_n4099_m9", "H0", 8), ("proj_coeffs_n4099_m9", "P1", None), ("proj_update_n257_m7", "Y0", 256),
         ("proj_update_n4099_m32", "Y1", 0), ("oblique_project_n257_m17", "Y1", 256), ("oblique_project_n257_m8", "H0", 7),
         ("border_product_n4099_m9", "Y1", 4099 + 8), ("border_product_n4099_m9", "Y0", 100), ("border_product_n257_m32", "P1", None)]


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


# ---- the orthogonalisation passes, the projection and the border product
def test_pass_b_sum_check_catches_a_flipped_bit(sim):
    """out[j] = h1[j] + h2[j] is one add: the lowest mantissa bit of one entry fails.  So do two ulps in the norm of pass C."""
    for name, pos in (("pass_b_f64_n4099_k149", 148), ("pass_b_f32_n65_k4", 0), ("pass_b_mv_f32_n65_nb3", None)):
        case = kl.BY_NAME[name]
        res = result(sim, case)
        assert kl.check_case(case, res)[0] == []
        bad = copy_of(res)
        bad["O"].view(np.uint64)[last_written(bad["O"]) if pos is None else pos] ^= np.uint64(1)
        fails = kl.check_case(case, bad)[0]
        assert any("out = h1 + h2 differs from the restatement" in f for f in fails), fails
    case = kl.BY_NAME["pass_c_f64_n4099_k8_w"]
    bad = copy_of(result(sim, case))
    bad["O"].view(np.uint64)[8] += np.uint64(2)
    assert any("ulps from the restatement" in f for f in kl.check_case(case, bad)[0])


def fails_of_restatement(sim, name, restate, mutant):
    case = kl.BY_NAME[name]
    res = result(sim, case)
    assert kl.check_case(case, restate(case, res))[0] == [], name
    fails = reference_fails(case, restate(case, res, mutant))
    assert fails, (mutant, name)
    return fails


@pytest.mark.parametrize("mutant,names", [
    ("ragged", ["pass_a_f64_n1_k1", "pass_a_f64_n65_k3", "pass_a_f64_n4099_k255", "pass_a_f32_n63_k5", "pass_a_f32_n4099_k256",
                "pass_a_f64_n131073_k2"]),
    ("grid+1", ["pass_a_f64_n131073_k2", "pass_a_f32_n131073_k2", "pass_a_f64_n16385_k256"]),
    ("w_float", ["pass_a_f32_n65_k2", "pass_a_f32_n4099_k62", "pass_a_f32_n4099_k256"]),
    ("old_w", ["pass_b_f64_n1_k1", "pass_b_f64_n65_k5", "pass_b_f64_n4099_k149", "pass_b_f32_n4099_k61"]),
    ("drop3", ["pass_b_f64_n64_k4", "pass_b_f64_n65_k5", "pass_b_f64_n4099_k256", "pass_b_f32_n65_k255"]),
    ("h1", ["pass_c_f64_n1_k1_dst", "pass_c_f64_n4099_k9_basis", "pass_c_f64_n4099_k8_w", "pass_c_f32_n4099_k256_dst", "pass_c_f32_n257_k8_w"])])
def test_pass_check_catches_a_mutant(sim, mutant, names):
    """Pass A without the ragged last tile, with the tiles credited to the wrong workgroup, with w rounded to float; pass B
    with h2 from the old w, without the fourth quarter sum; pass C with h1."""
    for name in names:
        fails = fails_of_restatement(sim, name, kl.restate_pass, mutant)
        if mutant == "grid+1":                           # the coefficient and stage two are right: only the partials show it
            assert all("a partial against its rows" in f for f in fails), fails


@pytest.mark.parametrize("mutant,names", [
    ("G_T", ["proj_coeffs_n1_m2", "proj_coeffs_n257_m9", "proj_coeffs_n4099_m32", "border_product_n1_m2", "border_product_n257_m9",
             "border_product_n4099_m32"]),
    ("drop_chunk", ["proj_coeffs_n1_m1", "proj_coeffs_n257_m9", "proj_coeffs_n4099_m17", "proj_coeffs_n257_m32", "proj_coeffs_n257_m5"])])
def test_projection_check_catches_a_mutant(sim, mutant, names):
    """G applied transposed (the border tail: C read row-major); the dots without the last chunk of columns."""
    for name in names:
        fails_of_restatement(sim, name, kl.restate_proj, mutant)


def test_pass_canaries_notice_a_stray_write(sim):
    """A partial too many, out[k] after pass B, h2[0] after pass A, the padding behind column k - 1 of a basis that takes dst,
    the scratch of a batched column behind its own grid, and w after pass A."""
    def stray(name, key, pos, value=0.0):
        case = kl.BY_NAME[name]
        res = result(sim, case)
        assert kl.check_case(case, res)[0] == []
        bad = copy_of(res)
        assert bad[key].view(np.uint64)[pos] != np.float64(value).view(np.uint64)
        bad[key][pos] = value
        fails = kl.check_case(case, bad)[0]
        assert any("written outside its output set" in f for f in fails), (name, key, fails)
        return res
    res = stray("pass_a_f64_n65_k3", "P", 2 * 3)
    assert int((res["P"].view(np.uint64) != np.uint64(kl.CANARY)).sum()) == 2 * 3          # exactly grid * k partials
    stray("pass_b_f64_n65_k3", "O", 3)
    stray("pass_a_f64_n65_k3", "H2", 0)
    stray("pass_a_f32_n4099_k62", "W", 4098)
    case = kl.BY_NAME["pass_c_f64_n255_k9_basis"]
    assert case.p["ld"] == 260
    stray(case.name, "V", 8 * 260 + 255)
    stray(case.name, "H1", 0)
    case = kl.BY_NAME["pass_a_mv_f64_n65_nb3"]
    res = result(sim, case)
    stray(case.name, "P", int(res["tab"][3, 1]) + int(res["grid"][1]) * case.p["ks"][1])
    stray("proj_coeffs_n257_m9", "H0", 9)
    stray("proj_coeffs_n257_m9", "P1", 2 * 9)
    stray("proj_update_n257_m7", "H1", 0)
    stray("border_product_n257_m9", "Z1", 257)
    stray("border_product_n257_m9", "Y1", 257 + 9)


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
