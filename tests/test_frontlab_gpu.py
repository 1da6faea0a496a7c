"""-m gpu: the batched multifrontal LU front by front on the MI355X (tests/frontlab through the product library), against a
float64 LAPACK reference, under every switch of the factorisation kernels.

Every environment variant runs in a child process of its own (the switches are read once per process) with a time limit;
after the first child that fails, times out or dies from a signal no further GPU child is started."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "frontlab"))
import cases as fl  # noqa: E402
import child as flchild  # noqa: E402

VARIANTS = [
    ("default", {}),
    ("gemm_tile_64", {"HYMLS_MI_GEMM_TILE": "64"}),
    ("gemm_tile_128", {"HYMLS_MI_GEMM_TILE": "128"}),
    ("outer_block_128", {"HYMLS_MI_OUTER_BLOCK": "128"}),      # plain right-looking order
    ("pivot_scalar", {"HYMLS_MI_PIVOT_BLOCKED": "0"}),        # every pivot piece on k_big_pivot
    ("trmm_scalar", {"HYMLS_MI_TRMM_SCALAR": "1"}),           # panel products on k_big_trmm_u / _l
    ("solve_kt_1024", {"HYMLS_MI_SOLVE_KT": "1024"}),         # 1024-column tiles of the big-front solve
    ("wide_factor_flops", {"HYMLS_MI_WIDE_FACTOR_FLOPS": "1000"}),   # one-workgroup fronts pushed onto the wide path
]
CHILD_TIMEOUT = 240
_SWITCHES = {k for _, env in VARIANTS for k in env}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """variant -> output directory, or the reason it has no results."""
    fl.build("gpu")
    base = tmp_path_factory.mktemp("frontlab")
    out, failed = {}, None
    for name, env in VARIANTS:
        if failed:
            out[name] = "not started: variant %s failed before" % failed
            continue
        e = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        e.update(env)
        d = str(base / name)
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "frontlab", "child.py"), d], env=e,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            out[name] = "timed out after %d s" % CHILD_TIMEOUT
            failed = name
            continue
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            out[name] = "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
            failed = name
            continue
        out[name] = d
    return out


_refs = {}


def reference(case):
    if case.name not in _refs:
        _refs[case.name] = fl.reference(case)
    return _refs[case.name]


def results(runs, variant):
    d = runs[variant]
    assert os.path.isdir(d), "variant %s: %s" % (variant, d)
    return {c.name: flchild.load(d, c) for c in fl.CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [v for v, _ in VARIANTS])
def test_fronts_match_lapack(runs, variant):
    res = results(runs, variant)
    bad = []
    for case in fl.CASES:
        r = res[case.name]
        main = r["main"]
        bad += ["%s: canary: %s" % (case.name, m) for m in fl.canary_failures(case, main)]
        want = fl.expected_flag(case)
        if case.tweak:
            if not main["flag"] & want:
                bad.append("%s: flag %d lacks bit %d" % (case.name, main["flag"], want))
            continue
        if main["flag"] != 0:
            bad.append("%s: flag %d (growth %.3g)" % (case.name, main["flag"], main["growth"]))
        bad += ["%s: %s" % (case.name, m) for m in fl.accuracy_failures(case, main, reference(case))]
        if case.repro:
            for key in ("S", "x"):
                if not fl.same_bits(r["chunked"][key], main[key]):
                    bad.append("%s: chunked run differs from the unchunked one in %s" % (case.name, key))
                if not fl.same_bits(r["alone"][key][0], main[key][1]):
                    bad.append("%s: member 1 factored alone differs from the batch in %s" % (case.name, key))
    assert bad == []


@pytest.mark.gpu
def test_gemm_tiles_give_identical_bits(runs):
    ref = results(runs, "default")
    for variant in ("gemm_tile_64", "gemm_tile_128"):
        other = results(runs, variant)
        diff = [c.name for c in fl.CASES if not c.tweak and
                not (fl.same_bits(ref[c.name]["main"]["S"], other[c.name]["main"]["S"]) and
                     fl.same_bits(ref[c.name]["main"]["x"], other[c.name]["main"]["x"]))]
        assert diff == [], "%s differs from the default tile choice" % variant


@pytest.mark.gpu
def test_case_list_covers_every_branch(runs):
    res = results(runs, "default")
    got = fl.coverage([(c, res[c.name]["main"]) for c in fl.CASES] +
                      [(c, res[c.name]["chunked"]) for c in fl.CASES if c.repro])
    assert sorted(fl.REQUIRED_GPU - got) == []


@pytest.mark.gpu
def test_growth_flag_on_every_pivot_kernel(runs):
    """Bit 2 on the one-workgroup path (LDS and global memory) and on both pivot-piece kernels of the wide path."""
    res = results(runs, "default")
    for name in ("dense_w20_s2_growth", "dense_w80_s2_growth", "dense_w64_s2_growth_wide", "dense_w65_s2_growth_wide"):
        main = res[name]["main"]
        assert main["flag"] == 2 and main["growth"] > 1e8, (name, main["flag"], main["growth"])
