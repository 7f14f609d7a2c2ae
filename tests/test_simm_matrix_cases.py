"""The SIMM kernel matrix on the CPU: the case table of simm_matrix_cases
covers every instantiation the restated dispatch can reach, the restatement's
constants are the ones in pyfasst_amd/csrc/fasst_simm.hip, and the longdouble
oracle the GPU tests are held to is a yardstick (no downcast on the way, and
the float64 oracle agrees with it to rounding on every case's inputs)."""
import os
import re

import numpy as np
import pytest

import simm_matrix_cases as M
from helpers import ROOT, rel_elem

SRC = os.path.join(ROOT, "pyfasst_amd", "csrc", "fasst_simm.hip")


def test_every_simm_arm_has_a_case():
    """Per ST two KM forms of k_simm_numden, k_hphi_partial, k_hgamma_rows and
    k_simm_wmt_xy (16), four of k_simm_xy_hmt (8), the three GEMM-path
    branches (6); stereo only: two of k_is_partial and two of k_alpha_partial
    (4); six k_simm_sm bodies; two NF0 product kernels, two mono HM rescales,
    three consumers of the pending scale, one / several slabs for each of the
    two skinny products (4): 51."""
    full = M.reachable_arms()
    assert len(full) == 51
    ids = [c.id for c in M.CASES]
    assert len(set(ids)) == len(ids)
    here = set()
    for c in M.CASES:
        arms = M.case_arms(c)
        assert arms <= full, (c.id, sorted(arms - full))
        here |= arms
    assert here == full, sorted(full - here)
    # the zero case adds no arm: it is not what pins one
    assert M.case_arms(M.ZERO_CASE) <= here

    # pairings the union does not show: who consumes the pending scale when
    # HGAMMA is fixed, the mono column scale on the GEMM path, the ragged
    # frame slab next to an odd N
    def some(pred):
        return any(pred(c, M.case_arms(c)) for c in M.CASES)
    assert some(lambda c, a: "pend@wmt" in a and "pend@hmt" not in a)
    assert some(lambda c, a: "pend@materialise" in a and not c.hgamma)
    assert some(lambda c, a: "pend@materialise" in a and c.hgamma and c.stereo)
    assert some(lambda c, a: {"hm_colscale", "xy_gemm<0>"} <= a)
    assert some(lambda c, a: {"hm_colscale", "xy_hmt<0,4,1>"} <= a)
    assert some(lambda c, a: {"hm_colscale", "xy_hmt<0,8,0>"} <= a)
    for N in (514, 515):
        nz, kchunk = M.hmt_split(130, N)
        assert nz == 2 and N - kchunk in (226, 227) and (N - kchunk) % 32 != 0
        assert some(lambda c, a: c.shape[:2] == (130, N) and "hmt_nzN" in a)
    nz, kchunk = M.wmt_split(520, 66)
    assert (nz, kchunk) == (11, 48) and 520 % kchunk != 0
    # the sizes the walker kernels and tiles turn at
    shapes = [c.shape for c in M.CASES]
    assert {255, 256, 257} <= {s[1] for s in shapes}
    assert {7, 17, 520} <= {s[0] for s in shapes}
    assert any(s[1] < 64 for s in shapes)
    assert {5, 8, 9, 17, 24, 25, 33, 41, 48, 49} <= {s[5] for s in shapes}
    # what keeps every case quick
    for s in shapes:
        assert (s[0] <= 300 or s[0] == 520) and s[1] <= 600 and s[2] <= 40, s


def test_restated_rule_at_its_edges():
    A = M.simm_arms
    assert A(70, 66, 4, 48, True, True, True) == {
        "numden<1,4>", "hphi_partial<1,4>", "hgamma_rows<1,4>", "is_partial<1,4>",
        "alpha_partial<4>", "nf0_dgemm2", "wmt_xy<1,4>", "xy_hmt<1,4,1>", "sm<48>", "wmt_nzN",
        "hmt_nz1", "pend@wmt", "pend@hmt"}
    assert A(70, 67, 5, 49, True, False, False, gemm_kind=2) == {
        "numden<1,8>", "hphi_partial<1,8>", "alpha_partial<8>", "nf0_kgemm", "wmt_gemm<1>",
        "xy_gemm<1>", "sm_gemm<1>", "pend@materialise"}
    # mono: HGAMMA always updated, recoError never filled
    assert A(16, 511, 8, 1, False, False, True) == {
        "numden<0,8>", "hphi_partial<0,8>", "hgamma_rows<0,8>", "nf0_dgemm2", "hm_rowscale",
        "wmt_xy<0,8>", "xy_hmt<0,8,0>", "sm<8>", "wmt_nz1", "hmt_nz1", "pend@wmt", "pend@hmt"}
    assert "hmt_nzN" in A(16, 512, 8, 1, False, True, False)
    with pytest.raises(ValueError):
        A(70, 66, 4, 3, False, True, False)
    with pytest.raises(ValueError):
        A(70, 66, 9, 3, True, True, False)
    # the splits at the benchmark's size (DESIGN: 313 x 8 and 33 x 15 blocks)
    assert M.wmt_split(2049, 20000)[0] == 8 and M.hmt_split(2049, 20000)[0] == 15
    # kWmtMaxChunk binds only past 16 x 512 bins, beyond any test's size: there
    # the restated nz = max(nz, chunks) line keeps every chunk within 512 bins
    assert M.wmt_split(9000, 66) == (18, 512) and M.wmt_split(8192, 20000) == (16, 512)
    # a device with fewer CUs moves the split, not the arms' names
    assert M.hmt_split(130, 514, slots=8) == M.hmt_split(130, 514)


def _one(pattern, text, rule):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: %d matches of %r in fasst_simm.hip" % (rule, len(found), pattern)
    return found[0]


def test_dispatch_constants_match_the_source():
    """The numbers and conditions simm_arms restates, read out of the
    source: a change to the dispatch fails here, naming the rule."""
    with open(SRC) as f:
        src = f.read()
    for name, want in (("kSimmKmax", M.K_MAX), ("kSmRmax", M.SM_RMAX),
                       ("kWmtMaxChunk", M.WMT_MAX_CHUNK), ("kSmRows", M.SM_ROWS)):
        got = int(_one(r"constexpr int %s = (\d+);" % name, src, name))
        assert got == want, "%s is %d in the source, %d in simm_matrix_cases" % (name, got, want)
    # the literal R > 48 tests (wmt_xy, xy_hmt, skinny_workspace) and refresh_sm's
    lit = re.findall(r"\bR > (\d+)\)", src)
    assert lit == [str(M.SM_RMAX)] * 3, "R > 48 tests: %r" % (lit,)
    _one(r"if \(c->R > kSmRmax\) return refresh_sm_gemm\(c\);", src, "refresh_sm's GEMM path")
    got = _one(r"const bool v16 = ([^;]+);", src, "v16")
    assert got == M.V16_RULE, "v16 is %r in the source" % got
    # kdispatch: KM = 4 for K <= 4, else 8
    body = _one(r"(?s)void kdispatch\(int K, L &&launch\) \{(.*?)\n\}", src, "kdispatch")
    assert re.findall(r"K <= (\d+)", body) == [str(M.KM_SMALL)], "kdispatch threshold"
    assert [int(v) for v in re.findall(r"integral_constant<int, (\d+)>", body)] == [
        M.KM_SMALL, M.K_MAX], "kdispatch KM values"
    # refresh_sm: RP = R rounded up to 8, one body per RP
    _one(r"const int RP = \(c->R \+ 7\) / 8 \* 8;", src, "refresh_sm RP")
    cases = _one(r"switch \(RP\) \{\s*((?:SM_CASE\(\d+\)\s*)+)\}", src, "refresh_sm SM_CASE list")
    assert tuple(int(v) for v in re.findall(r"\d+", cases)) == M.SM_BODIES
    # round_split, wmt_split, hmt_split, expression by expression
    for rule, pat in (
            ("round_split fullness", r"if \(eff >= 0\.95\) return nz;"),
            ("wmt_split bx", r"const long bx = \(N \+ 63\) / 64;"),
            ("wmt_split lo", r"const int lo = std::max\(std::max\(1, \(F \+ kWmtMaxChunk - 1\) / "
                             r"kWmtMaxChunk\),\s*\(int\)std::min<long>\(16, \(2 \* slots \+ bx - 1\)"
                             r" / bx\)\);"),
            ("wmt_split hi", r"int nz = round_split\(bx, lo, std::max\(lo, std::min\(16, F / 64\)\),"
                             r" slots\);"),
            ("wmt_split chunk floor", r"nz = std::max\(nz, \(F \+ kWmtMaxChunk - 1\) / "
                                      r"kWmtMaxChunk\);"),
            ("wmt_split kchunk", r"const int kchunk = \(\(F \+ nz - 1\) / nz \+ 15\) / 16 \* 16;"),
            ("wmt_split nz", r"return \{\(F \+ kchunk - 1\) / kchunk, kchunk\};"),
            ("hmt_split by", r"const long by = \(F \+ 63\) / 64;"),
            ("hmt_split hi", r"const int hi = std::max\(1, std::min\(32, N / 256\)\);"),
            ("hmt_split lo", r"const int nz = round_split\(by, std::min\(hi, \(int\)std::max<long>"
                             r"\(1, slots / \(2 \* by\)\)\), hi, slots\);"),
            ("hmt_split kchunk", r"const int kchunk = \(\(N \+ nz - 1\) / nz \+ 31\) / 32 \* 32;"),
            ("hmt_split nz", r"return \{\(N \+ kchunk - 1\) / kchunk, kchunk\};"),
            ("slots", r"c->slots = 2L \* ncu;"),
            ("mono always updates HGAMMA", r"c->stereo \? update_hgamma : 1,"),
            ("mono HM rescale", r"if \(R == 1\)\s*k_rowscale<<<")):
        _one(pat, src, rule)
    assert M.SPLIT_FULL == 0.95 and M.DEFAULT_SLOTS == 2 * 256


ALL = M.CASES + [M.ZERO_CASE]


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_longdouble_oracle_is_a_yardstick(case):
    """The longdouble run returns np.longdouble for every parameter (the
    random initial draws alone start as float64) and, but for recoError on
    the zero case, finite values; the float64 oracle is within 1e-13 of it
    elementwise, so the case's inputs are well enough conditioned for the GPU
    to be held to a small multiple of that."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for n_iter in case.iters:
        ref = M.oracle_run(case.id, n_iter, 'longdouble')
        f64 = M.oracle_run(case.id, n_iter, 'float64')
        for name, hi, lo in zip(M.names(case), ref, f64):
            assert hi.dtype == np.longdouble and lo.dtype == np.float64, (name, hi.dtype)
            assert hi.shape == lo.shape, name
            if case.zero and name == 'recoError':
                assert np.array_equal(np.isfinite(hi), np.isfinite(lo))
                assert np.isinf(hi[0]) and np.isinf(hi[1]) and np.isinf(hi[2])
                ok = np.isfinite(hi)
                hi, lo = hi[ok], lo[ok]
            assert np.all(np.isfinite(hi)), name
            e = rel_elem(lo, hi, floor=1e-12)
            assert e < 1e-13, (case.id, n_iter, name, e)
