"""The GEMM layer's host arithmetic (pyfasst_amd/csrc/fasst_gemm.hip:
tile_shape, gemm_plan, gemm_workspace) through fasst_gemm_plan.

CPU-only: fasst_gemm_plan makes no device call.  k_gemm writes split z of
output b at work + (b nz + z) M N, so a workspace that disagrees with the
plan, an empty split or a K range that is no multiple of the 16-row chunk is
an out-of-bounds write or a lost k-term on the device; here they are
arithmetic.
"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyfasst_amd", "csrc")

MN = (1, 16, 47, 48, 49, 64, 65, 128, 129, 300)
KS = (1, 15, 16, 17, 63, 64, 127, 128, 129, 130, 200, 257, 1000, 1030, 2049)
NBS = (1, 2, 4)


def plan(M, N, K, NB):
    """(nz, kchunk, (wgm, wtm, wtn), work_doubles)"""
    from pyfasst_amd import _lib
    v = [ctypes.c_int(-1) for _ in range(5)]
    w = ctypes.c_longlong(-1)
    _lib.check(_lib.lib.fasst_gemm_plan(M, N, K, NB, *[ctypes.byref(x) for x in v], ctypes.byref(w)),
               "fasst_gemm_plan")
    nz, kchunk, wgm, wtm, wtn = (x.value for x in v)
    return nz, kchunk, (wgm, wtm, wtn), w.value


def promised_shape(M, N, NB):
    """tile_shape's comment, restated: the 48-wide single-wave strips for the
    skinny side, otherwise the largest tile 16 accumulators per wave allow."""
    if NB == 1:
        return (1, 3, 2) if M <= 48 else ((4, 2, 3) if N <= 48 else (2, 4, 4))
    if NB == 2:
        return (1, 3, 2) if M <= 48 else ((2, 2, 4) if M <= 64 else (2, 4, 2))
    return (1, 3, 1) if M <= 48 else (2, 2, 2)


@pytest.mark.parametrize("NB", NBS)
def test_plan_sweep(NB):
    for M in MN:
        for N in MN:
            shape = promised_shape(M, N, NB)
            for K in KS:
                nz, kchunk, got, work = plan(M, N, K, NB)
                what = "M %d N %d K %d NB %d -> nz %d kchunk %d" % (M, N, K, NB, nz, kchunk)
                assert got == shape, what
                assert NB * got[1] * got[2] <= 16, what
                assert nz >= 1 and kchunk >= 1, what
                if nz > 1:
                    assert kchunk % 16 == 0, what
                # every split owns at least one k, together they own all of K
                assert nz * kchunk >= K and (nz - 1) * kchunk < K, what
                assert work == (NB * nz * M * N if nz > 1 else 0), what
                if K < 128:
                    assert nz == 1, what


@pytest.mark.parametrize("NB", NBS)
def test_plan_recomputes_nz_from_the_rounded_chunk(NB):
    """K = 1030 on one tile doubles nz to 16; ceil(1030 / 16) = 65 rounds up to
    an 80-row chunk, and 13 of those cover K."""
    nz, kchunk, _, work = plan(40, 50, 1030, NB)
    assert (nz, kchunk) == (13, 80)
    assert work == NB * 13 * 40 * 50


def test_plan_does_not_split_a_full_grid():
    """16 x 131077 on 48 x 128 tiles is 1025 tiles: K = 128 could split in
    two, the grid is already full."""
    nz, kchunk, shape, work = plan(16, 131077, 128, 1)
    assert shape == (1, 3, 2)
    assert nz == 1 and work == 0
    # one column fewer is 1024 tiles, still full; 1023 tiles split
    assert plan(16, 131072, 128, 1)[0] == 1
    assert plan(16, 130944, 128, 1)[0] == 2


def test_callers_without_a_workspace_never_split():
    """sf_product (fasst_sfnmf.hip) runs gemm<false, false, 1> with work =
    nullptr and a padded ldc on the strength of 'gemm_plan never splits this
    product': K < kSfWide, any F x N."""
    src = open(os.path.join(CSRC, "fasst_sfnmf.hip")).read()
    wide = int(re.search(r"constexpr int kSfWide = (\d+);", src).group(1))
    call = re.search(r"// K < kSfWide: gemm_plan never splits this product.*?nullptr\);", src, re.S)
    assert call and "gemm<false, false, 1>" in call.group(0)
    assert re.search(r"f\.wide = f\.K >= kSfWide;", src)
    assert wide >= 2
    for M in MN + (1025, 2049):
        for N in MN + (1000, 10000):
            for K in range(1, wide):
                assert plan(M, N, K, 1)[0] == 1, (M, N, K)
    # the bound is the plan's own: the first K that can split is 128
    assert plan(40, 50, 127, 1)[0] == 1 and plan(40, 50, 128, 1)[0] == 2
    assert wide <= 128


def test_plan_refuses_bad_arguments():
    from pyfasst_amd import _lib
    for M, N, K, NB in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (-3, 4, 5, 2), (4, 4, 4, 0),
                        (4, 4, 4, 3), (4, 4, 4, 8)):
        assert _lib.lib.fasst_gemm_plan(M, N, K, NB, None, None, None, None, None, None) == \
            _lib.FASST_ERR_SHAPE
        assert "fasst_gemm_plan" in _lib.last_error()
    # null outputs are skipped
    assert _lib.lib.fasst_gemm_plan(40, 50, 1030, 1, None, None, None, None, None, None) == \
        _lib.FASST_OK
