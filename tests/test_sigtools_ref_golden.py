"""The NumPy restatement tests/sigtools_ref.py against the reference's own
numbers (tests/golden/sigtools.npz, written by make_golden_sigtools.py).
CPU only.  medianFilter and invHermMat2D bit-equal; prinComp2D (direct sums
against fftconvolve) and f0detectionFunction within DESIGN.md §7.4's bounds.
"""
import os

import numpy as np
import pytest

import sigtools_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sigtools.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", sorted(S.MEDIAN_CASES))
def test_median_bit_equal(g, name):
    x, length = S.median_input(name)
    assert same(x, g['med_%s_in' % name])
    assert same(S.median_filter(x, length), g['med_%s_out' % name])


@pytest.mark.parametrize("name", sorted(S.inv_inputs()))
def test_invherm_bit_equal(g, name):
    res = S.inv_herm_2d(*S.inv_inputs()[name])
    for k, v in zip(('i00', 'i01', 'i11'), res):
        assert same(v, g['inv_%s_%s' % (name, k)]), k


@pytest.mark.parametrize("name", sorted(S.PCA_CASES))
def test_pca_within_bounds(g, name):
    X0, X1, nb = S.pca_inputs(name)
    assert same(X0, g['pca_%s_X0' % name]) and same(X1, g['pca_%s_X1' % name])
    ref = [g['pca_%s_%s' % (name, k)] for k in ('lambdaM', 'lambdam', 'vM', 'vm')]
    got = S.prin_comp_2d(X0, X1, nb, with_den=True)
    e = S.pca_errors(got[:4], ref, got[4], got[5])
    print(name, e)
    for k in ('lambdaM', 'lambdam', 'vM', 'vm'):
        assert e[k] < S.BOUND[k], (k, e)
    if name in S.PCA_TABLE:
        assert e['excluded'] <= S.EXCLUDED_MAX, e


def test_pca_zero_row_replacements(g):
    """den == 0 on the exact-zero row, in the reference's numbers too."""
    for src in (S.prin_comp_2d(*S.pca_inputs('zero_row')),
                [g['pca_zero_row_' + k] for k in ('lambdaM', 'lambdam', 'vM', 'vm')]):
        assert np.all(src[2][0, 1] == 1) and np.all(src[2][1, 1] == 0)
        assert np.all(src[3][0, 1] == 0) and np.all(src[3][1, 1] == 1)
        assert np.all(src[0][1] == 0) and np.all(src[1][1] == 0)


@pytest.mark.parametrize("name", sorted(S.HS_CASES))
def test_hs_within_bound(g, name):
    TF, kw = S.hs_input(name)
    assert same(TF, g['hs_%s_TF' % name])
    hs, f0 = S.f0_detection(TF, **kw)
    assert same(f0, g['hs_%s_f0' % name])
    assert hs.shape == g['hs_%s_hs' % name].shape
    assert np.array_equal(hs == 0, g['hs_%s_hs' % name] == 0)
    e = S.hs_error(hs, g['hs_%s_hs' % name])
    print(name, e)
    assert e < S.BOUND['hs']


def test_hs_cases_cover_what_they_claim(g):
    """Harmonics inside the axis, past its last bin, F0s with no bin at all,
    and harmonics with several bins (the max)."""
    from pyfasst_amd.tools import signalTools as st  # host code only
    TF, kw = S.hs_input('sum')
    f0 = g['hs_sum_f0']
    fr = np.arange(65) * 44100 / 128.
    assert f0[-1] * kw['numberHarmonics'] > fr[-1] > f0[0]
    assert np.any(g['hs_sum_hs'] == 0)
    ptr, idx = st.harmonic_bins(fr, f0, kw['numberHarmonics'], 1.5)
    assert np.max(np.diff(ptr)) > 1


def test_harmonic_bins_interval_search_is_the_full_test():
    """The interval search of harmonic_bins selects what the reference's
    expression selects on every bin (its fallback for an unsorted axis)."""
    from pyfasst_amd.tools import signalTools as st
    fr = np.arange(65) * 44100 / 128.
    for thr in (0.5, 1.5, 0., 7.):
        f0 = st.f0_table(300., 2500., 2)
        ptr, idx = st.harmonic_bins(fr, f0, 12, thr)
        perm = np.random.RandomState(0).permutation(65)
        ptr2, idx2 = st.harmonic_bins(fr[perm], f0, 12, thr)  # not increasing: full test
        assert np.array_equal(ptr, ptr2)
        for a, b in zip(ptr[:-1], ptr[1:]):
            assert np.array_equal(idx[a:b], np.sort(perm[idx2[a:b]]))


def test_sort_spectrum(g):
    res = S.sort_spectrum(g['sort_in'], S.SORT_HS, S.SORT_HP, **S.SORT_KW)
    assert same(res[1], g['sort_f0s']) and same(res[0], g['sort_sorted'])
    assert same(res[4], g['sort_f0table'])
    assert S.hs_error(res[2], g['sort_hs']) < S.BOUND['hs']
    assert S.hs_error(res[3], g['sort_hp']) < S.BOUND['hs']
