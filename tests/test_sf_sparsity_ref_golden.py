"""The restatement of reweigh_sparsity_constraint and of the sigma schedule
(tests/sf_sparsity_ref.py) against the REFERENCE's own run,
tests/golden/sf_sparse.npz (tests/golden/make_golden_sf_sparsity.py).  CPU only.

Bounds: the bare applications 1e-14 relative; the 4-iteration run the one
tests/test_sf_ref_golden.py holds sf_inst to: equality."""
import copy
import os

import numpy as np

import sf_sparsity_ref as SP
from helpers import GOLDEN, load, rel
from sf_ref import PARTS, fixture_oracle


def _oracle(g):
    o, X = fixture_oracle(g, SP.SPARSE_CASE)
    SP.set_sparsity(o, [int(L) for L in g['sparsity']])
    return o


def test_fixture_is_what_the_generator_describes():
    g = load('sf_sparse')
    assert os.path.getsize(os.path.join(GOLDEN, "sf_sparse.npz")) < 1 << 20
    assert list(g['sparsity']) == [int(L) for L in SP.SPARSE_LENGTHS] == [3, 0, 2]
    assert len(g['logliks']) == 4
    assert g['init_TW_0_0'].shape[0] == 13 and g['init_TW_2_0'].shape[0] == 4
    assert 'init_TW_2_1' not in g
    # the same model as sf_inst, which ran without the constraint
    s = load('sf_inst')
    np.testing.assert_array_equal(g['init_TW_0_0'], s['init_TW_0_0'])
    assert g['logliks'][0] == s['logliks'][0] and g['logliks'][1] != s['logliks'][1]


def test_sigma_schedule():
    g = load('sf_sparse')
    o = _oracle(g)
    sig = SP.sigma_schedule(o)
    assert sig.shape == (4,) and abs(sig[0] - 169.) < 1e-10 and abs(sig[-1] - 9.) < 1e-12
    np.testing.assert_allclose(sig[1:] / sig[:-1], (9. / 169.) ** (1. / 3.), rtol=1e-14)
    # one iteration: max(iter_num - 1, 1) keeps the first sigma
    assert abs(SP.sigma_schedule(o, 1)[0] - 169.) < 1e-10


def test_bare_reweigh_reproduces_the_reference():
    g = load('sf_sparse')
    for sigma in (169., 9.):
        o = _oracle(g)
        before = copy.deepcopy(o.spec_comps)
        SP.reweigh_sparsity_constraint(o, sigma)
        for k in range(3):
            ref = g['rw%d_TW_%d' % (sigma, k)]
            got = o.spec_comps[k]['factor'][0]['TW']
            assert rel(got, ref) < 1e-14, (sigma, k, rel(got, ref))
            changed = not np.array_equal(got, before[k]['factor'][0]['TW'])
            assert changed == bool(g['sparsity'][k]), (sigma, k)
        # factor 1 is never touched
        for k in range(2):
            np.testing.assert_array_equal(o.spec_comps[k]['factor'][1]['TW'],
                                          before[k]['factor'][1]['TW'])


def test_schedule_reproduces_the_reference():
    g = load('sf_sparse')
    o = _oracle(g)
    ll = SP.estim_param_a_post_model(o)
    np.testing.assert_array_equal(ll, g['logliks'])
    np.testing.assert_array_equal(o.noise['PSD'], g['final_psd'])
    for j in range(3):
        np.testing.assert_array_equal(np.array(o.spat_comps[j]['params']),
                                      g['final_params_%d' % j])
        for i, fac in o.spec_comps[j]['factor'].items():
            for part in PARTS:
                np.testing.assert_array_equal(fac[part], g['final_%s_%d_%d' % (part, j, i)],
                                              err_msg="%s %d %d" % (part, j, i))


def test_recorded_precision_gap_is_the_measured_one():
    """REWEIGH_TOL, the GPU tests' bound, is 16 x the float64 / longdouble gap
    of the restatement on the bare cases (floor 1e-13): the recorded gap is
    the measured one."""
    if np.finfo(np.longdouble).eps < 1e-18:   # (a longdouble wider than float64)
        gap = SP.precision_gap()
        print("precision gap %.4g" % gap)
        assert abs(gap / SP.PRECISION_GAP - 1.0) < 0.05, gap
    assert SP.REWEIGH_TOL == max(16 * SP.PRECISION_GAP, 1e-13)


def test_median_filter_windows():
    """The reference's windows: the last sample in none, an even count
    averaged, an empty window or a NaN giving the sample itself."""
    x = np.array([5., 1., 4., 2., 3.])
    np.testing.assert_array_equal(SP.median_filter(x, 1), [5., 3., 2.5, 3., 2.])
    np.testing.assert_array_equal(SP.median_filter(np.array([7.]), 3), [7.])
    y = np.array([1., np.nan, 2., 3.])
    np.testing.assert_array_equal(SP.median_filter(y, 1)[2:], [2., 2.])
    assert np.isnan(SP.median_filter(y, 1)[1])
