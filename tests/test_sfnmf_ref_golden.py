"""The restatements of tests/sfnmf_ref.py (SFNMF_decomp_init,
multiChanSourceF0Filter.initializeFreeMats) against the REFERENCE's own runs,
tests/golden/sfnmf.npz (tests/golden/make_golden_sfnmf.py).  CPU only.

Bound: both sides run the same NumPy expressions in the same order, so bit
equality is expected; the assertion is 1e-14, max-normalised (helpers.rel)."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, load, rel
import sfnmf_ref as S
from sf_ref import PARTS, class_ref

BOUND = 1e-14


@pytest.fixture(scope="module")
def g():
    return load("sfnmf")


@pytest.mark.parametrize("case", sorted(S.SFNMF_CASES))
def test_restatement_reproduces_the_reference(g, case):
    SX, inits = S.case_inputs(case)
    np.testing.assert_array_equal(SX, g[case + '_SX'])
    for k, v in (inits or {}).items():
        np.testing.assert_array_equal(v, g['%s_%s' % (case, k)])
    assert int(g[case + '_seed']) == S.SFNMF_CASES[case][0]
    np.random.seed(int(g[case + '_seed']))
    res = S.sfnmf_decomp_init(SX, **dict(S.case_kwargs(case), **(inits or {})))
    assert np.random.rand() == float(g[case + '_rand'])
    s = S.SFNMF_SHAPE
    shapes = dict(W=(s['F'], s['K']), H=(s['K'], s['N']), WFilt=(s['F'], s['Kf']),
                  HFilt=(s['Kf'], s['N']), Wres=(s['F'], s['Kr']), Hres=(s['N'], s['Kr']))
    for n, v in zip(S.NAMES, res):
        ref = g['%s_%s' % (case, n)]
        assert v.shape == ref.shape == shapes[n], n
        assert rel(v, ref) < BOUND, (n, rel(v, ref))


def test_switched_off_factors_are_the_inputs(g):
    """What the fixtures say about the reference: a switched-off update leaves
    its factor as supplied, and with all four off only the residual moves."""
    off = {'w_off': 'W', 'h_off': 'H', 'wfilt_off': 'WFilt', 'hfilt_off': 'HFilt'}
    init = {'W': 'Winit', 'H': 'Hinit', 'WFilt': 'WFiltInit', 'HFilt': 'HFiltInit'}

    def supplied(case, n):
        a = g['%s_%s' % (case, init[n])]
        return a.T if n in ('H', 'HFilt') else a
    for case, n in off.items():
        # H is rescaled by the W update's column sums and by the HFilt
        # normalisation even when its own update is off
        if n in ('W', 'WFilt'):
            np.testing.assert_array_equal(g['%s_%s' % (case, n)], supplied(case, n))
    for n in init:
        np.testing.assert_array_equal(g['all_off_' + n], supplied('all_off', n))
    assert np.all(np.isfinite(g['all_off_Wres'])) and np.all(np.isfinite(g['all_off_Hres']))


def test_initialize_free_mats_restatement_reproduces_the_reference(g):
    c = S.CLASS_CFG
    src, srcw, filt, Cx = S.class_dicts()
    for a, k in ((src, 'cls_src'), (srcw, 'cls_srcw'), (filt, 'cls_filt'), (Cx, 'cls_Cx')):
        np.testing.assert_array_equal(a, g[k])

    class Shape(object):     # what class_ref reads of the model
        iter_num = 2
        nbFreqsSigRepr, nbFramesSigRepr = c['F'], c['T']
        nbComps, nbNMFResComps = c['nbComps'], c['nbNMFResComps']
        nbFilterComps, nbFilterWeigs = c['nbFilterComps'], c['nbFilterWeigs']
        rank = c['spatial_rank']
    o = class_ref(Shape, c['seed'], src, srcw, filt)
    S.initialize_free_mats(o, Cx, src, c['nbComps'], niter=c['niter'])
    assert np.random.rand() == float(g['cls_rand'])
    assert o.spec_comps[0]['factor'][0]['FB'] is o.spec_comps[1]['factor'][0]['FB']
    for j in range(c['nbComps']):
        assert rel(o.spat_comps[j]['params'], g['cls_params_%d' % j]) < BOUND, j
        for i, f in o.spec_comps[j]['factor'].items():
            for p in PARTS:
                ref = g['cls_%s_%d_%d' % (p, j, i)]
                assert f[p].shape == ref.shape
                assert rel(f[p], ref) < BOUND, (j, i, p, rel(f[p], ref))


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "sfnmf.npz")) < 1 << 20
