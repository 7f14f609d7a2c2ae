"""The restatement (tests/sf_ref.py RefFASSTsf) against the REFERENCE class's
own run on a dictionary wider than 128 columns, tests/golden/sf_wide.npz
(tests/golden/make_golden_sf_wide.py): this makes RefFASSTsf the live oracle
of tests/test_gpu_sf_wide.py.  CPU only.

Bound: equality, as tests/test_sf_ref_golden.py holds sf_inst to."""
import os

import numpy as np

from helpers import GOLDEN, load
import sf_wide_ref as W


def test_oracle_reproduces_the_reference_wide():
    g = load('sf_wide')
    o, X = W.fixture_oracle(g)
    np.testing.assert_array_equal(o.noise['ann_PSD_lim'][0], g['psd_lim0'])
    np.testing.assert_array_equal(o.noise['ann_PSD_lim'][1], g['psd_lim1'])
    f0, f1 = o.spec_comps[0]['factor'][0], o.spec_comps[1]['factor'][0]
    assert f0['FB'] is f1['FB'] and f0['FW'] is f1['FW'] and f0['TW'] is not f1['TW']
    assert o.spec_comps[0]['factor'][1]['FB'] is o.spec_comps[1]['factor'][1]['FB']
    ll = o.estim_param_a_post_model()
    W.compare_fixture(o, g, ll, None, None)
    np.testing.assert_array_equal(o.noise['PSD'], g['final_psd'])
    S = o.separated_images(X)
    np.testing.assert_array_equal(np.abs(S)[..., ::int(g['absS_step'])], g['absS'])


def test_fixture_is_what_the_generator_describes():
    g = load('sf_wide')
    assert os.path.getsize(os.path.join(GOLDEN, "sf_wide.npz")) < 1 << 20
    FB, FW = g['init_FB_0_0'], g['init_FW_0_0']
    Kb = FB.shape[1]
    assert FB.shape[0] == 129 and Kb > 128 and Kb % 16 and FW.shape == (Kb, Kb)
    assert len(g['logliks']) == 3
    for part in ('FB', 'FW'):       # one array in both source / filter components
        assert str(g['alias_%s_1_0' % part]) == '0_0'
    assert str(g['alias_FB_1_1']) == '0_1' and str(g['alias_TW_1_0']) == '1_0'
    assert 'init_FB_1_0' not in g and 'init_TW_1_0' in g
    assert tuple(str(p) for p in g['priors_0_0']) == ('fixed', 'fixed', 'free')
    # the constructor's renormalisation has already been over the weights:
    # diagonal, and no longer the identity the class creates them as
    assert not np.count_nonzero(FW - np.diag(np.diag(FW)))
    assert not np.array_equal(FW, np.eye(Kb))
    FWf = g['final_FW_0_0']
    assert not np.count_nonzero(FWf - np.diag(np.diag(FWf)))
