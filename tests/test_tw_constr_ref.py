"""Discrete-state time weights, CPU side: the NumPy restatement
(tests/tw_constr_ref.py) reproduces the reference's hmm_* fixtures
(tests/golden/make_golden_hmm.py), and the class surface of MultiChanHMM.

The restatement is held to what tests/test_oracle_golden.py asks of the EM
fixtures: equality."""
import inspect
import warnings

import numpy as np
import pytest

from helpers import load
from tw_constr_ref import HMM_CASES, MARGIN_MIN, oracle_from_fixture


@pytest.mark.parametrize("case", sorted(HMM_CASES))
def test_restatement_reproduces_the_reference(case):
    g = load(case)
    assert float(g['margin']) >= MARGIN_MIN
    m = oracle_from_fixture(g, case)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ll = m.estim_param_a_post_model()
    states = g['states']                       # [iter, comp, T]
    assert len(m.state_seqs) == states.shape[0]
    for i, seqs in enumerate(m.state_seqs):
        for k in sorted(seqs):
            np.testing.assert_array_equal(seqs[k], states[i, k])
    # every frame has exactly one active state
    assert m.margin >= MARGIN_MIN
    np.testing.assert_array_equal(ll, g['logliks'])
    for j in range(len(m.spat_comps)):
        np.testing.assert_array_equal(np.array(m.spat_comps[j]['params']),
                                      g['final_params_%d' % j])
    for k in sorted(m.spec_comps):
        fac = m.spec_comps[k]['factor'][0]
        for part in ('FB', 'FW', 'TW', 'TW_all', 'TW_DP_params'):
            np.testing.assert_array_equal(fac[part], g['final_%s_%d' % (part, k)])
        assert np.all(np.sum(fac['TW'] != 0, axis=0) == 1)


def test_restatement_gmm_hmm_raise_after_the_update():
    """'HMM' / 'GMM': the reference updates the model, then its
    renormalisation raises (audioModel.py:2015,2038-2040)."""
    g = load("hmm_shmm")
    for kind in ('HMM', 'GMM'):
        m = oracle_from_fixture(g, "hmm_shmm")
        for comp in m.spec_comps.values():
            comp['factor'][0]['TW_constr'] = kind
            del comp['factor'][0]['TW_DP_params']   # makeItSHMM's: first-use default instead
        before = m.spec_comps[0]['factor'][0]['FB'].copy()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with pytest.raises(NotImplementedError, match="not done yet"):
                m.estim_param_a_post_model()
        assert not np.array_equal(before, m.spec_comps[0]['factor'][0]['FB'])


def test_multichanhmm_surface():
    """MultiChanHMM, makeItHMM and makeItSHMM with the reference's signatures
    (audioModel.py:2510-2549), also through the `pyfasst` import name."""
    import pyfasst.audioModel as alias
    import pyfasst_amd.audioModel as am
    assert alias.MultiChanHMM is am.MultiChanHMM
    assert issubclass(am.MultiChanHMM, am.MultiChanNMFConv)
    sig = inspect.signature(am.MultiChanHMM.__init__)
    assert list(sig.parameters) == ['self', 'audio', 'nbComps', 'nbNMFComps', 'spatial_rank',
                                    'kwargs']
    assert [sig.parameters[n].default for n in ('nbComps', 'nbNMFComps', 'spatial_rank')] == \
        [3, 4, 2]
    for meth in ('makeItHMM', 'makeItSHMM'):
        assert list(inspect.signature(getattr(am.MultiChanHMM, meth)).parameters) == ['self']

    class Stub(am.MultiChanHMM):   # the two methods only touch spec_comps
        def __init__(self):
            self.spec_comps = {0: {'factor': {0: {'TW': np.ones((4, 7))}}}}
    s = Stub()
    s.makeItSHMM()
    fac = s.spec_comps[0]['factor'][0]
    P = 9 * np.eye(4) + 1.
    np.testing.assert_array_equal(fac['TW_DP_params'], P / np.vstack(P.sum(axis=1)))
    assert (fac['TW_constr'], fac['TW_DP_frdm_prior']) == ('SHMM', 'fixed')
    s.makeItHMM()
    assert (fac['TW_constr'], fac['TW_DP_frdm_prior']) == ('HMM', 'free')
