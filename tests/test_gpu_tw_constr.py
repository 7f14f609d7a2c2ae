"""Discrete-state time weights (TW_constr 'GSMM' / 'SHMM', MultiChanHMM) on
the GPU against the reference's hmm_* fixtures and the live restatement
(tests/tw_constr_ref.py).

Tolerances are the ones tests/test_gpu_parity.py applies: TIGHT for the WAV
fixtures (em_conv), 1e-10 on the logliks / 1e-8 on the parameters for the
STFT-domain synthetic models (test_em_stft_domain_vs_oracle).  State sequences
are compared for equality at every iteration; each comparison first requires
the restatement's own decision margin to be >= MARGIN_MIN."""
import copy
import os
import warnings

import numpy as np
import pytest
import scipy.io.wavfile as wf

import fasst_ref as R
from helpers import load, rel
from test_gpu_parity import TIGHT, _c3_like, _split_spec, _time_blobs
from tw_constr_ref import (HMM_CASES, MARGIN_MIN, RefFASSTConstr, constrain, make_shmm,
                           oracle_from_fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The GMM/GSMM/HMM")]

# the bounds tests/test_gpu_parity.py writes as literals in its STFT-domain
# comparisons with the oracle (test_em_stft_domain_vs_oracle: `rel(ll, llo) <
# 1e-10`, `rel(...) < 1e-8` on params / FB / TW; the same pair in
# test_em_multi_components_vs_oracle and test_time_blobs_vs_oracle), named here
# only to be used in several tests; no bound of this file's own
LL_TOL, PARAM_TOL = 1e-10, 1e-8


def _am():
    import pyfasst_amd.audioModel as am
    return am


def _as_constr(o):
    o.__class__ = RefFASSTConstr
    o.margin = np.inf
    o.state_seqs = []
    return o


def _pair(F, T, J, K, rank, iters, conv=True, seed=0):
    """Product and restatement on identical inputs (_c3_like; 'inst': the
    same construction without makeItConvolutive)."""
    if conv:
        m, o, X = _c3_like(F, T, J, K, rank, iters, seed)
        return m, _as_constr(o)
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    X = synthetic.stereo_mixture(F, T, J=J, K_true=4, rank=rank, seed=seed)
    np.random.seed(1)
    m = _am().MultiChanNMFInst_FASST(SpectralAudio(X=X), nbComps=J, nbNMFComps=K,
                                     spatial_rank=rank, iter_num=iters, wlen=2 * (F - 1),
                                     hopsize=(F - 1) // 2)
    o = RefFASSTConstr(iter_num=iters)
    o.set_transform([X[0], X[1]])
    np.random.seed(1)
    R.init_nmf_inst(o, J, K, rank)
    return m, o


def _run_stepwise(m):
    """estim_param_a_post_model's loop (audioModel.py:330-382) one
    GEM_iteration at a time, keeping each iteration's decoded sequences."""
    lls, states = [], []
    for i in range(m.iter_num):
        m.noise['PSD'] = m._annealed_psd(i)
        lls.append(m.GEM_iteration())
        states.append({k: v.copy() for k, v in m.tw_state_seq.items()})
    return np.array(lls), states


def _oracle_run(o):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ll = o.estim_param_a_post_model()
    assert o.margin >= MARGIN_MIN, "decision margin %.3g of the restatement" % o.margin
    return ll


def _compare(m, o, keys, ll, llo, ll_tol, tol):
    assert rel(ll, llo) < ll_tol
    for j in range(len(m.spat_comps)):
        assert rel(m.spat_comps[j]['params'], o.spat_comps[j]['params']) < tol
    for k in sorted(m.spec_comps):
        fm, fo = m.spec_comps[k]['factor'][0], o.spec_comps[k]['factor'][0]
        parts = ('FB', 'FW', 'TW') + (('TW_all', 'TW_DP_params') if k in keys else ())
        for part in parts:
            assert np.shape(fm[part]) == np.shape(fo[part]), (k, part)
            assert rel(fm[part], fo[part]) < tol, (k, part)
        if k in keys:
            assert np.all(np.sum(fm['TW'] != 0, axis=0) == 1)
        else:
            assert 'TW_all' not in fm


def _product_from_fixture(g, case, tmp_path):
    import json
    ctor = json.loads(str(g['ctor']))
    wav = os.path.join(str(tmp_path), case + ".wav")
    wf.write(wav, int(g['fs']), g['wav'])
    np.random.seed(0)
    m = _am().MultiChanHMM(wav, nbComps=ctor['nbComps'], nbNMFComps=ctor['nbNMFComps'],
                           spatial_rank=ctor['spatial_rank'], **ctor['kw'])
    m.makeItConvolutive()
    HMM_CASES[case](m)
    return m


@pytest.mark.parametrize("case", sorted(HMM_CASES))
def test_fixture_vs_reference(case, tmp_path):
    g = load(case)
    assert float(g['margin']) >= MARGIN_MIN
    states = g['states']
    m = _product_from_fixture(g, case, tmp_path)
    ll, seqs = _run_stepwise(m)
    for i in range(states.shape[0]):
        for k in sorted(m.spec_comps):
            np.testing.assert_array_equal(seqs[i][k], states[i, k])
    # the batched run (all iterations enqueued at once)
    m2 = _product_from_fixture(g, case, tmp_path)
    ll2 = m2.estim_param_a_post_model()
    for mod, l in ((m, ll), (m2, ll2)):
        assert rel(l, g['logliks']) < TIGHT
        for j in range(len(mod.spat_comps)):
            assert rel(mod.spat_comps[j]['params'], g['final_params_%d' % j]) < TIGHT
        for k in sorted(mod.spec_comps):
            fac = mod.spec_comps[k]['factor'][0]
            for part in ('FB', 'FW', 'TW', 'TW_all', 'TW_DP_params'):
                assert rel(fac[part], g['final_%s_%d' % (part, k)]) < TIGHT, (k, part)
            np.testing.assert_array_equal(mod.tw_state_seq[k], states[-1, k])


@pytest.mark.parametrize("F,T,J,K,rank,iters,kind,free,only,conv", [
    (33, 40, 2, 4, 1, 3, 'SHMM', False, None, True),
    (33, 40, 2, 4, 1, 3, 'GSMM', True, None, True),
    (65, 77, 2, 5, 2, 3, 'SHMM', True, None, True),    # ragged T, K no power of two, rank 2
    (65, 77, 2, 5, 2, 3, 'GSMM', False, None, True),
    (33, 40, 2, 70, 1, 2, 'SHMM', True, None, True),   # K spans two wavefronts in the decode
    (33, 40, 2, 70, 1, 2, 'GSMM', True, None, True),
    (33, 40, 3, 4, 1, 2, 'SHMM', False, [1], True),    # only source 1 constrained
    (33, 40, 2, 4, 1, 3, 'SHMM', True, None, False),   # 'inst' mixing
])
def test_synthetic_vs_restatement(F, T, J, K, rank, iters, kind, free, only, conv):
    m, o = _pair(F, T, J, K, rank, iters, conv)
    for mod in (m, o):
        constrain(mod, kind, only, dp_free=free)
    keys = sorted(m.spec_comps) if only is None else only
    llo = _oracle_run(o)
    ll, seqs = _run_stepwise(m)
    for i in range(iters):
        assert sorted(seqs[i]) == sorted(o.state_seqs[i]) == keys
        for k in keys:
            np.testing.assert_array_equal(seqs[i][k], o.state_seqs[i][k])
    _compare(m, o, keys, ll, llo, LL_TOL, PARAM_TOL)


@pytest.mark.parametrize("kind,free,other", [
    ('SHMM', True, 'split'),      # source 0 owns two spectral components
    ('GSMM', False, 'split'),
    ('SHMM', False, 'blobs'),     # source 0 has free time blobs
    ('GSMM', True, 'blobs'),
])
def test_constrained_next_to_multi_path_sources(kind, free, other):
    """A constrained source in a model whose other spatial component takes
    the sequential multi-component update (several spectral components, or
    time blobs): there the first preparation kernel turns the E-step's plane
    into hat_W in place before the discrete-state step reads it."""
    iters = 3
    m, o = _pair(33, 40, 2, 4, 1, iters)
    for mod in (m, o):
        if other == 'split':
            _split_spec(mod, {0: [2, 2], 1: [4]})   # keys: 0, 2 on source 0; 1 on source 1
            key = 1
        else:
            _time_blobs(mod, {0: (3, 'free', 'free')})
            key = 1
        assert mod.spec_comps[key]['spat_comp_ind'] == 1
        constrain(mod, kind, [key], dp_free=free)
    llo = _oracle_run(o)
    ll, seqs = _run_stepwise(m)
    for i in range(iters):
        assert sorted(seqs[i]) == sorted(o.state_seqs[i]) == [key]
        np.testing.assert_array_equal(seqs[i][key], o.state_seqs[i][key])
    _compare(m, o, [key], ll, llo, LL_TOL, PARAM_TOL)
    if other == 'blobs':
        assert rel(m.spec_comps[0]['factor'][0]['TB'], o.spec_comps[0]['factor'][0]['TB']) \
            < PARAM_TOL
    # the batched run and the step method take the same path
    m2, o2 = _pair(33, 40, 2, 4, 1, iters)
    for mod in (m2, o2):
        if other == 'split':
            _split_spec(mod, {0: [2, 2], 1: [4]})
        else:
            _time_blobs(mod, {0: (3, 'free', 'free')})
        constrain(mod, kind, [key], dp_free=free)
    ll2 = m2.estim_param_a_post_model()
    np.testing.assert_array_equal(m2.tw_state_seq[key], o.state_seqs[-1][key])
    _compare(m2, o, [key], ll2, llo, LL_TOL, PARAM_TOL)
    hat_W = np.array([o2.comp_spat_comp_power(j) for j in range(2)])
    hat_W *= 0.5 + np.random.RandomState(9).rand(*hat_W.shape)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o2.update_spectral_components(hat_W.copy())
    assert o2.margin >= MARGIN_MIN
    m3, _ = _pair(33, 40, 2, 4, 1, iters)
    if other == 'split':
        _split_spec(m3, {0: [2, 2], 1: [4]})
    else:
        _time_blobs(m3, {0: (3, 'free', 'free')})
    constrain(m3, kind, [key], dp_free=free)
    m3.update_spectral_components(hat_W.copy())
    np.testing.assert_array_equal(m3.tw_state_seq[key], o2.state_seqs[0][key])
    for part in ('FB', 'FW', 'TW', 'TW_all', 'TW_DP_params'):
        assert rel(m3.spec_comps[key]['factor'][0][part],
                   o2.spec_comps[key]['factor'][0][part]) < PARAM_TOL, part


def test_more_bins_than_the_lds_tile_holds_is_refused():
    """The discrete-state step keeps 4 frames of hat_W and a basis column in
    LDS, every bin of each: above F = 4096 a constraint is refused, with the
    model as it was."""
    from pyfasst_amd.audioObject import SpectralAudio
    rs = np.random.RandomState(0)
    F, T = 4113, 6
    X = rs.randn(2, F, T) + 1j * rs.randn(2, F, T)
    np.random.seed(1)
    m = _am().MultiChanNMFConv(SpectralAudio(X=X), nbComps=2, nbNMFComps=2, spatial_rank=1,
                               iter_num=1, wlen=2 * (F - 1), hopsize=(F - 1) // 2)
    m.makeItConvolutive()
    constrain(m, 'SHMM')
    before = _snapshot(m)
    with pytest.raises(NotImplementedError, match="4096"):
        m.estim_param_a_post_model()
    _same(before, _snapshot(m))
    constrain(m, 'NMF')                      # the same model runs without it
    assert np.all(np.isfinite(m.estim_param_a_post_model()))


def test_makeitshmm_batched_vs_restatement():
    """MultiChanHMM.makeItSHMM through estim_param_a_post_model's batch."""
    m0, o = _pair(33, 40, 2, 4, 1, 3)
    from pyfasst_amd.audioObject import SpectralAudio
    np.random.seed(1)
    m = _am().MultiChanHMM(SpectralAudio(X=m0.audioObject.X), nbComps=2, nbNMFComps=4,
                           spatial_rank=1, iter_num=3, wlen=64, hopsize=16)
    m.makeItConvolutive()
    m.makeItSHMM()
    make_shmm(o)
    llo = _oracle_run(o)
    ll = m.estim_param_a_post_model()
    for k in sorted(m.spec_comps):
        np.testing.assert_array_equal(m.tw_state_seq[k], o.state_seqs[-1][k])
    _compare(m, o, sorted(m.spec_comps), ll, llo, LL_TOL, PARAM_TOL)


@pytest.mark.parametrize("kind", ['GSMM', 'SHMM'])
def test_ties_go_to_the_lowest_index(kind):
    """State 3 an exact copy of state 1 (same FB.FW column, same TW_all row):
    neither decoder may ever select it."""
    m, _ = _pair(33, 40, 2, 4, 1, 3)
    for k in sorted(m.spec_comps):
        fac = m.spec_comps[k]['factor'][0]
        fac['FB'][:, 3] = fac['FB'][:, 1]
        fac['TW'][3] = fac['TW'][1]
        fac['FB_frdm_prior'] = 'fixed'   # the two columns stay bit-identical
    constrain(m, kind)
    _, seqs = _run_stepwise(m)
    picked = set()
    for s in seqs:
        for k, v in s.items():
            assert not np.any(v == 3)
            picked |= set(v.tolist())
    assert 1 in picked          # the tie did occur and went to the lower index
    for k in sorted(m.spec_comps):
        fac = m.spec_comps[k]['factor'][0]
        np.testing.assert_array_equal(fac['TW_all'][3], fac['TW_all'][1])


@pytest.mark.parametrize("kind", ['GSMM', 'SHMM'])
def test_run_to_run_determinism(kind):
    out = []
    for _ in range(2):
        m, _o = _pair(65, 77, 2, 5, 2, 3)
        constrain(m, kind, dp_free=True)
        ll = m.estim_param_a_post_model()
        out.append((ll, m))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    a, b = out[0][1], out[1][1]
    for j in range(2):
        np.testing.assert_array_equal(a.spat_comps[j]['params'], b.spat_comps[j]['params'])
    for k in sorted(a.spec_comps):
        np.testing.assert_array_equal(a.tw_state_seq[k], b.tw_state_seq[k])
        for part in ('FB', 'FW', 'TW', 'TW_all', 'TW_DP_params'):
            np.testing.assert_array_equal(a.spec_comps[k]['factor'][0][part],
                                          b.spec_comps[k]['factor'][0][part])


@pytest.mark.parametrize("kind", ['GSMM', 'SHMM'])
def test_step_method_vs_restatement(kind):
    """update_spectral_components(hat_W) alone, no renormalisation."""
    m, o = _pair(33, 40, 2, 4, 1, 1)
    for mod in (m, o):
        constrain(mod, kind, dp_free=True)
    rs = np.random.RandomState(7)
    hat_W = np.array([o.comp_spat_comp_power(j) for j in range(2)])
    hat_W *= 0.5 + rs.rand(*hat_W.shape)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.update_spectral_components(hat_W.copy())
    assert o.margin >= MARGIN_MIN
    m.update_spectral_components(hat_W.copy())
    for k in sorted(m.spec_comps):
        np.testing.assert_array_equal(m.tw_state_seq[k], o.state_seqs[0][k])
        fm, fo = m.spec_comps[k]['factor'][0], o.spec_comps[k]['factor'][0]
        for part in ('FB', 'FW', 'TW', 'TW_all', 'TW_DP_params'):
            assert rel(fm[part], fo[part]) < PARAM_TOL, (k, part)


def _snapshot(m):
    return copy.deepcopy((m.spat_comps, m.spec_comps))


def _same(a, b):
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            if 'factor' in x[k]:
                fx, fy = x[k]['factor'][0], y[k]['factor'][0]
                assert sorted(fx) == sorted(fy)
                for p in fx:
                    np.testing.assert_array_equal(np.asarray(fx[p]), np.asarray(fy[p]))
            else:
                np.testing.assert_array_equal(x[k]['params'], y[k]['params'])


@pytest.mark.parametrize("kind", ['GMM', 'HMM'])
def test_gmm_hmm_refused_before_anything_moves(kind):
    m, _ = _pair(33, 40, 2, 4, 1, 1)
    constrain(m, kind, dp_free=True)
    before = _snapshot(m)
    with pytest.raises(NotImplementedError, match="not done yet"):
        m.estim_param_a_post_model()
    _same(before, _snapshot(m))
    m2 = _am().MultiChanHMM
    assert callable(m2.makeItHMM)


def test_time_blobs_with_a_constraint_raise_attributeerror():
    m, _ = _pair(33, 40, 2, 4, 1, 1)
    constrain(m, 'SHMM')
    fac = m.spec_comps[0]['factor'][0]
    rs = np.random.RandomState(3)
    fac['TB'] = np.abs(rs.randn(3, 40)) + 0.2
    fac['TW'] = np.abs(rs.randn(4, 3)) + 0.2
    with pytest.raises(AttributeError, match="time blobs"):
        m.estim_param_a_post_model()


def test_lambda_corr_with_a_constraint_is_refused():
    m, _ = _pair(33, 40, 2, 4, 1, 1)
    constrain(m, 'GSMM')
    m.lambdaCorr = 0.5
    with pytest.raises(NotImplementedError, match="lambdaCorr"):
        m.estim_param_a_post_model()
    # and straight through the C ABI
    m.lambdaCorr = 0.
    m._upload()
    m._engine.set_corr(0.5, [0, 1], [0, 0])
    with pytest.raises(NotImplementedError, match="lambdaCorr"):
        m._engine.run(np.ones((1, m._engine.F)), 1.0)


def test_shared_spatial_component_is_refused():
    m, _ = _pair(33, 40, 2, 4, 1, 1)
    m.spec_comps[2] = copy.deepcopy(m.spec_comps[1])
    constrain(m, 'SHMM', [1])
    with pytest.raises(NotImplementedError, match="only one"):
        m.estim_param_a_post_model()


def test_unconstrained_path_is_untouched():
    """An em_conv-shaped NMF-only model gives bit-equal results whether or
    not the constraint setter was ever called on another context."""
    def nmf_run():
        m, _ = _pair(65, 77, 3, 8, 2, 3)
        ll = m.estim_param_a_post_model()
        return ll, _snapshot(m)
    ll_a, snap_a = nmf_run()
    c, _ = _pair(65, 77, 3, 8, 2, 2)
    constrain(c, 'SHMM', dp_free=True)
    c.estim_param_a_post_model()
    ll_b, snap_b = nmf_run()
    np.testing.assert_array_equal(ll_a, ll_b)
    _same(snap_a, snap_b)
    assert 'TW_all' not in snap_b[1][0]['factor'][0]
