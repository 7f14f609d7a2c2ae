"""Two-factor (source / filter) spectral components on the GPU (fasst_sf.hip)
against the live restatement oracle/fasst_ref.py, whose multi-factor branches
restate the reference's (comp_spat_comp_power, update_spectral_components,
renormalize_parameters).

Bounds: the project's own (tests/test_gpu_parity.py): TIGHT = 1e-9 on the
parameters and |S|, 1e-10 on the logliks.  All models use F = 65."""
import copy

import numpy as np
import pytest

import fasst_ref as R
from helpers import CASES, load, rel, spec_keys
from sf_ref import (SF_FIXTURES, class_ref, compare, compare_fixture, fixture_oracle,
                    fixture_product, pair)
from test_gpu_parity import TIGHT, TIGHT_CASE, _product_model, _spatial_groups

pytestmark = pytest.mark.gpu

LL_TOL = 1e-10
# the fixtures' parameters and |S|: TIGHT, scaled for sf_conv by the
# restatement's own sensitivity to a 1e-15 relative perturbation of Cx
# (tools/relcheck_sf.py: em_conv 2.2e-13, sf_inst 6.6e-15, sf_conv 6.4e-13):
# 1e-9 x 6.4e-13 / 2.2e-13, rounded up to one digit.  The
# logliks keep LL_TOL in every case: nothing further is scaled
FIXTURE_TOL = {'sf_inst': TIGHT, 'sf_conv': 3e-9}


@pytest.mark.parametrize("case", sorted(SF_FIXTURES))
def test_fixture_end_to_end_vs_reference(case, tmp_path):
    """WAV -> GPU STFT -> two-factor GEM iterations -> Wiener images against
    the reference's own run (tests/golden/sf_*.npz)."""
    g = load(case)
    m = fixture_product(g, case, tmp_path)
    for j in range(3):
        assert rel(m.spat_comps[j]['params'], g['init_params_%d' % j]) < 1e-14
        for i, fac in m.spec_comps[j]['factor'].items():
            for p in ('FB', 'FW', 'TW'):
                assert rel(fac[p], g['init_%s_%d_%d' % (p, j, i)]) < 1e-14
    ll = m.estim_param_a_post_model()
    assert rel(m.noise['PSD'], g['final_psd']) < 1e-14
    groups = {j: [j] for j in range(3)}
    S = m.separated_images(groups)
    print(case, "loglik rel err %.3g" % rel(ll, g['logliks']))
    compare_fixture(m, g, ll, S, LL_TOL, FIXTURE_TOL[case])
    # the device-resident separation: the per-image iSTFT of those images
    Y = m.separated_waveforms(groups)
    assert Y.shape[:2] == (3, 2)
    for n in range(3):
        for c in range(2):
            m.tft.transfo = S[n, c]
            np.testing.assert_array_equal(Y[n, c], m.tft.invertTransform())
            del m.tft.transfo
    # separate_spat_comps writes the reference's files
    m.separate_spat_comps(dir_results=str(tmp_path))
    assert len(m.files['spat_comp']) == 3


def test_grouped_sources_and_waveforms_vs_oracle(tmp_path):
    """Two components in one separation source (src_of grouping), a source
    list that leaves nothing out, images against the restatement and
    waveforms against the iSTFT of the images."""
    g = load('sf_conv')
    m = fixture_product(g, 'sf_conv', tmp_path)
    o, X = fixture_oracle(g, 'sf_conv')
    m.iter_num = o.iter_num = 2
    ll, llo = m.estim_param_a_post_model(), o.estim_param_a_post_model()
    print("loglik rel err %.3g" % rel(ll, llo))
    assert rel(ll, llo) < LL_TOL
    groups = {0: [0, 2], 1: [1]}
    S = m.separated_images(groups)
    So = o.separated_images(X, groups)
    assert S.shape == So.shape == (2, 2) + X[0].shape
    assert rel(np.abs(S), np.abs(So)) < FIXTURE_TOL['sf_conv']
    Y = m.separated_waveforms(groups)
    w = np.hanning(128)
    for n in range(2):
        for c in range(2):
            m.tft.transfo = S[n, c]
            np.testing.assert_array_equal(Y[n, c], m.tft.invertTransform())
            del m.tft.transfo
            yo = R.istft(So[n, c], w, w, 64, 128)[:Y.shape[2]]
            assert rel(Y[n, c], yo) < 1e-8
    # a component in no source is left out of the mixture covariance too, as
    # compute_inv_sigma_mix_2d sums the listed sources only
    part = {0: [2], 1: [0]}
    S = m.separated_images(part)
    So = o.separated_images(X, part)
    assert S.shape == So.shape == (2, 2) + X[0].shape
    assert rel(np.abs(S), np.abs(So)) < FIXTURE_TOL['sf_conv']
    assert rel(np.abs(S[1]), np.abs(m.separated_images(groups)[0])) > 1e-3


F = 65
FREE, FIX = 'free', 'fixed'
# source factor: fixed basis, identity weights; filter factor: FB 65 x Kb
# fixed, FW Kb x Kw free (not square), TW free
SRC = (13, 13, (FIX, FIX, FREE), True)


def _filt(Kb=13, Kw=3, pri=(FIX, FREE, FREE)):
    return (Kb, Kw, pri)


def _spec(Kb=13, Kw=3, comps=(0, 1)):
    return {k: [SRC, _filt(Kb, Kw)] for k in comps}


def _run_both(m, o, X=None):
    ll = m.estim_param_a_post_model()
    llo = o.estim_param_a_post_model()
    compare(m, o, ll, llo, LL_TOL, TIGHT)
    if X is not None:
        S = m.separated_images({j: [j] for j in range(len(m.spat_comps))})
        So = o.separated_images(X)
        assert S.shape == So.shape
        assert rel(np.abs(S), np.abs(So)) < TIGHT
    return ll


@pytest.mark.parametrize("T,Kb,Kw,iters", [
    (67, 13, 3, 3),      # nothing a multiple of 4, 16 or 64; FW not square
    (300, 13, 3, 2),     # several frame tiles: the split-K partial sums meet
    (67, 128, 128, 2),   # the ceiling
    (67, 13, 1, 2),      # Kw = 1
])
def test_two_factor_shapes_vs_oracle(T, Kb, Kw, iters):
    """Two source / filter components next to a one-factor free component
    (whose `other` is its own power, note N1), 'inst' rank 1."""
    m, o, X = pair(F, T, 3, 4, 1, iters, False, _spec(Kb, Kw))
    _run_both(m, o, X)


def test_rank_two_on_three_sources_conv():
    m, o, X = pair(F, 67, 3, 4, 2, 2, True, _spec())
    _run_both(m, o, X)


def test_rank_sum_sixteen():
    m, o, X = pair(F, 67, 4, 3, 4, 2, True, _spec(comps=(0, 2)))
    assert sum(np.shape(sc['params'])[0] for sc in m.spat_comps.values()) == 16
    _run_both(m, o)


def test_one_factor_component_with_free_fw():
    """The one-factor component next to the two-factor ones with FB, FW and TW
    all free: `other` = max(V_k, eps) formed once and kept through the three
    steps while V moves (note N1)."""
    def setup(mod):
        fac = mod.spec_comps[2]['factor'][0]
        fac['FW'] = fac['FW'] + 0.3 * np.abs(np.random.RandomState(3).randn(*fac['FW'].shape))
        fac['FW_frdm_prior'] = FREE
    m, o, X = pair(F, 67, 3, 4, 1, 3, False, _spec(), setup=setup)
    _run_both(m, o)


@pytest.mark.parametrize("fb0,fw1,tw1", [(a, b, c) for a in (FREE, FIX) for b in (FREE, FIX)
                                        for c in (FREE, FIX)])
def test_prior_combinations(fb0, fw1, tw1):
    """(FB_0, FW_1, TW_1) free / fixed, TW_0 free; FW_0 and FB_1 follow FB_0
    and FW_1 reversed so that each of the six priors takes both values."""
    fw0 = FIX if fb0 == FREE else FREE
    fb1 = FIX if fw1 == FREE else FREE
    spec = {0: [(13, 5, (fb0, fw0, FREE)), (6, 3, (fb1, fw1, tw1))],
            1: [SRC, _filt()]}
    m, o, X = pair(F, 67, 3, 4, 1, 2, False, spec)
    _run_both(m, o)


def test_omega():
    m, o, X = pair(F, 67, 3, 4, 1, 3, False, _spec(), omega=0.7)
    _run_both(m, o)


def test_fixed_spatial_component():
    def setup(mod):
        mod.spat_comps[1]['frdm_prior'] = FIX
    m, o, X = pair(F, 67, 3, 4, 1, 3, False, _spec(), setup=setup)
    _run_both(m, o)


def test_forced_tw_restart_of_factor_one():
    """TW of factor 1 zeroed: the component's power is 0, its TW stays 0
    through the update, the renormalisation finds sum(TW) < eps and the host
    redraws it from the same stream as the restatement.  The component's
    mixing parameters are fixed."""
    def setup(mod):
        mod.spec_comps[0]['factor'][1]['TW'][...] = 0.0
        # (a free mixing row of a source without power makes the 'inst' solve
        # singular, in the reference as here: hold that component's mixing)
        mod.spat_comps[0]['frdm_prior'] = FIX
    spec = _spec()
    spec[0] = [SRC, _filt(pri=(FIX, FIX, FREE))]
    m, o, X = pair(F, 67, 3, 4, 1, 2, False, spec, setup=setup)
    seen = []
    np.random.seed(11)
    ll = m.estim_param_a_post_model()
    np.random.seed(11)
    llo = o.estim_param_a_post_model(callback=lambda i, mod: seen.extend(mod.restarted))
    # (without power hat_W is 0 too, so factor 0's TW dies with it: two redraws,
    # in key-then-factor order on both sides)
    assert (0, 1) in seen
    compare(m, o, ll, llo, LL_TOL, TIGHT)
    assert np.sum(m.spec_comps[0]['factor'][1]['TW']) > 0


def test_determinism():
    out = []
    for _ in range(2):
        m, o, X = pair(F, 300, 3, 4, 2, 3, True, _spec())
        ll = m.estim_param_a_post_model()
        out.append((ll, [m.spat_comps[j]['params'] for j in range(3)],
                    [m.spec_comps[k]['factor'][i][p] for k in range(3)
                     for i in m.spec_comps[k]['factor'] for p in ('FB', 'FW', 'TW')]))
    assert np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1] + out[0][2], out[1][1] + out[1][2]):
        assert np.array_equal(a, b)


def _three(mod):
    mod.spec_comps[0]['factor'][2] = copy.deepcopy(mod.spec_comps[0]['factor'][1])


def _tb(mod):
    fac = mod.spec_comps[0]['factor'][1]
    fac['TB'] = np.ones((fac['TW'].shape[1], mod.nbFramesSigRepr))
    fac['TW'] = np.ones((fac['TW'].shape[0], fac['TW'].shape[1]))


def _constr(mod):
    mod.spec_comps[0]['factor'][0]['TW_constr'] = 'GSMM'


def _lam(mod):
    mod.lambdaCorr = 0.5


def _several(mod):
    mod.spec_comps[3] = copy.deepcopy(mod.spec_comps[2])


def _rank(mod):
    for sc in mod.spat_comps.values():
        sc['params'] = np.ones((2, 6))


def _kb(mod):
    fac = mod.spec_comps[0]['factor'][0]
    fac['FB'] = np.ones((F, 129))
    fac['FW'] = np.ones((129, 4))
    fac['TW'] = np.ones((4, mod.nbFramesSigRepr))


def _kw(mod):
    fac = mod.spec_comps[0]['factor'][1]
    fac['FW'] = np.ones((fac['FB'].shape[1], 129))
    fac['TW'] = np.ones((129, mod.nbFramesSigRepr))


@pytest.mark.parametrize("break_it,word", [
    (_three, "factors"), (_tb, "TB"), (_constr, "discrete-state"), (_lam, "lambdaCorr"),
    (_several, "spectral components"), (_rank, "rank"), (_kb, "Kb"), (_kw, "Kw")])
def test_refusals_leave_the_model_alone(break_it, word):
    m, o, X = pair(F, 67, 3, 4, 1, 1, False, _spec())
    m.estim_param_a_post_model()       # a device state that a refused call must not move
    before = m._engine.get_factors(0, 1), m._engine.sf_get_spatial(0, (2, 1))
    break_it(m)
    spat, spec = copy.deepcopy(m.spat_comps), copy.deepcopy(m.spec_comps)
    for call in (m.estim_param_a_post_model, m.GEM_iteration, m.renormalize_parameters,
                 m.separated_images):
        with pytest.raises(NotImplementedError, match=word):
            call()

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        return np.array_equal(a, b)
    assert same(m.spat_comps, spat) and same(m.spec_comps, spec)
    after = m._engine.get_factors(0, 1), m._engine.sf_get_spatial(0, (2, 1))
    for a, b in zip(before[0] + (before[1],), after[0] + (after[1],)):
        assert np.array_equal(a, b)


def test_piecewise_steps_refuse_a_two_factor_model():
    m, o, X = pair(F, 67, 3, 4, 1, 1, False, _spec())
    for call in (m.retrieve_subsrc_params, lambda: m.update_spectral_components(None),
                 lambda: m.compute_sigma_comp_2d(0, [0]), m.separate_spatial_filter_comp,
                 m.spatial_filter_gains):
        with pytest.raises(NotImplementedError):
            call()


def test_source_filter_class_runs_and_matches_restatement():
    """multiChanSourceF0Filter on a small transform: its initial structure is
    the reference's (tests/sf_ref.py class_ref, same seed; the structural
    check without a device is in tests/test_sf_ref_golden.py), then it runs."""
    import pyfasst_amd.audioModel as am
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    T = 40
    X = synthetic.stereo_mixture(F, T, J=3, K_true=4, rank=1, seed=2)
    audio = SpectralAudio(X=X, samplerate=8000)
    m = am.multiChanSourceF0Filter(audio, nbComps=3, nbFilterComps=6, nbFilterWeigs=[3],
                                   minF0=100, maxF0=400, stepnoteF0=2, iter_num=2, wlen=128,
                                   hopsize=64)
    assert m.nbSourceComps <= 128 and m.spec_comps[0]['factor'][1]['FW'].shape == (6, 3)
    assert m.spec_comps[0]['factor'][0]['FB'] is m.spec_comps[1]['factor'][0]['FB']
    dicts = [np.array(a) for a in (m.sourceFreqComps, m.sourceFreqWeights, m.filterFreqComps)]
    m._initialize_structures(seed=3)
    o = class_ref(m, 3, *dicts)
    for j in range(3):
        assert m.spat_comps[j]['params'].shape == o.spat_comps[j]['params'].shape
        assert rel(m.spat_comps[j]['params'], o.spat_comps[j]['params']) < 1e-14
        assert sorted(m.spec_comps[j]['factor']) == sorted(o.spec_comps[j]['factor'])
        for i, fo in o.spec_comps[j]['factor'].items():
            fm = m.spec_comps[j]['factor'][i]
            for p in ('FB', 'FW', 'TW'):
                assert fm[p].shape == fo[p].shape
                assert rel(fm[p], fo[p]) < 1e-14, (j, i, p)
            for p in ('FB_frdm_prior', 'FW_frdm_prior', 'TW_frdm_prior', 'TW_constr'):
                assert fm[p] == fo[p]
    o.set_transform([X[0], X[1]])
    o.noise['ann_PSD_lim'] = [np.array(v) for v in m.noise['ann_PSD_lim']]
    ll = m.estim_param_a_post_model()
    llo = o.estim_param_a_post_model()
    compare(m, o, ll, llo, LL_TOL, TIGHT)
    m.sparsity = [5]
    m._initialize_structures(seed=3)
    with pytest.raises(NotImplementedError, match="sparsity"):
        m.estim_param_a_post_model()


@pytest.mark.parametrize("case", ["em_conv", "em_multi"])
def test_single_factor_path_untouched(case, tmp_path):
    """A model without a two-factor component launches no kernel of
    fasst_sf.hip and still meets test_gpu_parity's bounds."""
    g = load(case)
    J = CASES[case][0]
    m = _product_model(case, g, tmp_path)
    m._engine.set_profiling(True)
    ll = m.estim_param_a_post_model()
    times = m._engine.kernel_times()
    m._engine.set_profiling(False)
    assert times and not [k for k in times if k.startswith("k_sf")], times
    assert not m._engine.sf
    tight = TIGHT_CASE.get(case, TIGHT)
    assert rel(ll, g['logliks']) < TIGHT
    for j in range(J):
        assert rel(m.spat_comps[j]['params'], g['final_params_%d' % j]) < tight
    for j in spec_keys(g, J):
        for p in ('FB', 'FW', 'TW'):
            assert rel(m.spec_comps[j]['factor'][0][p], g['final_%s_%d' % (p, j)]) < tight
    S = m.separated_images(_spatial_groups(m))
    assert rel(np.abs(S), np.abs(g['images'])) < tight


def test_two_factor_kernels_are_counted():
    m, o, X = pair(F, 67, 3, 4, 1, 1, False, _spec())
    m._upload()
    m._engine.set_profiling(True)
    m.estim_param_a_post_model()
    times = m._engine.kernel_times()
    assert {"k_sf_gemm", "k_sf_prod", "k_sf_other", "k_sf_ratio", "k_sf_update", "k_sf_hatw",
            "k_sf_energy", "k_sf_renorm"} <= set(times)
