"""Source / filter IS-NMF (tools/nmf.py:161-360) and
multiChanSourceF0Filter.initializeFreeMats (audioModel.py:2878-2908) on the
MI355X, against the reference's runs (tests/golden/sfnmf.npz) and the CPU
restatement (tests/sfnmf_ref.py, which test_sfnmf_ref_golden.py pins to those
runs).  Compute goes through libfasst_hip.so (sfnmf_*, include/fasst_nmf.h).

Bounds (max-normalised, helpers.rel).  The IS-NMF tests' own: 1e-10 against
golden, 1e-9 live (GEMM summation order differs from OpenBLAS).  Per golden
case the bound is scaled by the case's sensitivity over the nmf.npz
yardstick's, rounded up to one digit, where the case is the more sensitive:
the largest relative move of the restatement's outputs under a 1e-15 relative
perturbation of SX, 5 draws, measured on the CPU:
    nmf.npz yardstick 1.40e-15
    free 1.26e-15, all_off 1.38e-15, w_off 1.34e-15, wfilt_off 1.16e-15  -> x1
    h_off 1.48e-15, inits 1.68e-15, hfilt_off 2.36e-15                   -> x2
"""
import ctypes

import numpy as np
import pytest

from helpers import load, rel
import sfnmf_ref as S
from sf_ref import PARTS, class_ref, compare
from test_gpu_parity import TIGHT

pytestmark = pytest.mark.gpu

GOLD_TOL = {'free': 1e-10, 'all_off': 1e-10, 'w_off': 1e-10, 'wfilt_off': 1e-10,
            'h_off': 2e-10, 'inits': 2e-10, 'hfilt_off': 2e-10}
LIVE_TOL = 1e-9
LL_TOL = 1e-10                  # tests/test_gpu_multifactor.py's, with TIGHT


def _nmf():
    import pyfasst_amd.tools.nmf as nmf
    return nmf


def _check(res, ref, tol, what):
    for n, a, b in zip(S.NAMES, res, ref):
        assert a.shape == b.shape, (what, n, a.shape, b.shape)
        r = rel(a, b)
        print(what, n, "%.2e" % r)
        assert r < tol, (what, n, r)


@pytest.fixture(scope="module")
def g():
    return load("sfnmf")


@pytest.mark.parametrize("case", sorted(S.SFNMF_CASES))
def test_sfnmf_golden(g, case):
    inits = {k: g['%s_%s' % (case, k)] for k in ('Winit', 'Hinit', 'WFiltInit', 'HFiltInit')
             if '%s_%s' % (case, k) in g}
    np.random.seed(int(g[case + '_seed']))
    res = _nmf().SFNMF_decomp_init(g[case + '_SX'], **dict(S.case_kwargs(case), **inits))
    assert np.random.rand() == float(g[case + '_rand'])
    _check(res, [g['%s_%s' % (case, n)] for n in S.NAMES], GOLD_TOL[case], case)


def _sx(F, N, seed):
    rs = np.random.RandomState(seed)
    return rs.gamma(0.7, 1.0, size=(F, N)) * np.outer(rs.gamma(2, 1, F), np.ones(N)) + 1e-3


# a single component everywhere; ragged against every tile size; K above 128
# (the source pair on dgemm2); the F0 dictionary's width (ragged M tile of
# dgemm2, odd K: padded leading dimension); a wide filter; and, added to the
# listed shapes, the filter and residual pairs on the dgemm2 path as well
# (every pair takes it from 128 components), with an odd number of frames
LIVE = [(33, 17, 1, 1, 1, 3), (257, 301, 40, 20, 2, 3), (129, 90, 200, 7, 3, 3),
        (257, 64, 1093, 10, 2, 2), (65, 300, 16, 64, 8, 3), (70, 45, 3, 130, 129, 2)]


@pytest.mark.parametrize("F,N,K,Kf,Kr,niter", LIVE)
def test_sfnmf_vs_restatement(F, N, K, Kf, Kr, niter):
    SX = _sx(F, N, F + N)
    kw = dict(nbComps=K, nbFiltComps=Kf, nbResComps=Kr, niter=niter)
    np.random.seed(5)
    res = _nmf().SFNMF_decomp_init(SX, **kw)
    a = np.random.rand()
    np.random.seed(5)
    ref = S.sfnmf_decomp_init(SX, **kw)
    assert a == np.random.rand()
    _check(res, ref, LIVE_TOL, (F, N, K, Kf, Kr))


def test_sfnmf_zero_column_guard():
    """sumW == 0 -> 1.  A supplied Winit with an all-zero column does not
    reach the guard finitely: the reference's initial `W /= W.sum(axis=0)`
    (nmf.py:191-192) makes that column 0 / 0 and every output NaN (checked on
    the restatement below).  An all-zero component of Hinit does: the first W
    update multiplies its column by num = 0, the column sum is 0, the guard
    keeps W and H finite."""
    F, N, K, Kf, Kr = 40, 33, 5, 4, 2
    rs = np.random.RandomState(3)
    SX = rs.gamma(0.7, 1.0, size=(F, N)) + 1e-3
    W0 = rs.rand(F, K) + .1
    W0[:, 2] = 0
    np.random.seed(1)
    with np.errstate(all='ignore'):
        bad = S.sfnmf_decomp_init(SX, K, Kf, 1, Winit=W0, nbResComps=Kr)
    assert not np.all(np.isfinite(bad[0]))
    W0 = rs.rand(F, K) + .1
    H0 = rs.rand(N, K) + .1
    H0[:, 2] = 0
    kw = dict(nbComps=K, nbFiltComps=Kf, nbResComps=Kr, niter=3, Winit=W0, Hinit=H0)
    np.random.seed(1)
    ref = S.sfnmf_decomp_init(SX, **kw)
    assert all(np.all(np.isfinite(a)) for a in ref) and np.all(ref[0][:, 2] == 0)
    np.random.seed(1)
    res = _nmf().SFNMF_decomp_init(SX, **kw)
    assert np.all(res[0][:, 2] == 0) and np.all(res[1][2] == 0)
    _check(res, ref, LIVE_TOL, "zero column")


def test_sfnmf_zero_filter_frames():
    """HFiltInit with two all-zero frames: sumH = 0 multiplies H before the
    guard (nmf.py:316-319), so those frames of H come back zero, and HFilt
    there stays zero."""
    F, N, K, Kf, Kr = 40, 33, 5, 4, 2
    rs = np.random.RandomState(4)
    SX = rs.gamma(0.7, 1.0, size=(F, N)) + 1e-3
    HF = rs.rand(N, Kf) + .1
    HF[[4, 20]] = 0
    kw = dict(nbComps=K, nbFiltComps=Kf, nbResComps=Kr, niter=3, HFiltInit=HF)
    np.random.seed(1)
    ref = S.sfnmf_decomp_init(SX, **kw)
    assert all(np.all(np.isfinite(a)) for a in ref)
    np.random.seed(1)
    res = _nmf().SFNMF_decomp_init(SX, **kw)
    assert all(np.all(np.isfinite(a)) for a in res)
    assert np.all(res[1][:, [4, 20]] == 0) and np.all(res[3][:, [4, 20]] == 0)
    assert np.all(res[1][:, [3, 5]] > 0)
    _check(res, ref, LIVE_TOL, "zero frames")


def test_sfnmf_switches():
    """A factor nothing writes comes back bit-identical to the input.  W and
    WFilt are written only by their own updates; H is also rescaled by the W
    update (column sums) and the HFilt update (frame sums), HFilt by the WFilt
    update, so those are switched off with them."""
    F, N, K, Kf, Kr = 65, 47, 13, 6, 2
    rs = np.random.RandomState(8)
    SX = _sx(F, N, 9)
    init = dict(Winit=rs.rand(F, K) + .1, Hinit=rs.rand(N, K) + .1,
                WFiltInit=rs.rand(F, Kf) + .1, HFiltInit=rs.rand(N, Kf) + .1)
    given = (init['Winit'], init['Hinit'].T, init['WFiltInit'], init['HFiltInit'].T)
    base = dict(nbComps=K, nbFiltComps=Kf, nbResComps=Kr, niter=2, **init)
    on = dict(updateW=True, updateH=True, updateWFilt=True, updateHFilt=True)
    # (switches off, factors that must come back untouched)
    for off, same in ((('updateW',), (0,)), (('updateWFilt',), (2,)),
                      (('updateH', 'updateW', 'updateHFilt'), (0, 1)),
                      (('updateHFilt', 'updateWFilt'), (2, 3)),
                      (('updateW', 'updateH', 'updateWFilt', 'updateHFilt'), (0, 1, 2, 3))):
        sw = dict(on, **{k: False for k in off})
        np.random.seed(2)
        res = _nmf().SFNMF_decomp_init(SX, **dict(base, **sw))
        np.random.seed(2)
        ref = S.sfnmf_decomp_init(SX, **dict(base, **sw))
        for i in range(4):
            if i in same:
                assert np.array_equal(res[i], given[i]), (off, S.NAMES[i])
            else:
                assert not np.array_equal(res[i], given[i]), (off, S.NAMES[i])
        _check(res, ref, LIVE_TOL, off)
    # the residual always moves: with every init supplied its draw comes first
    np.random.seed(2)
    Wres0 = (1 + np.random.randn(F, Kr)) ** 2
    assert res[4].shape == Wres0.shape and not np.array_equal(res[4], Wres0)


def test_sfnmf_is_deterministic():
    F, N, K, Kf, Kr = 129, 90, 200, 7, 3
    SX = _sx(F, N, 1)
    out = []
    for _ in range(2):
        np.random.seed(7)
        out.append(_nmf().SFNMF_decomp_init(SX, nbComps=K, nbFiltComps=Kf, nbResComps=Kr, niter=3))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _class_state(m):
    out = {}
    for j, sc in m.spat_comps.items():
        out['params_%d' % j] = np.array(sc['params'])
    for k, comp in m.spec_comps.items():
        for i, f in comp['factor'].items():
            for p in PARTS:
                out['%s_%d_%d' % (p, k, i)] = np.array(f[p])
    return out


def test_initialize_free_mats_golden(g):
    """The product's method on the object of the reference's fixture (built
    without its constructor, tests/sfnmf_ref.py bare_model)."""
    import pyfasst_amd.audioModel as am
    c = S.CLASS_CFG
    src, srcw, filt, Cx = S.class_dicts()
    m = S.bare_model(am.multiChanSourceF0Filter, src, srcw, filt, Cx)
    m._initialize_structures(seed=c['seed'])
    tw = [m.spec_comps[j]['factor'][0]['TW'] for j in range(c['nbComps'] - 1)]
    m.initializeFreeMats(niter=c['niter'])
    assert np.random.rand() == float(g['cls_rand'])
    assert m.spec_comps[0]['factor'][0]['FB'] is m.spec_comps[1]['factor'][0]['FB']
    for j in range(c['nbComps'] - 1):       # written in place
        assert m.spec_comps[j]['factor'][0]['TW'] is tw[j]
    for k, v in _class_state(m).items():
        assert v.shape == g['cls_' + k].shape
        r = rel(v, g['cls_' + k])
        print(k, "%.2e" % r)
        assert r < 1e-10, (k, r)


def _class_model(F=65, T=40):
    import pyfasst_amd.audioModel as am
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    X = synthetic.stereo_mixture(F, T, J=3, K_true=4, rank=1, seed=2)
    m = am.multiChanSourceF0Filter(SpectralAudio(X=X, samplerate=8000), nbComps=3,
                                   nbFilterComps=6, nbFilterWeigs=[3], minF0=100, maxF0=400,
                                   stepnoteF0=2, iter_num=2, wlen=128, hopsize=64)
    return m, X


def test_initialize_free_mats_class_then_gem():
    """The small class model of test_source_filter_class_runs_and_matches_
    restatement: initializeFreeMats against its restatement, then the GEM
    iterations from that state against RefFASSTsf from the same state."""
    m, X = _class_model()
    dicts = [np.array(a) for a in (m.sourceFreqComps, m.sourceFreqWeights, m.filterFreqComps)]
    m._initialize_structures(seed=3)
    o = class_ref(m, 3, *dicts)
    state = np.random.get_state()        # the NMF draws its H from the stream
    m.initializeFreeMats(niter=3)
    a = np.random.rand()
    np.random.set_state(state)
    S.initialize_free_mats(o, m.Cx, o.spec_comps[0]['factor'][0]['FB'], m.nbComps, niter=3)
    assert a == np.random.rand()
    assert m.spec_comps[0]['factor'][0]['FB'] is m.spec_comps[1]['factor'][0]['FB']
    assert m.spec_comps[0]['factor'][0]['FW'] is m.spec_comps[1]['factor'][0]['FW']
    sm, so = _class_state(m), _class_state(o)
    assert sorted(sm) == sorted(so)
    for k in sm:
        assert sm[k].shape == so[k].shape
        assert rel(sm[k], so[k]) < LIVE_TOL, (k, rel(sm[k], so[k]))
    o.set_transform([X[0], X[1]])
    o.noise['ann_PSD_lim'] = [np.array(v) for v in m.noise['ann_PSD_lim']]
    ll = m.estim_param_a_post_model()
    llo = o.estim_param_a_post_model()
    compare(m, o, ll, llo, LL_TOL, TIGHT)


def test_initialize_free_mats_wide_dictionary():
    """A hand-set 200-column dictionary: the initialisation runs (the NMF
    engine has no K ceiling), the estimation still refuses Kb > 128."""
    m, X = _class_model()
    rs = np.random.RandomState(6)
    F = m.nbFreqsSigRepr
    m.sourceFreqComps = np.hstack([np.abs(rs.randn(F, 199)) + 1e-3, np.ones((F, 1))])
    m.nbSourceComps = 200
    m.sourceFreqWeights = np.eye(200)
    dicts = [np.array(a) for a in (m.sourceFreqComps, m.sourceFreqWeights, m.filterFreqComps)]
    m._initialize_structures(seed=3)
    o = class_ref(m, 3, *dicts)
    state = np.random.get_state()
    m.initializeFreeMats(niter=2)
    np.random.set_state(state)
    S.initialize_free_mats(o, m.Cx, o.spec_comps[0]['factor'][0]['FB'], m.nbComps, niter=2)
    sm, so = _class_state(m), _class_state(o)
    for k in sm:
        assert np.all(np.isfinite(sm[k]))
        assert rel(sm[k], so[k]) < LIVE_TOL, (k, rel(sm[k], so[k]))
    assert m.spec_comps[0]['factor'][0]['TW'].shape == (200, m.nbFramesSigRepr)
    with pytest.raises(NotImplementedError, match="Kb"):
        m.estim_param_a_post_model()


def test_sfnmf_create_refuses_bad_shapes():
    from pyfasst_amd import _lib
    for dims in ((0, 5, 3, 2, 1), (5, -1, 3, 2, 1), (5, 5, 0, 2, 1), (5, 5, 3, 0, 1),
                 (5, 5, 3, 2, -2)):
        p = ctypes.c_void_p()
        assert _lib.lib.sfnmf_create(0, *dims, ctypes.byref(p)) == _lib.FASST_ERR_SHAPE, dims
        assert "sfnmf_create" in _lib.last_error() and not p.value
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("sfnmf_")) == [
        "sfnmf_create", "sfnmf_destroy", "sfnmf_get_params", "sfnmf_run", "sfnmf_set_data",
        "sfnmf_set_params"]
    assert _lib.lib.sfnmf_run(None, 1, 1, 1, 1, 1) == _lib.FASST_ERR_SHAPE
