"""pyfasst_amd.demixTF on the GPU against the reference's numbers
(tests/golden/demix_<case>.npz) and the live restatement (tests/demix_ref.py).

Bounds.  Features: the PCA test's own bounds
(sigtools_ref.BOUND): the confidence is a function of the two eigenvalues and
is held to BOUND['lambdaM'] relative to its maximum against the fixtures;
against the live restatement, which keeps the eigenvalues, it is held at each
point to the PCA test's bounds on them (relative to max lambdaM) propagated
through 20 log10(lambdaM / max(lambdam, eps)), which is what a small lambdam,
the difference tra - delta of two nearly equal numbers, amplifies; theta and phi are
functions of the large eigenvector (e0, e1), |e0| = cos(theta), |e1| =
sin(theta), whose components the PCA test holds to BOUND['vM']: theta is held
to that bound, and phi = angle(e1 / e0), compared on the circle, to the bound
propagated through the quotient, BOUND['vM'] (1 / |e0| + 1 / |e1|); thetaVar is
held to the host formula of the device's own confidence at 1e-12 and, against
the reference's plane, to the confidence bound times the formula's condition
number: var = p / ((nb - 1)(p - 1)^2) with p = 10^(c / 20) has
|d ln var / dc| = (ln 10 / 20)(p + 1) / (p - 1).
Masks: exact, which tests/test_demix_ref_golden.py makes legitimate for the
fixtures (no decision margin below 1e-9); for the live cases the margins come
from the restatement run here and points below 1e-9 may differ, capped at
0.1 % of the plane.
"""
import os
import warnings

import numpy as np
import pytest
import scipy.io.wavfile as wf

import demix_ref as D
import sigtools_ref as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIGHT = 1e-9
CAP = 1e-3


@pytest.fixture(scope="module")
def dm():
    import pyfasst_amd.demixTF as m
    return m


def write_wav(path, samples, fs=D.FS):
    wf.write(str(path), fs, samples)
    return str(path)


def to_int16(x):
    return np.round(x / np.abs(x).max() * 30000).astype(np.int16)


def circ(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def phi_error(phi, ref_phi, ref_theta):
    """max |phi - ref| on the circle over 1 / |e0| + 1 / |e1|."""
    phi, ref_phi, ref_theta = (np.atleast_1d(a) for a in (phi, ref_phi, ref_theta))
    with np.errstate(all='ignore'):
        w = 1 / np.cos(ref_theta) + 1 / np.sin(ref_theta)
    well = ~np.isnan(ref_phi) & np.isfinite(w)
    return float(np.max(circ(phi, ref_phi)[well] / w[well])) if well.any() else 0.


def conf_allowed(ref):
    """Per point, the PCA test's bounds on the eigenvalues (relative to max
    lambdaM) propagated through 20 log10(lambdaM / max(lambdam, eps))."""
    top = np.max(ref['lbd0'])
    with np.errstate(all='ignore'):
        return 20 / np.log(10) * (S.BOUND['lambdaM'] * top / ref['lbd0'] +
                                  S.BOUND['lambdam'] * top / np.maximum(ref['lbd1'], D.eps))


def check_features(got, ref, neighbors):
    conf, theta, phi, var = (got[k] for k in ('confidence', 'thetaAll', 'phiAll', 'thetaVarAll'))
    for v in (0.0, D.eps):
        assert np.array_equal(conf == v, ref['confidence'] == v), v
    for v in (0.0, np.inf):
        assert np.array_equal(var == v, ref['thetaVarAll'] == v), v
    for k in ('thetaAll', 'phiAll'):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    if 'lbd0' in ref:
        allowed = conf_allowed(ref)
        live = (ref['confidence'] != 0) & (ref['confidence'] != D.eps) & np.isfinite(allowed)
        ratio = np.abs(conf - ref['confidence'])[live] / allowed[live]
        e_conf = S.BOUND['lambdaM'] * (np.max(ratio) if live.any() else 0.)
    else:
        e_conf = np.max(np.abs(conf - ref['confidence'])) / np.max(np.abs(ref['confidence']))
    ok = ~np.isnan(ref['thetaAll'])
    e_theta = np.max(np.abs(theta - ref['thetaAll'])[ok]) if ok.any() else 0.
    e_phi = phi_error(phi, ref['phiAll'], ref['thetaAll'])
    # the kernel's variance formula on its own confidence
    host = D.RefDEMIX(np.zeros((4, 2)), 1, neighbors=neighbors).estim_var_theta(conf)
    fin = np.isfinite(host) & (host > 0)
    e_var = np.max(np.abs(var[fin] - host[fin]) / host[fin]) if fin.any() else 0.
    # ... and against the reference's plane, through the condition number
    rv, rc = ref['thetaVarAll'], ref['confidence']
    pts = np.isfinite(rv) & (rv > 0) & (rc > D.eps)
    if 'lbd0' in ref:
        dconf = conf_allowed(ref)
        pts &= np.isfinite(dconf)
    else:
        dconf = np.full(rc.shape, S.BOUND['lambdaM'] * np.max(np.abs(rc)))
    with np.errstate(all='ignore'):
        p = 10 ** (rc / 20.)
        kappa = np.log(10) / 20 * (p + 1) / (p - 1)
    pts &= np.isfinite(kappa)
    with np.errstate(all='ignore'):
        dvar = np.abs(var - rv)
    e_var_ref = (np.max((dvar[pts] / rv[pts]) / (kappa * dconf)[pts]) if pts.any() else 0.)
    print("features", dict(conf=e_conf, theta=e_theta, phi=e_phi, var=e_var,
                           var_vs_ref_over_allowed=e_var_ref))
    assert e_conf < S.BOUND['lambdaM']
    assert e_theta < S.BOUND['vM']
    assert e_phi < S.BOUND['vM']
    assert e_var < 1e-12
    assert e_var_ref < 1


def run_gpu(dm, wav, refine=True, **kw):
    d = dm.DEMIX(wav, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d.comp_clusters()
    out = dict(confidence=d.confidence, thetaAll=d.thetaAll, phiAll=d.phiAll,
               thetaVarAll=d.thetaVarAll)
    cc = d.clusterCentroids
    L = out['confidence'].shape[1]
    out['round_index'] = np.array([c.index_freq * L + c.index_time for c in cc])
    for k in ('theta', 'phi', 'confidence', 'delta', 'zoom'):
        out['round_' + k] = np.array([getattr(c, k) for c in cc], dtype=float)
    out['round_size'] = np.array(d._sizes)
    # the counts the delta pass returned, round by round
    out['dev_size'] = np.array(d.round_sizes)
    out['dev_remaining'] = np.array(d.round_remaining)
    masks = np.array(d.clusters)
    out['masks'] = masks
    out['subTFpointSet'] = d.subTFpointSet
    if refine and d.nsources is not None:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            d.refine_clusters()
        out['ref_theta'] = np.array([c.theta for c in d.clusterCentroids])
        out['ref_delta'] = np.array([c.delta for c in d.clusterCentroids])
        out['ref_confidence'] = np.array([c.confidence for c in d.clusterCentroids])
        out['ref_index'] = np.array([c.index_freq * L + c.index_time for c in d.clusterCentroids])
        out['ref_sizes'] = np.array([m.sum() for m in d.clusters])
        out['steering'] = d.steeringVectorsFromCentroids()
    return d, out


def remaining_counts(masks):
    left = np.ones(masks.shape[1:], dtype=bool)
    rem = []
    for m in masks:
        left &= ~m
        rem.append(int(left.sum()))
    return np.array(rem)


# ------------------------------------------------------------------ fixtures
_gpu = {}


def fixture_run(dm, tmp_path_factory, name):
    if name not in _gpu:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        wav = write_wav(tmp_path_factory.mktemp(name) / "x.wav", g['wav'], int(g['fs']))
        _gpu[name] = (g,) + run_gpu(dm, wav, **D.CASES[name])
    return _gpu[name]


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_features_vs_reference(dm, tmp_path_factory, name):
    g, d, out = fixture_run(dm, tmp_path_factory, name)
    check_features(out, g, D.CASES[name]['neighbors'])


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_comp_clusters_vs_reference(dm, tmp_path_factory, name):
    g, d, out = fixture_run(dm, tmp_path_factory, name)
    assert np.array_equal(out['round_index'], g['round_index'])
    want = np.unpackbits(g['clusters'], axis=1)[:, :out['masks'][0].size].astype(bool)
    got = out['masks'].reshape(len(out['masks']), -1)
    if not np.array_equal(got, want):
        # the fixture's margins are >= 1e-9 (tests/test_demix_ref_golden.py)
        rnd, pt = np.argwhere(got != want)[0]
        ref, _ = D.run_case(D.read_scaled(g['wav']), int(g['fs']), **D.CASES[name])
        pytest.fail("%s: round %d point %d differs, margin %g" %
                    (name, rnd, pt, ref.point_margin.flat[pt]))
    assert np.array_equal(out['round_size'], g['round_size'])
    assert np.array_equal(remaining_counts(out['masks']), g['round_remaining'])
    assert np.array_equal(out['dev_size'], g['round_size'])
    assert np.array_equal(out['dev_remaining'], g['round_remaining'])
    assert int(out['subTFpointSet'].sum()) == int(g['round_remaining'][-1])
    assert np.array_equal(out['round_delta'], g['round_delta'], equal_nan=True)
    assert np.array_equal(out['round_zoom'], g['round_zoom'])
    scale = np.max(np.abs(g['confidence']))
    assert np.max(np.abs(out['round_confidence'] - g['round_confidence'])) / scale < S.BOUND['lambdaM']
    assert np.max(np.abs(out['round_theta'] - g['round_theta'])) < S.BOUND['vM']
    assert phi_error(out['round_phi'], g['round_phi'], g['round_theta']) < S.BOUND['vM']


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_refine_and_steering_vs_reference(dm, tmp_path_factory, name):
    g, d, out = fixture_run(dm, tmp_path_factory, name)
    assert np.array_equal(out['ref_index'], g['ref_index'])
    assert np.array_equal(out['ref_delta'], g['ref_delta'])
    assert np.array_equal(out['ref_sizes'], g['ref_sizes'])
    for k in ('ref_theta', 'ref_confidence'):
        assert np.max(np.abs(out[k] - g[k]) / np.abs(g[k])) < TIGHT, k
    assert out['steering'].shape == g['steering'].shape
    assert np.max(np.abs(out['steering'] - g['steering'])) < TIGHT


# --------------------------------------------------------------- live shapes
# name: (samples, seed, silent second channel, constructor arguments) -> F, L
LIVE = {
    'f65_l67': (69 * 64, 3, False, dict(nsources=3, wlen=128, hopsize=64, neighbors=5)),
    'f129_l300': (317 * 64, 4, False, dict(nsources=3, wlen=256, hopsize=64, neighbors=20)),
    'f2049_l70': (69 * 2048, 5, False, dict(nsources=3, wlen=4096, hopsize=2048, neighbors=2)),
    'silent': (69 * 64, 6, True, dict(nsources=2, wlen=128, hopsize=64, neighbors=5)),
    'maxclusters': (69 * 64, 7, False, dict(nsources=None, maxclusters=3, wlen=128, hopsize=64,
                                            neighbors=5)),
}
SHAPES = {'f65_l67': (65, 67), 'f129_l300': (129, 300), 'f2049_l70': (2049, 70),
          'silent': (65, 67), 'maxclusters': (65, 67)}


@pytest.mark.parametrize("name", sorted(LIVE))
def test_live_vs_restatement(dm, tmp_path, name):
    n, seed, silent, kw = LIVE[name]
    samples = to_int16(D.live_mixture(n, seed, silent_second=silent))
    if silent:
        assert not samples[:, 1].any()
    wav = write_wav(tmp_path / "x.wav", samples)
    d, out = run_gpu(dm, wav, **kw)
    ref, want = D.run_case(D.read_scaled(samples), D.FS, pca='direct', **kw)
    assert out['confidence'].shape == SHAPES[name]
    check_features(out, want, kw['neighbors'])
    npts = out['confidence'].size
    low = ref.point_margin.reshape(-1) < D.MARGIN_MIN
    assert low.sum() <= CAP * npts, "bad case: the restatement's own margins exceed the cap"
    for k in ('theta', 'delta', 'threshold', 'argmax'):
        print(name, k, ref.margins[k])
    assert np.array_equal(out['round_index'], want['round_index'])
    wmask = np.unpackbits(want['clusters'], axis=1)[:, :npts].astype(bool)
    gmask = out['masks'].reshape(len(out['masks']), -1)
    assert gmask.shape == wmask.shape
    diff = (gmask != wmask).any(axis=0)
    assert not (diff & ~low).any(), "a point with margin %g differs" % (
        ref.point_margin.reshape(-1)[diff & ~low].min())
    assert diff.sum() <= CAP * npts
    if not diff.any():
        assert np.array_equal(out['round_size'], want['round_size'])
        assert np.array_equal(remaining_counts(out['masks']), want['round_remaining'])
        assert np.array_equal(out['dev_size'], want['round_size'])
        assert np.array_equal(out['dev_remaining'], want['round_remaining'])
    assert np.array_equal(out['round_delta'], want['round_delta'], equal_nan=True)
    if name == 'maxclusters':
        assert len(out['round_index']) == 3 and out['subTFpointSet'].sum() > 0
    if not diff.any():
        assert np.array_equal(out['subTFpointSet'], want['subTFpointSet'])
    if 'ref_theta' in want:
        assert np.array_equal(out['ref_index'], want['ref_index'])
        assert np.array_equal(out['ref_delta'], want['ref_delta'])
        if not diff.any():
            assert np.array_equal(out['ref_sizes'], want['ref_sizes'])
            # a centroid that the refinement did not re-estimate keeps its
            # point's confidence, with that point's feature bound
            own = conf_allowed(want).reshape(-1)[want['ref_index']]
            own = np.where(np.isfinite(own), own, 0.)
            assert np.all(np.abs(out['ref_theta'] - want['ref_theta']) <=
                          TIGHT * np.abs(want['ref_theta']))
            assert np.all(np.abs(out['ref_confidence'] - want['ref_confidence']) <=
                          TIGHT * np.abs(want['ref_confidence']) + own)
            assert np.max(np.abs(out['steering'] - want['steering'])) < TIGHT


# ------------------------------------------------- determinism and residency
def test_determinism(dm, tmp_path):
    n, seed, silent, kw = LIVE['f129_l300']
    wav = write_wav(tmp_path / "x.wav", to_int16(D.live_mixture(n, seed)))
    _, a = run_gpu(dm, wav, **kw)
    _, b = run_gpu(dm, wav, **kw)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_residency(dm, tmp_path):
    """comp_clusters() and refine_clusters() launch kernels and download none
    of the feature planes or masks; reading an attribute does.  What the
    counter sees is demix_get_plane / demix_get_mask: the two STFT planes,
    which the package's STFT returns as host arrays (`sig_repr`) and
    demix_features uploads before the feature stage, are outside it."""
    n, seed, silent, kw = LIVE['f65_l67']
    wav = write_wav(tmp_path / "x.wav", to_int16(D.live_mixture(n, seed)))
    d = dm.DEMIX(wav, **kw)
    k0, t0 = dm.launch_count(), dm.transfer_count()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d.comp_clusters()
        k1 = dm.launch_count()
        d.refine_clusters()
    assert k1 >= k0 + 3 + 4 * len(d.round_ms) and dm.launch_count() > k1
    assert dm.transfer_count() == t0
    assert d.features_ms > 0 and all(ms > 0 for ms in d.round_ms)
    conf = d.confidence
    assert dm.transfer_count() == t0 + 1
    assert len(d.clusters) == len(d.clusterCentroids)
    assert dm.transfer_count() == t0 + 1 + len(d.clusterCentroids)
    # assigning uploads: the next step sees it
    conf[:] = 0
    conf[7, 11] = 50.
    d.confidence = conf
    d.init_subpts_set()
    p = d.get_max_confidence_point()
    assert (p.index_freq, p.index_time, p.confidence) == (7, 11, 50.)
    sub = d.subTFpointSet
    assert sub.all()
    sub[7, 11] = False
    d.subTFpointSet = sub
    p = d.get_max_confidence_point()
    assert (p.index_freq, p.index_time) == (0, 0)


def test_candidate_mask_and_host_forms(dm, tmp_path):
    """getTFpointsNearTheta_OneScale returns the device pass's candidate mask;
    compute_temporal / identify_deltaT on it agree with the loop's own round."""
    n, seed, silent, kw = LIVE['f65_l67']
    wav = write_wav(tmp_path / "x.wav", to_int16(D.live_mixture(n, seed)))
    d = dm.DEMIX(wav, **kw)
    d.comp_sig_repr()
    d.comp_pcafeatures()
    d.comp_parameters()
    d.init_subpts_set()
    c = d.get_max_confidence_point()
    t0 = dm.transfer_count()
    mask, bound = d.getTFpointsNearTheta_OneScale(c)
    assert dm.transfer_count() == t0 + 1
    theta = d.thetaAll
    with np.errstate(all='ignore'):
        host = np.abs(theta - c.theta) < bound
    gap = np.abs(np.abs(theta - c.theta) - bound)
    assert mask.dtype == bool and np.isfinite(bound) and mask[c.index_freq, c.index_time]
    assert np.array_equal(mask[gap > 1e-12], host[gap > 1e-12])
    sums, _ = d._theta_pass(c)
    fun_dev = d._detection_function(sums, 2)
    fun_host = d.compute_temporal(mask, 2)
    assert fun_host.shape == (256,)
    assert np.max(np.abs(fun_dev - fun_host)) <= 1e-12 * np.max(np.abs(fun_host))
    delta = d.identify_deltaT(mask, c)
    d2 = dm.DEMIX(wav, **kw)
    d2.comp_clusters()
    assert np.array_equal(delta if delta is not None else np.nan,
                          d2.clusterCentroids[0].delta, equal_nan=True)


def test_stftold_is_the_hann_stft(dm, tmp_path):
    """'stftold' (a Hann window of wlen, nfft = fsize, hop = hopsize) is, for a
    power-of-two wlen, the 'stft' representation with winFunc=np.hanning."""
    n, seed, silent, kw = LIVE['f65_l67']
    wav = write_wav(tmp_path / "x.wav", to_int16(D.live_mixture(n, seed)))
    _, a = run_gpu(dm, wav, tfrepresentation='stftold', **kw)
    _, b = run_gpu(dm, wav, winFunc=np.hanning, **kw)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert not np.array_equal(a['confidence'], run_gpu(dm, wav, **kw)[1]['confidence'])


def test_module_helpers(dm):
    """decibel, invdb, get_indices_peak, confidenceFromVar and the constants of
    pyfasst_amd.demixTF itself."""
    assert (dm.eps, dm.uVarBound, dm.uDistBound) == (1e-10, 2.33, 2.33)
    assert dm.db is dm.decibel
    seq = np.array([0., 1., 3., 2.5, 1., 0., 0., 2.9])
    assert np.array_equal(np.flatnonzero(dm.get_indices_peak(seq, 2, 0.8)), [2, 3])
    assert np.array_equal(np.flatnonzero(dm.get_indices_peak(seq, 7, 0.5)), [7])
    wrap = np.array([3., 2.9, 0., 0., 0., 2.8])
    assert np.array_equal(np.flatnonzero(dm.get_indices_peak(wrap, 0, 0.8)), [0, 1, 5])
    assert dm.decibel(10.) == 20. and dm.invdb(40.) == 100.
    assert dm.invdb(dm.decibel(3.0)) == pytest.approx(3.0, rel=1e-15)
    assert dm.confidenceFromVar(0.01, 5) == pytest.approx(
        20 * np.log10((0.08 + 1 + np.sqrt(1.16)) / 0.08), rel=1e-15)
    for v in (1e-3, 0.5):
        assert dm.confidenceFromVar(v, 20) == D.confidenceFromVar(v, 20)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_object_usable(dm, tmp_path):
    n, seed, silent, kw = LIVE['f65_l67']
    samples = to_int16(D.live_mixture(n, seed))
    wav = write_wav(tmp_path / "x.wav", samples)
    with pytest.raises(NotImplementedError, match="mqt"):
        dm.DEMIX(wav, tfrepresentation='mqt')
    d = dm.DEMIX(wav, nsources=None, maxclusters=4, wlen=128, hopsize=64, neighbors=5)
    d.comp_clusters()
    with pytest.raises(NotImplementedError, match="nsources"):
        d.refine_clusters()
    with pytest.raises(NotImplementedError, match="spatial_filtering"):
        d.spatial_filtering()
    assert len(d.clusters) == 4 and d.steeringVectorsFromCentroids().shape == (4, 65, 2)
    d.nsources = 2
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d.refine_clusters()
    assert len(d.clusterCentroids) <= 2
    mono = write_wav(tmp_path / "m.wav", samples[:, 0])
    with pytest.raises(ValueError, match="stereo"):
        dm.DEMIX(mono, wlen=128, hopsize=64).comp_clusters()


def test_two_minute_crop(dm, tmp_path):
    """A signal longer than 2 * 60 * fs samples is analysed on its middle
    slice (demixTF.py:406-416)."""
    from pyfasst_amd.tftransforms import tft
    fs, n = 1000, 2 * 60 * 1000 + 4001
    rs = np.random.RandomState(0)
    samples = to_int16(rs.randn(n, 2))
    wav = write_wav(tmp_path / "x.wav", samples, fs)
    d = dm.DEMIX(wav, wlen=128, hopsize=64, neighbors=5)
    d.comp_sig_repr()
    start = (n - 120 * fs) // 2
    x = D.read_scaled(samples)[start:start + 120 * fs]
    t = tft.STFT(linFTLen=128, atomHopFactor=0.5, winFunc=tft.sqrt_blackmanharris, fs=fs)
    t.computeTransform(x[:, 1])
    assert d.sig_repr[1].shape == t.transfo.shape == (65, 120 * fs // 64 + 2)
    assert np.array_equal(d.sig_repr[1][:, 100], t.transfo[:, 100])
    assert not hasattr(d.audioObject, '_data')


# ----------------------------------------------------------------- isolation
def test_initializeConvParams_still_refuses_demix(tmp_path):
    """The boundary of this change: FASST.initializeConvParams('demix') keeps
    its refusal (the assertion of tests/test_gpu_surface.py) and leaves the
    model as it was."""
    import pyfasst_amd.audioModel as am
    g = np.load(os.path.join(GOLDEN, "convinit_rand.npz"))
    wav = write_wav(tmp_path / "convinit.wav", g['wav'], int(g['fs']))
    np.random.seed(0)
    m = am.MultiChanNMFConv(wav, nbComps=3, nbNMFComps=4, spatial_rank=[1, 2, 1],
                            iter_num=3, wlen=256, hopsize=64)
    before = {j: (c['mix_type'], c['params'].copy()) for j, c in m.spat_comps.items()}
    with pytest.raises(NotImplementedError):
        m.initializeConvParams()
    for j, c in m.spat_comps.items():
        assert c['mix_type'] == before[j][0] == 'inst'
        assert np.array_equal(c['params'], before[j][1])


def test_fasst_estimation_launches_nothing_from_demix(dm):
    """A FASST estimation (the smoke model: one GEM run and the Wiener
    images) in this process launches nothing from fasst_demix.hip."""
    import __graft_entry__ as ge
    k0 = dm.launch_count()
    ge.smoke()
    assert dm.launch_count() == k0
