"""The spatial package on the GPU (pyfasst_amd.spatial, fasst_spatial.hip)
against the reference's own numbers (tests/golden/spatial_pkg.npz) and, at the
shapes where the kernels can go wrong, against the NumPy restatement
tests/spatial_pkg_ref.py.

Tolerances: S.BOUND[function] = 16 x the float64 / longdouble
difference of the restatement over these very shapes, floor 1e-13, relative
to the largest magnitude of the output; the steering vectors also within
S.STEER_ULP_BOUND of the float64 restatement.
"""
import numpy as np
import pytest

import spatial_pkg_ref as S
from helpers import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return load("spatial_pkg")


@pytest.fixture(scope="module")
def sv():
    import pyfasst_amd.spatial.steering_vectors as sv
    return sv


@pytest.fixture(scope="module")
def dd():
    import pyfasst_amd.spatial.dirdiag as dd
    return dd


def close(got, ref, key):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    e = S.rel_max(got, ref)
    print(key, "rel", e, "bound", S.BOUND[key])
    assert e < S.BOUND[key], (key, e)


def steer_close(got, ref):
    close(got, ref, 'steer_ula')
    e = float(np.max(np.abs(got - ref)))
    print("steering vectors: abs", e, "bound", S.STEER_ULP_BOUND)
    assert e <= S.STEER_ULP_BOUND, e


# ------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("name", sorted(S.ULA_CASES))
def test_steer_ula_fixture(g, sv, name):
    for i, th in enumerate(S.ULA_THETAS):
        a = sv.gen_steer_vec_far_src_uniform_linear_array(S.FREQS33, S.ULA_CASES[name], th,
                                                          S.ULA_DIST)
        steer_close(a, g['ula_%s_%d' % (name, i)])


def test_steer_acous_fixture(g, sv):
    a = sv.gen_steer_vec_acous(S.FREQS33, S.ACOUS_DIST)
    close(a, g['acous'], 'steer_acous')


@pytest.mark.parametrize("name", ['a', 'b', 'zero_bin'])
def test_dir_diag_stereo_fixture(g, sv, name):
    Cx, kw = S.dd_input(name)
    close(sv.cx_tmean(Cx), g['dd_%s_mean' % name], 'cx_tmean')
    d, th = sv.dir_diag_stereo(Cx, **kw)
    assert np.array_equal(th, g['dd_%s_theta' % name])
    close(d, g['dd_%s_diagram' % name], 'capon')
    if name == 'zero_bin':   # the clamped determinant: no error, a zero column
        assert np.all(d[:, 5] == 0)


def test_dir_diag_stereo_singular_fixture(g, sv):
    assert int(g['dd_singular_raised']) == 1
    Cx, kw = S.dd_input('singular')
    with pytest.raises(ValueError, match="Not possible to compute directivity, singular "
                                         "covariance"):
        sv.dir_diag_stereo(Cx, **kw)


@pytest.mark.parametrize("name", sorted(S.MVDR_CASES))
def test_mvdr_fixture(g, dd, name):
    close(dd.make_MVDR_filter_target(*S.mvdr_input(name)), g['mvdr_%s' % name], 'mvdr')


@pytest.mark.parametrize("name", sorted(S.mvdr_bad_inputs()))
def test_mvdr_error_branches(g, dd, name):
    t, i, exc = S.mvdr_bad_inputs()[name]
    with pytest.raises(exc) as e:
        dd.make_MVDR_filter_target(t, i)
    assert str(g['mvdr_bad_%s' % name]) == exc.__name__ + ": " + str(e.value)


def test_generate_steer_vec_thetas_fixture(g, dd):
    fr, th, A = dd.generate_steer_vec_thetas(**S.SVT_KW)
    assert np.array_equal(fr, g['svt_freqs']) and np.array_equal(th, g['svt_thetas'])
    steer_close(A, g['svt_A'])
    fr, th, A2, Raa = dd.generate_steer_vec_thetas(computeRaa=True, **S.SVT_KW)
    assert np.array_equal(A, A2)
    close(Raa, g['svt_Raa'], 'steer_ula')


@pytest.mark.parametrize("n", S.ULAD_SENSORS)
def test_directivity_filter_diagram_fixture(g, dd, n):
    kw = dict(S.ULAD_KW, n_sensors=n)
    th, fr, d = dd.directivity_filter_diagram_ULA(theta_filter=np.pi / 4., **kw)
    assert np.array_equal(th, g['ulad_%d_thetas' % n]) and np.array_equal(fr, g['ulad_%d_freqs' % n])
    close(d, g['ulad_%d_none' % n], 'ula_response')
    d = dd.directivity_filter_diagram_ULA(w_filter=S.ulad_filter(n), doplot='3d', fig=1, **kw)[2]
    close(d, g['ulad_%d_given' % n], 'ula_response')
    with pytest.raises(ValueError) as e:
        dd.directivity_filter_diagram_ULA(w_filter=S.ulad_filter(n)[:, :-1], **kw)
    assert str(e.value) == str(g['ulad_%d_bad' % n])


# ----------------------------------------------------------- live comparisons
@pytest.mark.parametrize("F", S.LIVE_TMEAN_F)
@pytest.mark.parametrize("T", S.LIVE_TMEAN_T)
def test_cx_tmean_live(sv, F, T):
    """T crosses the 64-frame split with a ragged last chunk, F the 256-bin
    tile with a ragged and with whole tiles."""
    Cx = S.cx_of(F, T, 100 + T)
    got = sv.cx_tmean(Cx)
    close(got, S.cx_tmean(Cx), 'cx_tmean')
    assert np.array_equal(got, sv.cx_tmean(Cx))


@pytest.fixture(scope="module")
def cx_b():
    return S.dd_input('b')


@pytest.mark.parametrize("ntheta", S.LIVE_CAPON_NTHETA)
def test_capon_live(sv, cx_b, ntheta):
    Cx, kw = cx_b
    kw = dict(kw, ntheta=ntheta)
    d, th = sv.dir_diag_stereo(Cx, **kw)
    ref, rth = S.dir_diag_stereo(Cx, **kw)
    assert d.shape == (ntheta, 65) and np.array_equal(th, rth)
    close(d, ref, 'capon')
    d2, _ = sv.dir_diag_stereo(Cx, **kw)
    assert np.array_equal(d, d2)


@pytest.mark.parametrize("n", S.LIVE_RESP_SENSORS)
def test_ula_response_live(dd, n):
    for w in (None, S.ulad_filter(n)):
        kw = dict(S.ULAD_KW, n_sensors=n, w_filter=w, theta_filter=np.pi / 4.)
        close(dd.directivity_filter_diagram_ULA(**kw)[2], S.ula_diagram(**kw)[2], 'ula_response')


def test_ula_response_ceiling(dd, sv):
    assert sv.MAX_SENSORS == S.MAX_SENSORS
    n = S.MAX_SENSORS + 1
    with pytest.raises(NotImplementedError, match="sensors"):
        dd.directivity_filter_diagram_ULA(n_sensors=n, w_filter=S.ulad_filter(n), **S.ULAD_KW)


def test_steer_ula_live(sv):
    """One angle, and a batch in one launch, with the phase up to 4 x 120 rad."""
    fr, nch = S.LIVE_STEER_FREQS, S.LIVE_STEER_NCH
    th = S.LIVE_STEER_THETAS
    a = sv.gen_steer_vec_far_src_uniform_linear_array(fr, nch, th[0], S.ULA_DIST)
    steer_close(a, S.steer_ula(fr, nch, th[0], S.ULA_DIST))
    k0 = sv.launch_count()['k_steer_ula']
    batch = sv.steer_ula_batch(fr, nch, th, S.ULA_DIST)
    assert sv.launch_count()['k_steer_ula'] == k0 + 1
    assert batch.shape == (len(th), nch, fr.size) and np.array_equal(batch[0], a)
    steer_close(batch, np.array([S.steer_ula(fr, nch, t, S.ULA_DIST) for t in th]))
    one = sv.gen_steer_vec_far_src_uniform_linear_array(fr[:7], 1, 0.3, S.ULA_DIST)
    assert np.array_equal(one, np.ones((1, 7), complex))


# -------------------------------------------------------------- the model route
def _model(Cx=None, X=None, wlen=128):
    import pyfasst_amd.audioModel as am
    from pyfasst_amd.audioObject import SpectralAudio
    np.random.seed(2)
    m = am.MultiChanNMFConv(SpectralAudio(X=X, Cx=Cx, samplerate=8000), nbComps=2, nbNMFComps=4,
                            spatial_rank=2, iter_num=1, wlen=wlen, hopsize=wlen // 4)
    m.makeItConvolutive()
    return m


def test_resident_route_equals_host_route(sv):
    from pyfasst_amd import synthetic
    F, T, ntheta = 65, 300, 16
    m = _model(X=synthetic.stereo_mixture(F, T, J=2, K_true=3, rank=2, seed=12))
    b0 = sv.transfer_bytes()
    d, th = m.dir_diag_stereo(ntheta=ntheta, distanceInterMic=0.2)
    moved = sv.transfer_bytes() - b0
    # the diagram, the determinants, the frequencies and the sines: no F x T plane
    assert moved == 8 * (ntheta * F + F + F + ntheta) and moved < 8 * F * T
    assert m._Cx is None
    mean = m._engine.cx_tmean()
    assert m._Cx is None and mean.shape == (4, F)
    d1, th1 = sv.dir_diag_stereo(m, nft=128, ntheta=ntheta, samplerate=8000, distanceInterMic=0.2)
    d2, th2 = sv.dir_diag_stereo(m.Cx, nft=128, ntheta=ntheta, samplerate=8000,
                                 distanceInterMic=0.2)
    assert np.array_equal(d, d1) and np.array_equal(d, d2)
    assert np.array_equal(th, th1) and np.array_equal(th, th2)
    assert np.array_equal(mean, sv.cx_tmean(m.Cx))
    close(d, S.dir_diag_stereo(m.Cx, nft=128, ntheta=ntheta, samplerate=8000,
                               distanceInterMic=0.2)[0], 'capon')


def test_a_model_that_asks_for_no_diagram_launches_none(sv):
    from pyfasst_amd import synthetic
    k0 = sv.launch_count()
    m = _model(X=synthetic.stereo_mixture(65, 48, J=2, K_true=3, rank=2, seed=0))
    ll = m.estim_param_a_post_model()
    m.separated_images()
    assert np.all(np.isfinite(ll))
    assert sv.launch_count() == k0
    m.dir_diag_stereo(ntheta=3)
    k1 = sv.launch_count()
    assert k1['k_cx_tmean'] == k0['k_cx_tmean'] + 2
    assert k1['k_capon_diagram'] == k0['k_capon_diagram'] + 1
    assert all(k1[k] == k0[k] for k in k0 if k not in ('k_cx_tmean', 'k_capon_diagram'))
    assert all(v >= 0 for v in sv.last_ms().values())


def test_singular_covariance_leaves_the_model_usable(sv):
    Cx, kw = S.dd_input('singular')
    m = _model(Cx=Cx, wlen=64)
    with pytest.raises(ValueError, match="singular covariance"):
        m.dir_diag_stereo(ntheta=7)
    ll = m.estim_param_a_post_model()
    assert len(ll) == 1 and np.all(np.isfinite(ll))
    Cx, kw = S.dd_input('a')
    m.Cx = Cx
    d, _ = m.dir_diag_stereo(ntheta=7)
    close(d, S.dir_diag_stereo(Cx, **kw)[0], 'capon')


def test_wrong_shapes_raise(sv, dd):
    Cx, kw = S.dd_input('a')
    with pytest.raises(ValueError):   # nft // 2 + 1 bins against the 33 of Cx
        sv.dir_diag_stereo(Cx, nft=128, ntheta=7)
    with pytest.raises(ValueError):
        sv.dir_diag_stereo(Cx[:2], **kw)
    with pytest.raises(NotImplementedError, match="matplotlib"):
        dd.producePicDiagramAgainstDistNSensors()
    with pytest.raises(NotImplementedError, match="matplotlib"):
        dd.produceMVDRplots()


def test_alias_identity():
    import pyfasst.spatial.dirdiag
    import pyfasst.spatial.steering_vectors
    import pyfasst_amd.spatial.dirdiag
    import pyfasst_amd.spatial.steering_vectors
    assert pyfasst.spatial.dirdiag is pyfasst_amd.spatial.dirdiag
    assert pyfasst.spatial.steering_vectors is pyfasst_amd.spatial.steering_vectors
    assert pyfasst_amd.spatial.steering_vectors.soundCelerity == 340.
    assert pyfasst_amd.spatial.dirdiag.sound_celerity == 300.
