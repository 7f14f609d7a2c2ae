"""The time-invariant spatial filter (separate_spatial_filter_comp,
audioModel.py:891-1061) and GCC-PHAT (:1316-1324) on the GPU, against the
reference's recorded run (tests/golden/spatial_<case>*.npz) and, at the shapes
where the kernels can go wrong, against its NumPy restatement
(tests/spatial_filter_ref.py, pinned to the same fixtures by
test_spatial_ref_golden.py).

Tolerances.  The gains are R_n inv(R_aa) over their trace: with
cond(R_aa) <= 1e3 (stored in each fixture, asserted for each synthetic draw)
the amplified rounding is about 1e3 x a few ulp ~ 1e-13, held to 1e-12 of
max|WG|.  The images are one 2x2 product further: rel 1e-12.  The fused
waveforms and the iSTFT of the downloaded images share the 2x2 apply and can
differ only by contraction rounding carried through a linear transform:
1e-13 of max|y|.  WAV samples: 1 LSB (int16 truncation flips on 1e-13)."""
import json
import os

import numpy as np
import pytest
import scipy.io.wavfile as wf

import spatial_filter_ref as SR
from helpers import rel

pytestmark = pytest.mark.gpu

GAIN_TOL = 1e-12
IMAGE_TOL = 1e-12
FUSED_TOL = 1e-13
STFT_CASES = ("spatial_conv", "spatial_conv_j1")


def _am():
    import pyfasst_amd.audioModel as am
    return am


_fixtures = {}


def fixture(case):
    if case not in _fixtures:
        _fixtures[case] = SR.load_fixture(case)
    return _fixtures[case]


def fixture_model(case, tmp_path):
    """The model on the fixture's WAV, 'conv', holding the fixture's mixing
    parameters (no EM)."""
    g = fixture(case)
    ctor = json.loads(str(g['ctor']))
    wav = os.path.join(str(tmp_path), "golden_%s.wav" % case)   # the generator's file root
    wf.write(wav, int(g['fs']), g['wav'])
    np.random.seed(0)
    m = _am().MultiChanNMFConv(wav, nbComps=ctor['nbComps'], nbNMFComps=ctor['nbNMFComps'],
                               spatial_rank=ctor['spatial_rank'], **ctor['kw'])
    m.makeItConvolutive()
    for j, p in enumerate(g['params']):
        m.spat_comps[j]['params'] = np.array(p)
    return m, g


def gain_err(WG, ref):
    return float(np.max(np.abs(WG - ref)) / np.max(np.abs(ref)))


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("case", SR.CASES)
def test_gains_and_images_vs_reference(case, tmp_path):
    m, g = fixture_model(case, tmp_path)
    assert float(g['cond_max']) <= 1e3
    WG = m.spatial_filter_gains()
    assert WG.shape == g['WG'].shape
    e = gain_err(WG, g['WG'])
    print(case, "gains", e)
    assert e <= GAIN_TOL
    S = m.spatial_filter_images()
    assert S.shape == g['images'].shape
    e = rel(S, g['images'])
    print(case, "images", e)
    assert e <= IMAGE_TOL


@pytest.mark.parametrize("case", SR.CASES)
def test_wav_files_vs_reference(case, tmp_path):
    m, g = fixture_model(case, tmp_path)
    m.separate_spatial_filter_comp(dir_results=str(tmp_path))
    names = [str(f) for f in g['files']]
    assert [os.path.basename(f) for f in m.files['spatial']] == names
    J = len(names)
    assert names == ["golden_%s_%d-%d_spatial.wav" % (case, n, J) for n in range(J)]
    for n, fn in enumerate(m.files['spatial']):
        assert os.path.dirname(fn) == str(tmp_path)
        y = wf.read(fn)[1].astype(np.int64)
        ref = g['sep_wav_%d' % n].astype(np.int64)
        assert y.shape == ref.shape
        d = int(np.max(np.abs(y - ref)))
        print(case, n, "max LSB", d)
        assert d <= 1
    # the suffix argument: only the listed sources get one
    m.separate_spatial_filter_comp(dir_results=str(tmp_path), suffix={0: 'lead'})
    want = ["golden_%s_%d-%d_spatial%s.wav" % (case, n, J, '_lead' if n == 0 else '')
            for n in range(J)]
    assert [os.path.basename(f) for f in m.files['spatial']] == want
    assert all(os.path.exists(f) for f in m.files['spatial'])


@pytest.mark.parametrize("case", STFT_CASES)
def test_fused_waveforms_vs_inverted_images(case, tmp_path):
    m, g = fixture_model(case, tmp_path)
    Y = m.spatial_filter_waveforms()
    S = m.spatial_filter_images()
    assert Y.shape == (S.shape[0], 2, g['wav'].shape[0])
    ref = np.empty_like(Y)
    for n in range(S.shape[0]):
        for c in range(2):
            m.tft.transfo = S[n, c]
            ref[n, c] = m.tft.invertTransform()
            del m.tft.transfo
    e = float(np.max(np.abs(Y - ref)) / np.max(np.abs(ref)))
    print(case, "fused vs images", e)
    assert e <= FUSED_TOL


@pytest.mark.parametrize("case", STFT_CASES)
def test_gcc_phat_vs_reference(case, tmp_path):
    m, g = fixture_model(case, tmp_path)
    out = m.gcc_phat_tdoa_2d()
    assert out.shape == g['gcc'].shape
    e = rel(out, g['gcc'])
    print(case, "gcc", e)
    assert e <= 1e-12


def test_gcc_phat_other_transform_is_the_numpy_expression(tmp_path):
    m, g = fixture_model("spatial_mqt", tmp_path)
    out = m.gcc_phat_tdoa_2d()
    assert out.shape == g['gcc'].shape
    assert np.array_equal(out, SR.gcc_phat(m.Cx[1], 256), equal_nan=True)
    # the MinQT's exactly-zero points are 0/0, here as in the reference
    assert np.isnan(out).any() and np.isnan(g['gcc']).any()


# ---------------------------------------------------------------- synthetic
def synthetic_model(F, T, ranks, seed, inst=False):
    """STFT-domain model with random complex 'conv' params (cond(R_aa) <= 1e3
    asserted by the callers through SR.cond_max)."""
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    am = _am()
    J = len(ranks)
    X = synthetic.stereo_mixture(F, T, J=min(J, 3), K_true=2, rank=2, seed=seed)
    np.random.seed(seed)
    cls = am.MultiChanNMFInst_FASST if inst else am.MultiChanNMFConv
    m = cls(SpectralAudio(X=X), nbComps=J, nbNMFComps=2, spatial_rank=list(ranks), iter_num=1,
            wlen=2 * (F - 1), hopsize=(F - 1) // 2)
    params = []
    if not inst:
        m.makeItConvolutive()
        rs = np.random.RandomState(1000 + seed)
        for j, r in enumerate(ranks):
            p = rs.randn(r, 2, F) + 1j * rs.randn(r, 2, F)
            m.spat_comps[j]['params'] = p
            params.append(p)
    return m, X, params


def test_known_answer_single_component():
    """J = 1, rank 2: R_aa = R_1, so the gain is I / 2 and the images X / 2."""
    m, X, params = synthetic_model(65, 40, [2], seed=3)
    assert SR.cond_max(params) <= 1e3
    WG = m.spatial_filter_gains()
    want = np.zeros((1, 2, 2, 65), dtype=complex)
    want[0, 0, 0] = want[0, 1, 1] = 0.5
    assert np.max(np.abs(WG - want)) <= 1e-12
    S = m.spatial_filter_images()
    assert rel(S[0], X / 2) <= 1e-12


@pytest.mark.parametrize("F,T,ranks,seed", [
    (65, 77, [1, 2, 3], 0),        # ragged F and T, mixed ranks
    (33, 5, [2] * 16, 1),          # J and the total rank at their ceilings
    (129, 96, [1, 1], 6),         # R_aa full rank only through the mean
])
def test_shapes_vs_restatement(F, T, ranks, seed):
    m, X, params = synthetic_model(F, T, ranks, seed)
    J = len(ranks)
    cond = SR.cond_max(params)
    print("cond", cond)
    assert cond <= 1e3
    ref = SR.gains(params)
    WG = m.spatial_filter_gains()
    assert WG.shape == (J, 2, 2, F)
    e = gain_err(WG, ref)
    print("gains", e)
    assert e <= GAIN_TOL
    S = m.spatial_filter_images()
    assert S.shape == (J, 2, F, T)
    e = rel(S, SR.images(ref, X))
    print("images", e)
    assert e <= IMAGE_TOL
    # sum_n WG_n trace_n = sum_n R_n inv(R_aa) = J I at every bin (the traces
    # from the unnormalised product); each term carries the gain tolerance
    # times its trace, and the sum is divided by J here
    raw = SR.gains(params, normalise=False)
    tr = np.real(raw[:, 0, 0] + raw[:, 1, 1])                  # [J, F]
    tot = np.sum(WG * tr[:, None, None, :], axis=0)            # [2, 2, F]
    eye = J * np.eye(2)[:, :, None]
    e = float(np.max(np.abs(tot - eye))) / J
    print("identity", e)
    assert e <= GAIN_TOL * float(np.max(np.abs(ref))) * float(np.max(np.abs(tr)))
    # the fused waveforms at this shape against the inverted images
    t = m.tft
    Y = m._engine.spatial_filter_waveforms(t.synthWindow, t.window, t.ftlen, t.fthop)
    from pyfasst_amd.tftransforms.stft import istft
    for n in (0, J - 1):
        for c in range(2):
            y = istft(S[n, c], window=t.synthWindow, analysisWindow=t.window, hopsize=t.fthop,
                      nfft=t.ftlen)
            assert y.shape == Y[n, c].shape
            assert np.max(np.abs(Y[n, c] - y)) <= FUSED_TOL * np.max(np.abs(y))


def test_gcc_phat_zero_frame():
    """A frame of zeros is 0/0 = NaN in that frame alone, in the product and
    in the restatement; every other frame agrees."""
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    F, T, t0 = 65, 21, 7
    X = synthetic.stereo_mixture(F, T, J=2, K_true=2, rank=2, seed=5)
    X[:, :, t0] = 0
    np.random.seed(0)
    m = _am().MultiChanNMFConv(SpectralAudio(X=X), nbComps=2, nbNMFComps=2, spatial_rank=2,
                               iter_num=1, wlen=128, hopsize=32)
    out = m.gcc_phat_tdoa_2d()
    ref = SR.gcc_phat(X[0] * np.conj(X[1]), 128)
    assert out.shape == ref.shape == (128, T)
    for a in (out, ref):
        bad = np.nonzero(~np.isfinite(a).all(axis=0))[0]
        assert list(bad) == [t0]
    keep = np.arange(T) != t0
    assert rel(out[:, keep], ref[:, keep]) <= 1e-12


# ---------------------------------------------------------------- refusals
def test_inst_model_raises_as_reference():
    m, X, _ = synthetic_model(33, 20, [1, 2], seed=0, inst=True)
    for call in (m.separate_spatial_filter_comp, m.spatial_filter_gains, m.spatial_filter_images):
        with pytest.raises(NotImplementedError, match="Mixing params not convolutive..."):
            call()
    assert 'spatial' not in getattr(m, 'files', {})


def test_inst_context_refused_at_the_abi():
    from pyfasst_amd import _lib
    m, X, _ = synthetic_model(33, 20, [1, 2], seed=0, inst=True)
    m._upload()
    eng = m._engine
    WG = np.zeros((2, 2, 2, 33), dtype=complex)
    S = np.zeros((2, 2, 33, 20), dtype=complex)
    w = np.hanning(64)
    y = np.zeros((2, 2, 16 * 19 + 32))
    assert _lib.lib.fasst_spatial_filter_gains(eng._h, _lib.dptr(WG)) == _lib.FASST_ERR_UNSUPPORTED
    assert "not convolutive" in _lib.last_error()
    assert _lib.lib.fasst_spatial_filter_images(eng._h, _lib.dptr(S)) == _lib.FASST_ERR_UNSUPPORTED
    assert _lib.lib.fasst_spatial_filter_waveforms(eng._h, _lib.dptr(w), _lib.dptr(w), 64, 64, 16,
                                                   _lib.dptr(y)) == _lib.FASST_ERR_UNSUPPORTED
    assert not WG.any() and not S.any() and not y.any()


def test_mvdr_2d_is_refused():
    m, X, _ = synthetic_model(33, 20, [2], seed=0)
    with pytest.raises(NotImplementedError, match="steering_vectors"):
        m.mvdr_2d(0.3)
