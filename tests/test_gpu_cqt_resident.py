"""MinQT / CQT models whose observation and separation stay on the GPU:
fasst_set_audio_cqt and the batched inverse behind separated_waveforms() /
spatial_filter_waveforms() (include/fasst_cqt.h), against the route they
replace on the same model: per-channel tft.computeTransform() + Engine.set_stft
for the front end, separated_images() / spatial_filter_images() inverted image
by image through tft.invertTransform() for the back end.

Tolerances.  The front end runs the kernels of cqt_forward in the same
operation order, so Cx is compared with np.array_equal.  The batched inverse
runs the kernels of cqt_inverse on the images the Wiener kernel left in HBM
(the download / upload of the old route is exact); the spatial filter forms
each image value with the 2x2 apply of spatial_filter_images() as it is
loaded, which can differ by contraction rounding carried through a linear
transform.  Both are held to the project's fused-against-images bound, 1e-13
of max|ref| (FUSED_TOL of test_gpu_spatial_filter.py).  WAV samples: 1 LSB
(the int16 truncation flips on such a difference).

Shapes: fs 8000, wlen 256, hop 64, 12 bins per octave; 'mqt' has 3 octaves
(FFTLen 512, one atom per frame), 'cqt' 5 octaves with 5 atoms per frame, so
nframes differs from octave to octave; 4001 samples (odd: no multiple of any
octave's hop) with different channels."""
import os

import numpy as np
import pytest
import scipy.io.wavfile as wf

pytestmark = pytest.mark.gpu

FUSED_TOL = 1e-13
FS, N = 8000, 4001
TRANSF = {
    'mqt': dict(transf='mqt', tffmin=100, tfbpo=12),
    'cqt': dict(transf='cqt', tffmin=100, tffmax=3000, tfbpo=12),
}
FIX, FREE = 'fixed', 'free'


def _am():
    import pyfasst_amd.audioModel as am
    return am


def write_wav(tmp_path, name="mix"):
    """Two different channels: tones with a different level and delay each,
    plus independent noise."""
    rs = np.random.RandomState(5)
    t = np.arange(N) / float(FS)
    a = np.sin(2 * np.pi * 440 * t) + 0.6 * np.sin(2 * np.pi * 1230 * t + 0.3)
    b = np.sin(2 * np.pi * 2100 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))
    x = np.stack([0.9 * a + 0.3 * b, 0.2 * np.roll(a, 3) + 0.8 * np.roll(b, 5)], axis=1)
    x += 0.05 * rs.randn(N, 2)
    x = np.int16(x / np.abs(x).max() * 20000)
    assert not np.array_equal(x[:, 0], x[:, 1])
    fn = os.path.join(str(tmp_path), name + ".wav")
    wf.write(fn, FS, x)
    return fn


def model(tmp_path, transf, J, K=3, conv=True, rank=2):
    np.random.seed(0)
    cls = _am().MultiChanNMFConv if conv else _am().MultiChanNMFInst_FASST
    m = cls(write_wav(tmp_path), nbComps=J, nbNMFComps=K, spatial_rank=[rank] * J, iter_num=2,
            wlen=256, hopsize=64, **TRANSF[transf])
    if conv:
        m.makeItConvolutive()
        # per-bin mixing filters that differ from component to component
        rs = np.random.RandomState(11)
        for j in range(J):
            p = np.asarray(m.spat_comps[j]['params'])
            m.spat_comps[j]['params'] = p + 0.3 * (rs.randn(*p.shape) + 1j * rs.randn(*p.shape))
    assert int(m.tft.octaveNr) >= 3
    return m


def invert_images(m, S):
    """The route the device call replaces: one tft.invertTransform() per image."""
    ref = np.empty(S.shape[:2] + (int(m.tft.datalen_init),))
    for n in range(S.shape[0]):
        for c in range(2):
            m.tft.transfo = S[n, c]
            ref[n, c] = m.tft.invertTransform()
            del m.tft.transfo
    return ref


def err(Y, ref):
    return float(np.max(np.abs(Y - ref)) / np.max(np.abs(ref)))


# ---------------------------------------------------------------- 1. front end
@pytest.mark.parametrize("transf", ["mqt", "cqt"])
def test_front_end_bit_equal(transf, tmp_path):
    from pyfasst_amd.engine import Engine
    m = model(tmp_path, transf, J=2)
    assert m.tft.batch_info()[0] == 2          # both channels in one chain
    assert not hasattr(m.tft, '_spCQT')        # no host copy of a transform
    Cx = np.array(m.Cx)
    lim = [np.array(v) for v in m.noise['ann_PSD_lim']]
    kept = {a: getattr(m.tft, a) for a in ('datalen_init', 'maxBlock', 'prefixZeros',
                                           'suffixZeros', 'nframes', 'freqbins')}
    # the parent's route on the same samples
    data = np.asarray(m.audioObject.data, dtype=np.float64)
    X = []
    for c in range(2):
        m.tft.computeTransform(data[:, c])
        X.append(m.tft.transfo)
    X = np.array(X)
    assert np.max(np.abs(X[0] - X[1])) > 0
    e = Engine(X.shape[1], X.shape[2], m.device)
    e.set_stft(X)
    assert np.array_equal(Cx, e.get_cx())
    mix = e.mix_psd()
    assert np.array_equal(lim[0], np.real(mix) / 100.)
    assert np.array_equal(lim[1], np.real(mix) / 10000.)
    assert (m.nbFreqsSigRepr, m.nbFramesSigRepr) == X.shape[1:]
    for a, v in kept.items():
        assert np.array_equal(v, getattr(m.tft, a)), a
    if transf == 'mqt':
        assert m.tft.offsetSTFT == m.tft.cqtkernel.first_center


# ---------------------------------------------------------------- 2. separation
GROUPS = [None, {0: [0, 2], 1: [1]}]


@pytest.mark.parametrize("transf", ["mqt", "cqt"])
@pytest.mark.parametrize("J", [1, 3])
def test_separated_waveforms_vs_inverted_images(transf, J, tmp_path):
    m = model(tmp_path, transf, J)
    for groups in GROUPS if J == 3 else GROUPS[:1]:
        Y = m.separated_waveforms(groups)
        B, launches = m.tft.batch_info()
        S = m.separated_images(groups)
        nsrc = J if groups is None else len(groups)
        assert Y.shape == (nsrc, 2, N) and S.shape[:2] == (nsrc, 2) and B == 2 * nsrc
        ref = invert_images(m, S)
        e = err(Y, ref)
        print(transf, J, groups, "waveforms vs images", e)
        assert e <= FUSED_TOL
        # the chain was launched once for all images
        assert m.tft.batch_info() == (1, launches)


@pytest.mark.parametrize("transf", ["mqt", "cqt"])
@pytest.mark.parametrize("J", [1, 3])
def test_spatial_filter_waveforms_vs_inverted_images(transf, J, tmp_path):
    m = model(tmp_path, transf, J)
    Y = m.spatial_filter_waveforms()
    assert m.tft.batch_info()[0] == 2 * J
    S = m.spatial_filter_images()
    assert Y.shape == (J, 2, N)
    e = err(Y, invert_images(m, S))
    print(transf, J, "spatial filter waveforms vs images", e)
    assert e <= FUSED_TOL


def _factor(rs, F, T, Kb, Kw, pri, eye=False):
    FW = np.eye(Kb) if eye else 0.75 * np.abs(rs.randn(Kb, Kw)) + 0.25
    return {'FB': 0.75 * np.abs(rs.randn(F, Kb)) + 0.25, 'FW': FW,
            'TW': 0.75 * np.abs(rs.randn(FW.shape[1], T)) + 0.25, 'TB': [],
            'FB_frdm_prior': pri[0], 'FW_frdm_prior': pri[1], 'TW_frdm_prior': pri[2],
            'TB_frdm_prior': [], 'TW_constr': 'NMF'}


def test_two_factor_waveforms_vs_inverted_images(tmp_path):
    """Source / filter components on two of three spatial components of a
    MinQT model on a WAV file."""
    m = model(tmp_path, 'mqt', J=3, K=4, conv=False, rank=1)
    F, T = m.nbFreqsSigRepr, m.nbFramesSigRepr
    for k in (0, 1):
        rs = np.random.RandomState(7 + 31 * k)
        m.spec_comps[k]['factor'] = {
            0: _factor(rs, F, T, 13, 13, (FIX, FIX, FREE), True),
            1: _factor(rs, F, T, 6, 3, (FIX, FREE, FREE))}
    assert m._is_sf()
    for groups in ({j: [j] for j in range(3)}, {0: [0, 2], 1: [1]}):
        Y = m.separated_waveforms(groups)
        assert m.tft.batch_info()[0] == 2 * len(groups)
        S = m.separated_images(groups)
        assert Y.shape == (len(groups), 2, N)
        e = err(Y, invert_images(m, S))
        print("two-factor", groups, "waveforms vs images", e)
        assert e <= FUSED_TOL


# ---------------------------------------------------------------- 3. batch hazards
@pytest.mark.parametrize("transf", ["mqt", "cqt"])
def test_silent_source_among_loud_ones_b8(transf, tmp_path):
    m = model(tmp_path, transf, J=4)
    m.spec_comps[0]['factor'][0]['TW'][:] = 0.0
    Y = m.separated_waveforms()
    assert m.tft.batch_info()[0] == 8
    assert np.all(Y[0] == 0.0)
    assert all(np.max(np.abs(Y[n, c])) > 1e-3 for n in range(1, 4) for c in range(2))
    e = err(Y, invert_images(m, m.separated_images()))
    print(transf, "B=8 with a silent source", e)
    assert e <= FUSED_TOL


@pytest.mark.parametrize("transf", ["mqt", "cqt"])
def test_silent_image_beside_a_loud_one_b2(transf, tmp_path):
    """One component whose filters are zero on channel 0: image (0, 0) is
    exactly zero, image (0, 1) is not (B = 2)."""
    m = model(tmp_path, transf, J=1)
    p = np.array(m.spat_comps[0]['params'])    # rank x channel x F
    p[:, 0, :] = 0.0
    m.spat_comps[0]['params'] = p
    Y = m.separated_waveforms()
    assert m.tft.batch_info()[0] == 2
    assert np.all(Y[0, 0] == 0.0)
    assert np.max(np.abs(Y[0, 1])) > 1e-3
    assert err(Y, invert_images(m, m.separated_images())) <= FUSED_TOL


@pytest.mark.parametrize("transf", ["mqt", "cqt"])
@pytest.mark.parametrize("B", [4, 8])
def test_swapping_two_sources_swaps_the_waveforms(transf, B, tmp_path):
    """The source table with sources 0 and 1 exchanged: the images, and so the
    slots of the batch, change places; the waveforms follow bit for bit."""
    J = 3 if B == 4 else 5
    m = model(tmp_path, transf, J, K=2)
    a = {0: [0, J - 1], 1: [1]}
    b = {0: [1], 1: [0, J - 1]}
    for n in range(2, B // 2):
        a[n] = b[n] = [n]
    Ya = m.separated_waveforms(a)
    assert m.tft.batch_info()[0] == B
    Yb = m.separated_waveforms(b)
    assert Ya.shape == Yb.shape == (B // 2, 2, N)
    assert np.array_equal(Ya[0], Yb[1]) and np.array_equal(Ya[1], Yb[0])
    assert np.array_equal(Ya[2:], Yb[2:])
    assert not np.array_equal(Ya[0], Ya[1])


# ---------------------------------------------------------------- 4. it is batched
@pytest.mark.parametrize("transf", ["mqt", "cqt"])
def test_launch_count_does_not_grow_with_the_batch(transf, tmp_path):
    m = model(tmp_path, transf, J=4)
    assert m.tft.batch_info()[0] == 2                  # the front end
    S = m.separated_images()
    m.tft.transfo = S[0, 0]
    m.tft.invertTransform()
    del m.tft.transfo
    one = m.tft.batch_info()
    assert one[0] == 1 and one[1] > 0
    m.separated_waveforms()
    assert m.tft.batch_info() == (8, one[1])
    m.spatial_filter_waveforms()
    assert m.tft.batch_info() == (8, one[1])


# ---------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("transf", ["mqt", "cqt"])
def test_repeatable_and_single_inverse_untouched(transf, tmp_path):
    m = model(tmp_path, transf, J=3)
    S = m.separated_images()

    def single():
        m.tft.transfo = S[1, 1]
        y = m.tft.invertTransform()
        del m.tft.transfo
        return y
    y0 = single()
    Y1 = m.separated_waveforms()
    y1 = single()
    Y2 = m.separated_waveforms()
    assert np.array_equal(Y1, Y2)
    assert np.array_equal(y0, y1)
    Z1 = m.spatial_filter_waveforms()
    assert np.array_equal(y0, single())
    assert np.array_equal(Z1, m.spatial_filter_waveforms())


# ---------------------------------------------------------------- 6. files
def test_wav_files_as_the_old_route(tmp_path):
    m = model(tmp_path, 'mqt', J=2)
    scale = m.audioObject._maxdata
    nfr = m.audioObject.nframes
    groups = {0: [0], 1: [1]}
    ref = invert_images(m, m.separated_images(groups))
    m.separate_comps(dir_results=str(tmp_path), spec_comp_ind=groups, suffix={1: 'acc'})
    names = [os.path.basename(f) for f in m.files['spat_comp']]
    assert names == ["mix_0-2.wav", "mix_1-2_acc.wav"]
    for n, fn in enumerate(m.files['spat_comp']):
        y = wf.read(fn)[1].astype(np.int64)
        old = np.int16(ref[n].T[:nfr, :] * scale).astype(np.int64)
        assert y.shape == old.shape
        d = int(np.max(np.abs(y - old)))
        print("separate_comps", n, "max LSB", d)
        assert d <= 1
    ref = invert_images(m, m.spatial_filter_images())
    m.separate_spatial_filter_comp(dir_results=str(tmp_path), suffix={0: 'lead'})
    names = [os.path.basename(f) for f in m.files['spatial']]
    assert names == ["mix_0-2_spatial_lead.wav", "mix_1-2_spatial.wav"]
    for n, fn in enumerate(m.files['spatial']):
        y = wf.read(fn)[1].astype(np.int64)
        old = np.int16(ref[n].T[:nfr, :] * scale).astype(np.int64)
        assert y.shape == old.shape
        d = int(np.max(np.abs(y - old)))
        print("separate_spatial_filter_comp", n, "max LSB", d)
        assert d <= 1


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_model_alone(tmp_path):
    from pyfasst_amd.tftransforms import minqt
    m = model(tmp_path, 'mqt', J=2)
    Y = m.separated_waveforms()
    Cx = np.array(m._engine.get_cx())
    eng, cqt = m._engine, m.tft._context()
    psd = np.asarray(m.noise['PSD'], dtype=np.float64) * np.ones(m.nbFreqsSigRepr)
    data = np.asarray(m.audioObject.data, dtype=np.float64)
    other = minqt.MinQTransfo(fmin=100, fmax=18000, bins=24, fs=FS, perfRast=1, linFTLen=256,
                              atomHopFactor=0.25, device=m.device)
    calls = [
        lambda: eng.separate_waveforms_cqt(other._context(), psd, N),   # other F
        lambda: eng.separate_waveforms_cqt(cqt, psd, N + 4096),         # other T
        lambda: eng.separate_waveforms_cqt(cqt, psd, 0),
        lambda: eng.separate_waveforms_cqt(cqt, psd, -3),
        lambda: eng.spatial_filter_waveforms_cqt(other._context(), N),
        lambda: eng.spatial_filter_waveforms_cqt(cqt, 0),
        lambda: eng.set_audio_cqt(other._context(), data),
        lambda: eng.set_audio_cqt(cqt, data[:N - 1500]),
        lambda: eng.set_audio_cqt(cqt, data[:0]),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert np.array_equal(Cx, eng.get_cx()), i
    assert np.array_equal(Y, m.separated_waveforms())
