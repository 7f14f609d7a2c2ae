"""The ODGD / WF0 dictionary family of separateLeadFunctions on the GPU
(dict_odgd, include/fasst_dict.h) against the NumPy restatement
(tests/dict_family_ref.py) run live and the reference's own numbers
(tests/golden/dict_family.npz).

Bounds, each relative to the column's largest
magnitude: D.WAVEFORM_BOUND and D.SPECTRUM_BOUND for the complex waveform and
spectrum (ten times the float64 restatement's deviation from its np.longdouble
evaluation over these shapes), D.POWER_BOUND = 1e-10 for |spectrum|^2 columns
(the bound of dict_wf0_stft against tests/golden/wf0.npz).
"""
import ctypes

import numpy as np
import pytest

import dict_family_ref as D
from helpers import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slf():
    from pyfasst_amd.SeparateLeadStereo import separateLeadFunctions
    return separateLeadFunctions


@pytest.fixture(scope="module")
def g():
    return load("dict_family")


def _last_ms():
    from pyfasst_amd import _lib
    ms = ctypes.c_double(-1.0)
    assert _lib.lib.dict_last_ms(ctypes.byref(ms)) == 0
    return ms.value


def _check_pair(got, ref, gold, name):
    odgd, spec = got
    for other in (ref, gold):
        assert odgd.shape == other[0].shape and odgd.dtype == np.complex128
        assert spec.shape == other[1].shape and spec.dtype == np.complex128
        ew, es = D.colrel(odgd, other[0]), D.colrel(spec, other[1])
        print(name, "waveform %.3e  spectrum %.3e" % (ew, es))
        assert ew < D.WAVEFORM_BOUND, (name, ew)
        assert es < D.SPECTRUM_BOUND, (name, es)
    # the windowed signal is real: exactly Hermitian, as np.fft.fft returns it
    n = spec.size
    assert spec[0].imag == 0 and spec[n // 2].imag == 0
    assert np.array_equal(spec[1:], np.conj(spec[:0:-1]))


@pytest.mark.parametrize("name", sorted(D.ODGD_CASES))
def test_odgd_spec(slf, g, name):
    got = D.run_odgd_case(name, slf)
    _check_pair(got, D.run_odgd_case(name), (g['odgd_%s_odgd' % name], g['odgd_%s_spec' % name]),
                name)
    if name == 'zero_partials':
        assert not np.any(got[0]) and not np.any(got[1])


@pytest.mark.parametrize("name", sorted(D.CHIRP_CASES))
def test_odgd_spec_chirped(slf, g, name):
    got = D.run_chirp_case(name, slf)
    _check_pair(got, D.run_chirp_case(name),
                (g['chirp_%s_odgd' % name], g['chirp_%s_spec' % name]), name)


def test_flat_chirp_is_the_plain_comb(slf):
    kw = D.CHIRP_CASES['flat']
    ckw = {k: v for k, v in kw.items() if k not in ('F1', 'F2')}
    oc, sc = slf.generate_ODGD_spec_chirped(**kw)
    for o, s in (slf.generate_ODGD_spec(kw['F1'], **ckw), D.generate_ODGD_spec(kw['F1'], **ckw)):
        assert D.colrel(oc, o) < D.WAVEFORM_BOUND and D.colrel(sc, s) < D.SPECTRUM_BOUND


def test_inharmonicity_is_ignored(slf):
    _, kw = D.ODGD_CASES['inharmo']
    a = slf.generate_ODGD_spec_inharmo(**kw)
    b = slf.generate_ODGD_spec_inharmo(**dict(kw, inharmonicity=0.9))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        slf.generate_ODGD_spec_inharmo(**dict(kw, analysisWindowType=np.ones(kw['lengthOdgd'])))


def _colrel(a, b):
    return float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=0)))


@pytest.mark.parametrize("name", sorted(D.WF0_CASES))
def test_wf0_chirped(slf, g, name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    kw = D.WF0_CASES[name]
    F0Table, WF0 = slf.generate_WF0_chirped(loadWF0=False, **kw)
    F0r, WF0r = D.generate_WF0_chirped(**kw)
    ncol = {'mixed': 21, 'sinebell': 21, 'single': 1}[name]
    assert WF0.shape == (kw['Nfft'], ncol) and WF0.dtype == np.float64
    for F0o, WF0o in ((F0r, WF0r), (g['wf0_%s_F0Table' % name], g['wf0_%s_WF0' % name])):
        np.testing.assert_array_equal(F0Table, F0o)
        assert WF0.shape == WF0o.shape
        e = _colrel(WF0, WF0o)
        print(name, "power %.3e" % e)
        assert e < D.POWER_BOUND
    # all Nfft rows, the upper half the mirror of the lower
    assert np.array_equal(WF0[1:], WF0[:0:-1])
    assert np.all(WF0[kw['Nfft'] // 2 + 1:].max(axis=0) > 0)


def test_wf0_chirped_cache(slf, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    kw = D.WF0_CASES['mixed']
    F0a, WF0a = slf.generate_WF0_chirped(loadWF0=True, **kw)      # nothing stored yet: computes
    files = [p.name for p in tmp_path.iterdir()]
    assert len(files) == 1 and files[0].startswith('wf0gpu_') and files[0].endswith('.npz')
    # a launch in between, so that an unchanged dict_last_ms means "no launch"
    slf.generate_ODGD_spec(220., 8000., lengthOdgd=64, Nfft=64)
    stored = np.load(files[0])
    np.savez(files[0], F0Table=stored['F0Table'], WF0=stored['WF0'] + 1.0)
    ms = _last_ms()
    F0b, WF0b = slf.generate_WF0_chirped(loadWF0=True, **kw)
    assert _last_ms() == ms
    np.testing.assert_array_equal(F0b, F0a)
    np.testing.assert_array_equal(WF0b, WF0a + 1.0)               # the stored arrays
    F0c, WF0c = slf.generate_WF0_chirped(loadWF0=False, **kw)     # recomputed, and stored again
    np.testing.assert_array_equal(WF0c, WF0a)
    np.testing.assert_array_equal(np.load(files[0])['WF0'], WF0a)


def test_wf0_minqt_chirped_is_the_tr_path(slf, tmp_path, monkeypatch):
    """The smallest MinQT geometry of tests/golden/wf0_cqt.npz, 2 F0s x 2:
    bit-equal to generate_WF0_TR_chirped on the same MinQTransfo, and within
    1e-10 of the restatement (the bound of that file's comparison)."""
    from pyfasst_amd.tftransforms import tft
    from pyfasst_amd.tools.utils import sqrt_blackmanharris
    monkeypatch.chdir(tmp_path)
    fs, nft, fmin, fmax, bins = load("wf0_cqt")['cfg_m1'][:5]
    kw = dict(stepNotes=1, Ot=0.5, perF0=2, depthChirpInSemiTone=0.5)
    F0Table, WF0, mqt = slf.generate_WF0_MinQT_chirped(
        200, 210, cqtfmax=fmax, cqtfmin=fmin, cqtbins=int(bins), Fs=fs, Nfft=int(nft),
        lengthWindow=int(nft), loadWF0=False, cqtWinFunc=sqrt_blackmanharris, **kw)
    assert WF0.shape == (int(mqt.freqbins), 4) and F0Table.shape == (2,)
    assert isinstance(mqt, tft.tftransforms['mqt'])
    t = tft.tftransforms['mqt'](fmin=fmin, fmax=fmax, bins=int(bins), fs=fs, linFTLen=int(nft),
                                atomHopFactor=0.25, winFunc=sqrt_blackmanharris, perfRast=1)
    F0t, WF0t, _ = slf.generate_WF0_TR_chirped(t, 200, 210, loadWF0=False, **kw)
    np.testing.assert_array_equal(F0Table, F0t)
    np.testing.assert_array_equal(WF0, WF0t)
    F0r, WF0r, _ = D.generate_WF0_MinQT_chirped(
        200, 210, cqtfmax=fmax, cqtfmin=fmin, cqtbins=int(bins), Fs=fs, Nfft=int(nft),
        lengthWindow=int(nft), cqtWinFunc=sqrt_blackmanharris, **kw)
    np.testing.assert_array_equal(F0Table, F0r)
    assert _colrel(WF0, WF0r) < 1e-10
    # the cache round trip returns the same arrays and a transform
    _, WF0b, mqtb = slf.generate_WF0_MinQT_chirped(
        200, 210, cqtfmax=fmax, cqtfmin=fmin, cqtbins=int(bins), Fs=fs, Nfft=int(nft),
        lengthWindow=int(nft), loadWF0=True, cqtWinFunc=sqrt_blackmanharris, **kw)
    np.testing.assert_array_equal(WF0b, WF0)
    assert isinstance(mqtb, tft.tftransforms['mqt'])


def _raw_dict_odgd(n_cols, nfft):
    from pyfasst_amd import _lib
    L = 8
    f = np.full(max(n_cols, 1), 220.0)
    npart = np.ones(max(n_cols, 1), dtype=np.int32)
    amps = np.ones((max(n_cols, 1), 1), dtype=np.complex128)
    toff = np.zeros(max(n_cols, 1))
    win = np.ones((1, L))
    sel = np.zeros(max(n_cols, 1), dtype=np.int32)
    power = np.zeros((max(nfft, 1), max(n_cols, 1)))
    return _lib.lib.dict_odgd(0, n_cols, _lib.dptr(f), _lib.dptr(f), _lib.iptr(npart), 1,
                              _lib.dptr(amps), _lib.dptr(toff), 8000.0, L, 1, _lib.dptr(win),
                              _lib.iptr(sel), nfft, None, None, _lib.dptr(power))


def test_refusals_leave_the_device_usable(slf):
    from pyfasst_amd import _lib
    ok = D.ODGD_CASES['crop'][1]

    def valid_call_succeeds():
        odgd, spec = slf.generate_ODGD_spec(**ok)
        assert D.colrel(odgd, D.run_odgd_case('crop')[0]) < D.WAVEFORM_BOUND

    for nfft in (100, 16384):
        for call in (lambda: slf.generate_ODGD_spec(220., 8000., lengthOdgd=129, Nfft=nfft),
                     lambda: slf.generate_ODGD_spec_inharmo(220., 8000., lengthOdgd=129, Nfft=nfft),
                     lambda: slf.generate_ODGD_spec_chirped(210., 230., 8000., lengthOdgd=129,
                                                            Nfft=nfft),
                     lambda: slf.generate_WF0_chirped(200, 280, 8000, Nfft=nfft, lengthWindow=200,
                                                      loadWF0=False)):
            with pytest.raises(NotImplementedError, match="8192"):
                call()
        valid_call_succeeds()
    with pytest.raises(ValueError, match="Analysis window not understood"):
        slf.generate_ODGD_spec(220., 8000., lengthOdgd=129, Nfft=64, analysisWindowType='blackman')
    with pytest.raises(ValueError, match="Analysis window not understood"):
        slf.generate_ODGD_spec(220., 8000., lengthOdgd=129, Nfft=64, analysisWindowType='hann')
    slf.generate_ODGD_spec_chirped(210., 230., 8000., lengthOdgd=129, Nfft=64,
                                   analysisWindowType='hann')
    for n_cols, nfft in ((1, 0), (0, 64), (1, 100), (1, 16384)):
        assert _raw_dict_odgd(n_cols, nfft) == _lib.FASST_ERR_SHAPE
        assert "dict_odgd" in _lib.last_error()
    assert _raw_dict_odgd(1, 64) == _lib.FASST_OK
    with pytest.raises(NotImplementedError, match="nsgtMinQT"):
        slf.generate_WF0_NSGTMinQT_chirped(100, 800, 4000, 50)
    valid_call_succeeds()
