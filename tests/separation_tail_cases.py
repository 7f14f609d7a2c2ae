"""The separation tail: every call that turns a fitted model into source images
or waveforms, at shapes small enough to pin bit for bit.

run_cases() calls the library on seeded inputs and returns {name: array};
outputs above 2 KB are kept as SHA-256 digests (host_transfer_cases.digest).
tests/golden/make_golden_separation_tail.py saved its result from the library
as it stood before the calls shared one image producer per model and one iSTFT
sink; test_gpu_separation_tail.py compares against that with tolerance 0 (same
kernels, same launches, same inputs: any difference is a host bug).

STFT geometries (nfft, wlen, hop, T) = (8, 8, 2, 5) and (16, 8, 3, 4): F = 5 / 9
below Fp = 16, T below Tp = 16; the second has a window shorter than the FFT
and a hop that does not divide it.  Every waveform call runs with an analysis
window and with NULL.

Refusals ("refuse_*": the status; the NaN-filled output must stay NaN): per
STFT-waveform call nfft = 12 on an F = 7 model (no power of two), wlen > nfft,
hop = 0, an nfft whose bin count is not F, and for the three context calls a
context holding only set_cx.  "after_refusals_*" is a valid call on the
context that has just refused.
"""
import tempfile

import numpy as np

from host_transfer_cases import ISTFT_SHAPES, _cplx, _keep, _windows, istft_len

K = 3
BAD_F = 7   # nfft = 12: the right bin count, no power of two


def _pos(rng, *shape):
    return 0.5 + rng.random(shape)


def _opt(_lib, a):
    return _lib.dptr(a) if a is not None else None


def _stft_and_psd(F, T, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(_cplx(rng, 2, F, T)), 0.1 + rng.random(F)


# ---- models ------------------------------------------------------------------
def main_engine(F, T, conv=(True, False), stft=True):
    """Two components of rank 2 and K = 3; conv = (True, True) is the
    all-'conv' model of the spatial filter.  stft = False: only set_cx."""
    from pyfasst_amd.engine import Engine
    e = Engine(F, T)
    e.configure([2, 2], [K, K], list(conv))
    rng = np.random.default_rng(1000 + 10 * F + T)
    for j, cv in enumerate(conv):
        e.set_spectral(j, _pos(rng, F, K), _pos(rng, K, K), _pos(rng, K, T), True, True)
        e.set_spatial(j, _cplx(rng, 2, 2, F) if cv else _cplx(rng, 2, 2), True)
    give_observation(e, stft)
    return e


def sf_engine(F, T, stft=True):
    """J = 3, component 0 with two factors."""
    from pyfasst_amd.engine import Engine
    e = Engine(F, T)
    factors = [[(K, 2, 1, 1, 1), (2, 2, 1, 1, 1)], [(K, K, 1, 1, 1)], [(K, K, 1, 1, 1)]]
    e.sf_configure([2, 2, 2], [True, False, False], factors,
                   [[(-1, -1, -1)] * len(f) for f in factors])
    rng = np.random.default_rng(2000 + 10 * F + T)
    for j, facs in enumerate(factors):
        for i, (kb, kw) in enumerate(f[:2] for f in facs):
            e.set_factors(j, i, _pos(rng, F, kb), _pos(rng, kb, kw), _pos(rng, kw, T))
        e.sf_set_spatial(j, _cplx(rng, 2, 2, F) if j == 0 else _cplx(rng, 2, 2), True)
    give_observation(e, stft)
    return e


def give_observation(e, stft=True):
    X, _ = _stft_and_psd(e.F, e.T, 3000 + 10 * e.F + e.T)
    if stft:
        e.set_stft(X)
    else:
        e.set_cx(np.array([X[0] * X[0].conj(), X[0] * X[1].conj(), X[1] * X[1].conj()]))


def psd_of(e):
    return _stft_and_psd(e.F, e.T, 3000 + 10 * e.F + e.T)[1]


def nmf_inputs(F, N):
    rng = np.random.default_rng(4000 + 10 * F + N)
    return dict(F=F, N=N, W=_pos(rng, F, K), H=_pos(rng, K, N), J=2,
                src=np.array([0, 0, 1], dtype=np.int32),   # two components in source 0
                psd=0.1 + rng.random(F), X=np.ascontiguousarray(_cplx(rng, F, N)))


SF_SOURCES = ((0, 0, -1), (1, 0, 1))   # src_of: a dropped component; a shared source
# one source made of both components, column sets {0, 2} and {1}: NS = 1 != J
ONE_SOURCE = [[(0, 0b101), (1, 0b010)]]


# ---- the four STFT-waveform calls: (status, y), y NaN-filled before the call -------
def call_separate(_lib, e, nsrc, w, aw, nfft, hop, n=None):
    y = np.full((nsrc, 2, n or istft_len(False, w.size, hop, e.T)), np.nan)
    psd = psd_of(e)
    st = _lib.lib.fasst_separate_waveforms(e._h, _lib.dptr(psd), _lib.dptr(w), _opt(_lib, aw),
                                           w.size, nfft, hop, _lib.dptr(y))
    return st, y


def call_spatial(_lib, e, nsrc, w, aw, nfft, hop, n=None):
    y = np.full((nsrc, 2, n or istft_len(False, w.size, hop, e.T)), np.nan)
    st = _lib.lib.fasst_spatial_filter_waveforms(e._h, _lib.dptr(w), _opt(_lib, aw), w.size, nfft,
                                                 hop, _lib.dptr(y))
    return st, y


def call_sf(_lib, e, src_of, w, aw, nfft, hop, n=None):
    s = np.ascontiguousarray(src_of, dtype=np.int32)
    nsrc = int(s.max()) + 1
    y = np.full((nsrc, 2, n or istft_len(False, w.size, hop, e.T)), np.nan)
    psd = psd_of(e)
    st = _lib.lib.fasst_sf_separate_waveforms(e._h, _lib.dptr(psd), nsrc, _lib.iptr(s),
                                              _lib.dptr(w), _opt(_lib, aw), w.size, nfft, hop,
                                              _lib.dptr(y))
    return st, y


def call_nmf(_lib, m, w, aw, nfft, hop, n=None):
    y = np.full((m["J"], n or istft_len(False, w.size, hop, m["N"])), np.nan)
    st = _lib.lib.nmf_wiener_waveforms(0, m["F"], m["N"], K, _lib.dptr(m["W"]), _lib.dptr(m["H"]),
                                       m["J"], _lib.iptr(m["src"]), _lib.dptr(m["psd"]),
                                       _lib.dptr(m["X"]), _lib.dptr(w), _opt(_lib, aw), w.size,
                                       nfft, hop, _lib.dptr(y))
    return st, y


def _ok(_lib, res):
    st, y = res
    assert st == _lib.FASST_OK, _lib.last_error()
    assert not np.isnan(y).any()
    return y


def _refused(_lib, res):
    st, y = res
    assert st != _lib.FASST_OK
    assert np.isnan(y).all(), "a refused call wrote its output"
    return np.array([st])


def _refusals(_lib, out, name, call, F, T):
    """call(w, aw, nfft, hop, n): the three bad geometries a model of F = 5
    (nfft = 8) can be given; n sizes the output as the valid call's."""
    assert F == 5
    w8, _ = _windows(8)
    w10, _ = _windows(10)
    n = istft_len(False, 8, 2, T)
    out["refuse_%s_wlen_above_nfft" % name] = _refused(_lib, call(w10, None, 8, 2, n))
    out["refuse_%s_hop_0" % name] = _refused(_lib, call(w8, None, 8, 0, n))
    out["refuse_%s_other_bin_count" % name] = _refused(_lib, call(w8, None, 16, 2, n))


def _refuse_nfft_12(_lib, out):
    w, _ = _windows(8)
    T, n = 4, istft_len(False, 8, 2, 4)
    e = main_engine(BAD_F, T)
    out["refuse_separate_nfft_12"] = _refused(_lib, call_separate(_lib, e, 2, w, None, 12, 2, n))
    e.close()
    e = main_engine(BAD_F, T, conv=(True, True))
    out["refuse_spatial_nfft_12"] = _refused(_lib, call_spatial(_lib, e, 2, w, None, 12, 2, n))
    e.close()
    e = sf_engine(BAD_F, T)
    out["refuse_sf_nfft_12"] = _refused(_lib, call_sf(_lib, e, SF_SOURCES[1], w, None, 12, 2, n))
    e.close()
    out["refuse_nmf_nfft_12"] = _refused(_lib, call_nmf(_lib, nmf_inputs(BAD_F, T), w, None, 12, 2, n))


# ---- cases ---------------------------------------------------------------------
def stft_cases(_lib, out):
    for nfft, wlen, hop, T in ISTFT_SHAPES:
        F = nfft // 2 + 1
        g = "%d_%d_%d_%d" % (nfft, wlen, hop, T)
        w, aw = _windows(wlen)
        wins = (("aw", aw), ("noaw", None))
        first = nfft == 8   # the refusals run on the first geometry's contexts

        e = main_engine(F, T)
        _keep(out, "main_images_" + g, e.wiener_images(psd_of(e)))
        for tag, a in wins:
            _keep(out, "main_waveforms_%s_%s" % (g, tag), _ok(_lib, call_separate(_lib, e, 2, w, a, nfft, hop)))
        e.set_sources(ONE_SOURCE)
        _keep(out, "main_images_one_source_" + g, e.wiener_images(psd_of(e)))
        for tag, a in wins:
            _keep(out, "main_waveforms_one_source_%s_%s" % (g, tag),
                  _ok(_lib, call_separate(_lib, e, 1, w, a, nfft, hop)))
        e.set_sources(None)
        if first:
            _refusals(_lib, out, "separate", lambda *a: call_separate(_lib, e, 2, *a), F, T)
            _keep(out, "after_refusals_separate", _ok(_lib, call_separate(_lib, e, 2, w, aw, nfft, hop)))
        e.close()

        e = main_engine(F, T, conv=(True, True))
        _keep(out, "spatial_gains_" + g, e.spatial_filter_gains())
        _keep(out, "spatial_images_" + g, e.spatial_filter_images())
        for tag, a in wins:
            _keep(out, "spatial_waveforms_%s_%s" % (g, tag), _ok(_lib, call_spatial(_lib, e, 2, w, a, nfft, hop)))
        if first:
            _refusals(_lib, out, "spatial", lambda *a: call_spatial(_lib, e, 2, *a), F, T)
            _keep(out, "after_refusals_spatial", _ok(_lib, call_spatial(_lib, e, 2, w, aw, nfft, hop)))
        e.close()

        e = sf_engine(F, T)
        for s, src_of in enumerate(SF_SOURCES):
            _keep(out, "sf_images_%s_src%d" % (g, s), e.sf_wiener_images(psd_of(e), src_of))
            for tag, a in wins:
                _keep(out, "sf_waveforms_%s_src%d_%s" % (g, s, tag),
                      _ok(_lib, call_sf(_lib, e, src_of, w, a, nfft, hop)))
        if first:
            _refusals(_lib, out, "sf", lambda *a: call_sf(_lib, e, SF_SOURCES[1], *a), F, T)
            _keep(out, "after_refusals_sf", _ok(_lib, call_sf(_lib, e, SF_SOURCES[1], w, aw, nfft, hop)))
        e.close()

        m = nmf_inputs(F, T)
        from pyfasst_amd.tools import nmf
        _keep(out, "nmf_images_" + g, nmf.NMF_wiener_images(m["X"], m["W"], m["H"], {0: [0, 1], 1: [2]},
                                                            psd=m["psd"]))
        for tag, a in wins:
            _keep(out, "nmf_waveforms_%s_%s" % (g, tag), _ok(_lib, call_nmf(_lib, m, w, a, nfft, hop)))
        if first:
            _refusals(_lib, out, "nmf", lambda *a: call_nmf(_lib, m, *a), F, T)
            _keep(out, "after_refusals_nmf", _ok(_lib, call_nmf(_lib, m, w, aw, nfft, hop)))
    _refuse_nfft_12(_lib, out)


def no_stft_cases(_lib, out):
    """A context holding only set_cx refuses; given its STFT it then answers."""
    nfft, wlen, hop, T = ISTFT_SHAPES[0]
    F = nfft // 2 + 1
    w, aw = _windows(wlen)
    for name, make, call in (
            ("separate", lambda: main_engine(F, T, stft=False),
             lambda e: call_separate(_lib, e, 2, w, aw, nfft, hop)),
            ("spatial", lambda: main_engine(F, T, conv=(True, True), stft=False),
             lambda e: call_spatial(_lib, e, 2, w, aw, nfft, hop)),
            ("sf", lambda: sf_engine(F, T, stft=False),
             lambda e: call_sf(_lib, e, SF_SOURCES[1], w, aw, nfft, hop))):
        e = make()
        out["refuse_%s_no_stft" % name] = _refused(_lib, call(e))
        give_observation(e)
        _keep(out, "after_no_stft_" + name, _ok(_lib, call(e)))
        e.close()


def cqt_cases(out):
    """The three calls that end in the batched inverse, on the 'mqt' model of
    test_gpu_cqt_resident.py with J = 2; the two-factor one on its 'inst'
    variant with source / filter factors on component 0."""
    import test_gpu_cqt_resident as R
    with tempfile.TemporaryDirectory() as tmp:
        m = R.model(tmp, 'mqt', J=2)
        _keep(out, "cqt_separate", m.separated_waveforms())
        _keep(out, "cqt_spatial", m.spatial_filter_waveforms())
        m = R.model(tmp, 'mqt', J=2, K=4, conv=False, rank=1)
        F, T = m.nbFreqsSigRepr, m.nbFramesSigRepr
        rs = np.random.RandomState(7)
        m.spec_comps[0]['factor'] = {0: R._factor(rs, F, T, 13, 13, (R.FIX, R.FIX, R.FREE), True),
                                     1: R._factor(rs, F, T, 6, 3, (R.FIX, R.FREE, R.FREE))}
        assert m._is_sf()
        _keep(out, "cqt_sf_separate", m.separated_waveforms({0: [0], 1: [1]}))


def run_cases(_lib):
    out = {}
    stft_cases(_lib, out)
    no_stft_cases(_lib, out)
    cqt_cases(out)
    return out
