"""The stateless entry points whose host side is mostly transfers, at shapes
small enough to pin bit for bit: fasst_stft, fasst_istft, fasst_istft_simm,
fasst_mix_solve, fasst_inv_sigma_mix and fasst_wiener_gain.

run_cases() calls the library on seeded inputs and returns {name: array}.
tests/golden/make_golden_host_transfers.py saved its result once from the
library as it stood before the transfers went through DBuf's typed
upload / put / get; test_gpu_host_transfers.py compares against that with
tolerance 0 (same kernels, same inputs: any difference is a host bug).
"""
import ctypes

import numpy as np

# (nfft, wlen, hop, T): wlen == nfft with a dividing hop; wlen < nfft with a
# hop that does not divide the window
ISTFT_SHAPES = ((8, 8, 2, 5), (16, 8, 3, 4))
# signal lengths for nfft = wlen = 8, hop = 2: the empty signal and one sample
# (the device buffer is larger than the copy), and a ragged last frame
STFT_LENGTHS = (0, 1, 9)
STFT_NFFT, STFT_HOP = 8, 2


def _cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _windows(wlen):
    w = np.sin(np.pi * (np.arange(wlen) + 0.5) / wlen)
    aw = np.ascontiguousarray(w ** 2 + 0.25)
    return np.ascontiguousarray(w), aw


def istft_len(simm, wlen, hop, T):
    return hop * (T - 1) + wlen - (0 if simm else wlen // 2)


def call_istft(_lib, simm, X, w, aw, nfft, hop):
    """(status, y) of fasst_istft_simm / fasst_istft on X [F, T]."""
    fn = _lib.lib.fasst_istft_simm if simm else _lib.lib.fasst_istft
    T = X.shape[1]
    y = np.full(istft_len(simm, w.size, hop, T), np.nan)
    st = fn(0, _lib.dptr(X), T, _lib.dptr(w), _lib.dptr(aw) if aw is not None else None, w.size,
            nfft, hop, _lib.dptr(y))
    return st, y


def call_stft(_lib, x, w, nfft, hop):
    T = ctypes.c_int(0)
    xb = x if x.size else np.zeros(1)   # a valid pointer for the empty signal
    st = _lib.lib.fasst_stft(0, _lib.dptr(xb), x.size, _lib.dptr(w), w.size, nfft, hop, None,
                             ctypes.byref(T))
    assert st == _lib.FASST_OK, _lib.last_error()
    X = np.full((nfft // 2 + 1, T.value), np.nan + 0j)
    st = _lib.lib.fasst_stft(0, _lib.dptr(xb), x.size, _lib.dptr(w), w.size, nfft, hop,
                             _lib.dptr(X), ctypes.byref(T))
    assert st == _lib.FASST_OK, _lib.last_error()
    return X


def mix_solve_inputs(F, R, seed):
    rng = np.random.default_rng(seed)
    a = _cplx(rng, F, R, R)
    rss = a @ a.conj().transpose(0, 2, 1) + R * np.eye(R)   # Hermitian, well conditioned
    return (np.ascontiguousarray(rss), _cplx(rng, F, 2, R), _cplx(rng, R, 2, F))


def call_mix_solve(_lib, rss, rxs, mix, kind):
    """(status, mix after the call); the caller's mix is left alone."""
    F, R = rss.shape[0], rss.shape[1]
    out = mix.copy()
    k = np.ascontiguousarray(kind, dtype=np.int32)
    st = _lib.lib.fasst_mix_solve(0, F, R, _lib.dptr(rss), _lib.dptr(rxs), _lib.dptr(out),
                                  _lib.iptr(k))
    return st, out


def call_inv_sigma_mix(_lib, n, F, T, seed):
    rng = np.random.default_rng(seed)
    diag = 1.0 + rng.random((n, 2, F, T))
    off = 0.25 * _cplx(rng, n, F, T)
    psd = 0.1 + rng.random(F)
    idiag = np.full((2, F, T), np.nan)
    ioff = np.full((F, T), np.nan + 0j)
    st = _lib.lib.fasst_inv_sigma_mix(0, n, F, T, _lib.dptr(diag), _lib.dptr(off), _lib.dptr(psd),
                                      _lib.dptr(idiag), _lib.dptr(ioff))
    assert st == _lib.FASST_OK, _lib.last_error()
    return idiag, ioff


def call_wiener_gain(_lib, n, seed):
    rng = np.random.default_rng(seed)
    sd, isd = 1.0 + rng.random((2, n)), 1.0 + rng.random((2, n))
    so, iso = _cplx(rng, n), _cplx(rng, n)
    WG = np.full((2, 2, n), np.nan + 0j)
    st = _lib.lib.fasst_wiener_gain(0, n, _lib.dptr(sd), _lib.dptr(so), _lib.dptr(isd),
                                    _lib.dptr(iso), _lib.dptr(WG))
    assert st == _lib.FASST_OK, _lib.last_error()
    return WG


def run_cases(_lib):
    out = {}
    for nfft, wlen, hop, T in ISTFT_SHAPES:
        X = np.ascontiguousarray(_cplx(np.random.default_rng(nfft), nfft // 2 + 1, T))
        w, aw = _windows(wlen)
        for simm in (False, True):
            for tag, a in (("aw", aw), ("noaw", None)):
                st, y = call_istft(_lib, simm, X, w, a, nfft, hop)
                assert st == _lib.FASST_OK, _lib.last_error()
                out["istft%s_%d_%d_%d_%d_%s" % ("_simm" if simm else "", nfft, wlen, hop, T, tag)] = y
    w, _ = _windows(STFT_NFFT)
    for L in STFT_LENGTHS:
        x = np.random.default_rng(100 + L).standard_normal(L)
        out["stft_L%d" % L] = call_stft(_lib, x, w, STFT_NFFT, STFT_HOP)
    for name, R, kind in (("conv", 2, [2, 2]), ("inst", 3, [1, 1, 1])):
        st, mix = call_mix_solve(_lib, *mix_solve_inputs(3, R, 7 + R), kind)
        assert st == _lib.FASST_OK, _lib.last_error()
        out["mix_solve_" + name] = mix
    for n, F, T in ((2, 3, 5), (2, 1, 257)):
        idiag, ioff = call_inv_sigma_mix(_lib, n, F, T, 20 + T)
        out["inv_sigma_mix_%d_%d_%d_diag" % (n, F, T)] = idiag
        out["inv_sigma_mix_%d_%d_%d_off" % (n, F, T)] = ioff
    for n in (15, 257):
        out["wiener_gain_%d" % n] = call_wiener_gain(_lib, n, 30 + n)
    return out
