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


# ---- set / get round trips: offsets into a larger buffer, padded pitches ----
# F = 5 (Fp = 16), T = 7 (Tp = 16), K = 3 (below every padded KP), two sources:
# source 1's rows start at a non-zero offset, right behind source 0's.
RT_F, RT_T, RT_K = 5, 7, 3


def rt_engine(ranks=(2, 2), conv=(True, False)):
    from pyfasst_amd.engine import Engine
    e = Engine(RT_F, RT_T)
    e.configure(list(ranks), [RT_K] * len(ranks), list(conv))
    return e


def rt_rand(seed, *shape):
    return 0.5 + np.random.default_rng(seed).random(shape)


def sfnmf_round_trip(_lib, F, N, Ks, seed):
    """(what was set, what came back): W [F, K] and H [K, N] of the three
    factors of a source/filter NMF context."""
    h = ctypes.c_void_p()
    st = _lib.lib.sfnmf_create(0, F, N, Ks[0], Ks[1], Ks[2], ctypes.byref(h))
    assert st == _lib.FASST_OK, _lib.last_error()
    try:
        sent = []
        for i, K in enumerate(Ks):
            sent += [rt_rand(seed + 2 * i, F, K), rt_rand(seed + 2 * i + 1, K, N)]
        st = _lib.lib.sfnmf_set_params(h, *[_lib.dptr(a) for a in sent])
        assert st == _lib.FASST_OK, _lib.last_error()
        back = [np.full(a.shape, np.nan) for a in sent]
        st = _lib.lib.sfnmf_get_params(h, *[_lib.dptr(a) for a in back])
        assert st == _lib.FASST_OK, _lib.last_error()
        return sent, back
    finally:
        _lib.lib.sfnmf_destroy(h)


# ---- compute entry points whose host side moved onto DSpan -------------------
def call_viterbi(_lib, S, N, ld_d, ld_t, seed):
    """viterbi_tracking with host leading dimensions above the row widths, so
    both pitched uploads are narrower than their host pitch."""
    rng = np.random.default_rng(seed)
    dens = np.ascontiguousarray(rng.standard_normal((S, ld_d)))
    trans = np.ascontiguousarray(np.log(rng.random((S, ld_t))))
    prior = np.log(rng.random(S))
    path = np.full(N, -1, dtype=np.int64)
    st = _lib.lib.viterbi_tracking(0, S, N, _lib.dptr(dens), ld_d, _lib.dptr(prior),
                                   _lib.dptr(trans), ld_t,
                                   path.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    assert st == _lib.FASST_OK, _lib.last_error()
    return path


def call_nsgt_fft(_lib, n, sign, seed):
    x = np.ascontiguousarray(_cplx(np.random.default_rng(seed), n))
    out = np.full(n, np.nan + 0j)
    st = _lib.lib.fasst_nsgt_fft(0, n, sign, _lib.dptr(x), _lib.dptr(out))
    assert st == _lib.FASST_OK, _lib.last_error()
    return out


def digest(a):
    """A large output as its SHA-256 (shape and dtype included): equal digests
    are equal bits, and the fixture stays small."""
    import hashlib
    a = np.ascontiguousarray(a)
    assert not np.isnan(a).any()
    h = hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode() + a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _keep(out, name, a):
    a = np.ascontiguousarray(a)
    if a.nbytes <= 2048:
        out[name] = a
    else:
        out[name + "_sha256"] = digest(a)


def cqt_cases(out):
    """cqt24 on 101 samples, the smallest geometry of test_gpu_cqt_cells.py
    (4 octaves, the last of 3 frames): the cells, their raster and the inverse
    (perfRast = 0); the raster path forward and inverse (perfRast = 1) on
    test_gpu_cqt.py's cqt12 signal."""
    import cqt_cells_ref as C
    from pyfasst_amd.tftransforms import minqt
    kw = C.CASES["cqt24"][1]
    x = C.signal("cqt24")
    t = minqt.CQTransfo(**kw)
    t.computeTransform(x)
    for k, v in sorted(t.cellCQT.items(), key=lambda kv: str(kv[0])):
        _keep(out, "cqt_cell_%s" % k, np.array(v))
    _keep(out, "cqt_cells_raster", np.array(t.transfo))
    _keep(out, "cqt_cells_inverse", t.invertTransform())
    from helpers import CQT_CASES, load
    r = minqt.CQTransfo(perfRast=1, **CQT_CASES[3][2])   # cqt12 of test_gpu_cqt.py
    r.computeTransform(load("cqt")["x"])
    X = np.array(r.transfo)
    _keep(out, "cqt_raster_forward", X)
    r.transfo = X
    _keep(out, "cqt_raster_inverse", r.invertTransform())


def filter_cases(out):
    from pyfasst_amd.tftransforms.stft import filter_stft
    rs = np.random.RandomState(92)
    x = rs.randn(50, 2)
    W = rs.randn(2, 2, 33) + 1j * rs.randn(2, 2, 33)
    w, aw = _windows(64)
    _keep(out, "filter_stft", filter_stft(x, W, analysisWindow=aw, synthWindow=w, hopsize=16.0,
                                          nfft=64.0))


def nmf_cases(_lib, out):
    """One iteration of each context, then its getters.  F, N and the ranks
    are odd and below every padded size."""
    from pyfasst_amd.tools import nmf
    import pyfasst_amd.SeparateLeadStereo.SIMM.SIMM as SIMM
    F, N = 33, 17
    rs = np.random.RandomState(93)
    SXR, SXL = rs.gamma(0.8, 1.0, (F, N)), rs.gamma(0.8, 1.0, (F, N))
    for K in (3, 16):   # 16: the fused kernels and their transposed copies
        W, H = nmf._run(SXR, 0.5 + rs.rand(F, K), 0.5 + rs.rand(K, N), 1, True, True, None)
        _keep(out, "nmf_K%d_W" % K, W)
        _keep(out, "nmf_K%d_H" % K, H)
    R = 3
    res = SIMM._stereo_nmf_run(SXR, SXL, 0.5 + rs.rand(F, R), 0.5 + rs.rand(R, N), rs.rand(R), 1,
                               1.0, True, _lib.default_device())
    for name, a in zip(("bR", "bL", "HM", "WM", "err"), res):
        _keep(out, "snmf_" + name, np.asarray(a, dtype=np.float64))
    WF0, WG = rs.gamma(1.0, 1.0, (F, 5)), rs.gamma(1.0, 1.0, (F, 3))
    np.random.seed(94)
    res = SIMM.Stereo_SIMM(SXR, SXL, WF0, WG, numberOfFilters=1,
                           numberOfAccompanimentSpectralShapes=1, numberOfIterations=1,
                           computeError=True, verbose=False)
    for i, a in enumerate(res):
        _keep(out, "simm_stereo_%d" % i, np.asarray(a, dtype=np.float64))
    np.random.seed(95)
    res = SIMM.SIMM(SXR, WF0, WG, numberOfFilters=1, numberOfAccompanimentSpectralShapes=1,
                    numberOfIterations=1, verbose=False)
    for i, a in enumerate(res):
        _keep(out, "simm_mono_%d" % i, np.asarray(a, dtype=np.float64))


def nsgt_cases(out):
    """NSGT forward and backward on host arrays of the prime length 101, real
    (y is one double per sample) and complex (two per sample)."""
    import warnings
    from pyfasst_amd.tftransforms.nsgt import NSGT, OctScale
    rs = np.random.RandomState(96)
    for real in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = NSGT(OctScale(500, 3500, 4), 8000, 101, real=real, matrixform=False)
        x = rs.randn(101)
        c = t.forward(x)
        tag = "real" if real else "cplx"
        _keep(out, "nsgt_%s_forward" % tag, np.concatenate([np.ravel(b) for b in c]))
        _keep(out, "nsgt_%s_backward" % tag, np.asarray(t.backward(c)))


def gemm_cases(_lib, out):
    """The guarded-buffer harness: A one double past the allocation's base
    (a_skew = 1), guard words on both sides of every payload."""
    M, N, K, lda, ldb, ldc = 5, 6, 7, 6, 8, 9
    rng = np.random.default_rng(97)
    A = np.zeros((K, lda))
    B = np.zeros((K, ldb))
    A[:, :M] = rng.integers(-8, 9, (K, M))
    B[:, :N] = rng.integers(-8, 9, (K, N))
    C = np.full((M, ldc), -3.0)
    arm = ctypes.c_int(-1)
    st = _lib.lib.fasst_dgemm2_probe(0, M, N, K, _lib.dptr(A), lda, 1, _lib.dptr(B), ldb, 0,
                                     _lib.dptr(C), ldc, 0, ctypes.byref(arm))
    assert st == _lib.FASST_OK, _lib.last_error()
    assert np.array_equal(C[:, :N], A[:, :M].T @ B[:, :N])   # small integers: exact
    out["gemm_skew_C"] = C
    out["gemm_skew_arm"] = np.array([arm.value])


def run_compute_cases(_lib):
    out = {"viterbi_3_5": call_viterbi(_lib, 3, 5, 8, 4, 90)}
    for n in (7, 101):   # primes: the chirp-z path, tables uploaded per call
        for sign in (-1, 1):
            out["nsgt_fft_%d_%s" % (n, "fwd" if sign < 0 else "inv")] = call_nsgt_fft(_lib, n, sign, 91 + n)
    cqt_cases(out)
    filter_cases(out)
    nmf_cases(_lib, out)
    nsgt_cases(out)
    gemm_cases(_lib, out)
    return out
