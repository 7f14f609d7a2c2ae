"""NumPy restatement of the reference's filter_stft (tftransforms/stft.py:
133-227) and filter_conv_stft (:229-334), step for step in the reference's
order of operations (what NumPy < 1.12 did with the float sizes is written
with ints).  CPU only; tests/test_filter_stft_ref_golden.py pins it to the
fixtures of tests/golden/make_golden_filter.py, and the GPU tests run it live
for the shapes that have no fixture.

Also the case table shared by the maker and the tests: `CASES[name]` holds
the parameters, `draw(name)` redraws the inputs from RandomState(seed) with
the calls the maker made.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_stft.npz")


def sinebell(n):
    return np.sin((np.pi * np.arange(n)) / (1.0 * n))    # tools/utils.py:41-53


def _frame_setup(ns, analysisWindow, synthWindow, hopsize):
    if analysisWindow is None or len(analysisWindow) != len(synthWindow):
        analysisWindow = synthWindow
    wlen = synthWindow.size
    nframes = int(np.ceil(ns / np.double(hopsize)))
    newlen = int((nframes - 1) * hopsize + wlen)
    return analysisWindow, wlen, nframes, newlen


def filter_stft(data, W, analysisWindow=None, synthWindow=sinebell(2048), hopsize=256.0,
                nfft=2048.0, fs=44100.0):
    ns, nc = data.shape
    if nc != W.shape[0]:
        raise AttributeError("W does not have the right number of channels")
    analysisWindow, wlen, nframes, newlen = _frame_setup(ns, analysisWindow, synthWindow, hopsize)
    data = np.concatenate((np.zeros([wlen // 2, nc]), data))
    data = np.concatenate((data, np.zeros([newlen - data.shape[0], nc])))   # ValueError if < 0
    nfreq = int(nfft) // 2 + 1
    if nfreq != W.shape[2]:
        raise AttributeError("W not the right size")
    norm = np.zeros(newlen)
    out = np.zeros([newlen, nc])
    for n in range(nframes):
        b = int(n * hopsize)
        e = b + wlen
        ft = np.zeros([nc, nfreq], dtype=complex)
        for c in range(nc):
            ft[c] = np.fft.rfft(analysisWindow * data[b:e, c], int(nfft))
        fft = np.zeros_like(ft)
        if W.ndim == 3:
            for c1 in range(nc):
                for c2 in range(nc):
                    fft[c1] += W[c1, c2] * ft[c2]
        elif W.ndim == 4:
            for c1 in range(nc):
                for c2 in range(nc):
                    fft[c1] += W[c1, c2, :, n] * ft[c2]
        else:
            raise NotImplementedError("For W.ndim== 3 or 4" + str(W.ndim))
        norm[b:e] = norm[b:e] + synthWindow * analysisWindow
        for c in range(nc):
            fr = np.fft.irfft(fft[c], int(nfft))[:wlen]
            out[b:e, c] = out[b:e, c] + synthWindow * fr
    out = out[wlen // 2:]
    norm = norm[wlen // 2:]
    norm[norm == 0] = 1.
    return out / np.vstack(norm)


def filter_conv_stft(data, W, analysisWindow=None, synthWindow=sinebell(2048), hopsize=256.0,
                     nfft=2048.0, fs=44100.0, verbose=0):
    if (data.ndim == 2 and data.shape[1] != 1) or (data.ndim > 2):
        raise AttributeError("provided data should be single channel")
    if data.ndim == 2 and data.shape[1] == 1:
        data = data.flatten()
    ns = data.size
    nout = W.shape[0]
    analysisWindow, wlen, nframes, newlen = _frame_setup(ns, analysisWindow, synthWindow, hopsize)
    data = np.concatenate((np.zeros(wlen // 2), data))
    data = np.concatenate((data, np.zeros(newlen - data.shape[0])))
    nfreq = int(nfft) // 2 + 1
    if nfreq != W.shape[1]:
        raise AttributeError("W not the right size")
    norm = np.zeros(newlen)
    out = np.zeros([newlen, nout])
    for n in range(nframes):
        b = int(n * hopsize)
        e = b + wlen
        ft = np.fft.rfft(analysisWindow * data[b:e], int(nfft))
        if W.ndim == 2:
            fft = W * ft
        elif W.ndim == 3:
            fft = W[:, :, n] * ft
        else:
            raise ValueError("The provided filter does not have the right shape.")
        norm[b:e] = norm[b:e] + synthWindow * analysisWindow
        for c in range(nout):
            fr = np.fft.irfft(fft[c], int(nfft))[:wlen]
            out[b:e, c] = out[b:e, c] + synthWindow * fr
    out = out[wlen // 2:]
    norm = norm[wlen // 2:]
    norm[norm == 0] = 1.
    return out / np.vstack(norm)


# name -> parameters.  fn: 'stft' (filter_stft) or 'conv' (filter_conv_stft);
# M: channels (outputs of 'conv'); wdim: W.ndim; cplx: complex W; extra: surplus
# W frames; win: 'sine' (analysis = synthesis = sine bell), 'distinct'
# (hanning + 0.1 against a sine bell), 'wronglen' (an analysis window of
# wlen + 3 samples, which is replaced), 'none'; col: [T, 1] input for 'conv'.
def _c(fn, L, wlen, nfft, hop, M, wdim, cplx=True, extra=0, win='distinct', col=False):
    return dict(fn=fn, L=L, wlen=wlen, nfft=nfft, hop=hop, M=M, wdim=wdim, cplx=cplx, extra=extra,
                win=win, col=col)


CASES = {
    "base_m2": _c('stft', 1000, 64, 64, 16, 2, 3),
    "pad_m2_tv": _c('stft', 1000, 64, 128, 16, 2, 4),
    "mult_m1": _c('stft', 1024, 64, 64, 16, 1, 3, cplx=False),
    "short_m3": _c('stft', 50, 64, 64, 16, 3, 4),
    "hop24_m3": _c('stft', 1001, 64, 128, 24, 3, 3),
    "m4_tv_real": _c('stft', 1000, 64, 64, 16, 4, 4, cplx=False),
    "m5_surplus": _c('stft', 1000, 64, 128, 16, 5, 4, extra=2),
    "m5_ti_sine": _c('stft', 1000, 64, 64, 16, 5, 3, win='sine'),
    "wronglen_m2": _c('stft', 1000, 64, 64, 16, 2, 3, win='wronglen'),
    "none_m2": _c('stft', 1000, 64, 64, 24, 2, 4, win='none'),
    "conv_m1": _c('conv', 1000, 64, 64, 16, 1, 2),
    "conv_m2_tv": _c('conv', 1001, 64, 128, 24, 2, 3),
    "conv_m3_col": _c('conv', 1000, 64, 64, 16, 3, 3, cplx=False, col=True, extra=2),
    "conv_m3_ti": _c('conv', 50, 64, 128, 16, 3, 2, win='sine'),
    "lds_4096": _c('stft', 6000, 4096, 4096, 1024, 2, 4),
}


def seed_of(name):
    return sum(map(ord, name)) % 1000


def draw(name):
    """(data, W, analysisWindow, synthWindow) of a case, from RandomState(seed)."""
    c = CASES[name]
    rs = np.random.RandomState(seed_of(name))
    F = c['nfft'] // 2 + 1
    nframes = -(-c['L'] // c['hop']) + c['extra']
    if c['fn'] == 'stft':
        data = rs.randn(c['L'], c['M'])
        shape = (c['M'], c['M'], F) + ((nframes,) if c['wdim'] == 4 else ())
    else:
        data = rs.randn(c['L'], 1) if c['col'] else rs.randn(c['L'])
        shape = (c['M'], F) + ((nframes,) if c['wdim'] == 3 else ())
    W = rs.randn(*shape)
    if c['cplx']:
        W = W + 1j * rs.randn(*shape)
    sw = sinebell(c['wlen'])
    aw = {'sine': sw, 'distinct': np.hanning(c['wlen']) + 0.1,
          'wronglen': np.hanning(c['wlen'] + 3) + 0.1, 'none': None}[c['win']]
    return data, W, aw, sw


def run_ref(name, mod=None):
    """The case through `mod` (this module by default)."""
    import sys
    mod = mod or sys.modules[__name__]
    c = CASES[name]
    data, W, aw, sw = draw(name)
    fn = mod.filter_stft if c['fn'] == 'stft' else mod.filter_conv_stft
    return fn(data, W, analysisWindow=aw, synthWindow=sw, hopsize=float(c['hop']),
              nfft=float(c['nfft']))
