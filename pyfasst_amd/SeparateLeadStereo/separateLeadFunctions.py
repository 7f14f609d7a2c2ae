"""SIMM-pipeline STFT / iSTFT and dictionaries on the GPU (reference:
SeparateLeadStereo/separateLeadFunctions.py:90-521, :696-1146).

These differ from tftransforms/stft.py: `stft` takes a start/stop frame range
and pads half a window at both ends (:90-161); `istft` keeps the leading half
window and patches the first / last window of the normalisation from their
neighbours (:163-233).  FFTs and overlap-add run in libfasst_hip.so.
"""
import ctypes
import os

import numpy as np

from .. import _lib
from .._lib import check, dptr, lib
from ..tools.utils import nextpow2, sinebell

__all__ = ["nextpow2", "sinebell", "stft", "istft", "generate_WF0_chirped",
           "generate_WF0_MinQT_chirped", "generate_WF0_NSGTMinQT_chirped",
           "generate_WF0_TR_chirped", "generate_ODGD_spec", "generate_ODGD_spec_inharmo",
           "generate_ODGD_spec_chirped", "generateHannBasis"]


def _dev(device):
    return _lib.default_device() if device is None else device


def _int_hop(hopsize):
    if float(hopsize) != int(hopsize):
        raise NotImplementedError("non-integer hopsize %r" % (hopsize,))
    return int(hopsize)


def stft(data, window=sinebell(2048), hopsize=256.0, nfft=2048.0, fs=44100.0, start=0,
         stop=None, device=None):
    """X, F, N = stft(...)  (separateLeadFunctions.py:90-161)."""
    x = np.ascontiguousarray(np.asarray(data, dtype=np.float64).ravel())
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    L = w.size
    hop = _int_hop(hopsize)
    nfft_i = int(nfft)
    # frame count of :127-131 (half a window of zeros on both sides)
    n_data = x.size + 2 * int(L / 2.0)
    n_frames = int(np.ceil((n_data - L) / float(hopsize) + 1) + 1)
    T = ctypes.c_int(0)
    check(lib.fasst_stft(_dev(device), dptr(x), x.size, dptr(w), L, nfft_i, hop, None,
                         ctypes.byref(T)), "fasst_stft")
    Xall = np.empty((nfft_i // 2 + 1, T.value), dtype=np.complex128)
    check(lib.fasst_stft(_dev(device), dptr(x), x.size, dptr(w), L, nfft_i, hop, dptr(Xall),
                         ctypes.byref(T)), "fasst_stft")
    if stop is None:
        stop = n_frames
    if stop > n_frames or start < 0:
        raise ValueError("frames %d:%d outside the %d analysed frames" % (start, stop, n_frames))
    X = np.ascontiguousarray(Xall[:, start:stop])
    F = np.arange(nfft_i // 2 + 1) / nfft * fs
    N = np.arange(n_frames) * hopsize / fs
    return X, F, N


def istft(X, analysisWindow=None, window=sinebell(2048), hopsize=256.0, nfft=2048.0,
          originalDataLen=None, start=-1, stop=None, device=None):
    """data = istft(...)  (separateLeadFunctions.py:163-233)."""
    if analysisWindow is None:
        analysisWindow = window
    X = np.ascontiguousarray(X, dtype=np.complex128)
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    aw = np.ascontiguousarray(np.asarray(analysisWindow, dtype=np.float64))
    nfft_i, hop = int(nfft), _int_hop(hopsize)
    if X.shape[0] != nfft_i // 2 + 1:
        raise ValueError("X has %d bins, nfft=%d needs %d" % (X.shape[0], nfft_i, nfft_i // 2 + 1))
    T = X.shape[1]
    y = np.empty(hop * (T - 1) + w.size)
    check(lib.fasst_istft_simm(_dev(device), dptr(X), T, dptr(w), dptr(aw), w.size, nfft_i, hop,
                               dptr(y)), "fasst_istft_simm")
    if originalDataLen is not None:
        y = y[:originalDataLen]
    return y


# ---------------------------------------------------------------- dictionaries
def _odgd_amplitudes(F0, Ot, partialMax):
    """KLGLOTT88 partial amplitudes, the reference's expression
    (separateLeadFunctions.py:916-930); host-side parameters of the GPU synthesis."""
    frequency_numbers = np.arange(1, partialMax + 1)
    temp_array = 1j * 2.0 * np.pi * frequency_numbers * Ot
    return (F0 * 27 / 4 * (np.exp(-temp_array) + (2 * (1 + 2 * np.exp(-temp_array)) / temp_array) -
                           (6 * (1 - np.exp(-temp_array)) / (temp_array ** 2))) / temp_array)


def _comb_columns(F0Table, Fs, Ot, perF0, depthChirpInSemiTone):
    """Columns of WF0 (:829-879): the F0 comb, then perF0 - 1 chirps around
    it; per column F1, F2 and the KLGLOTT88 partial amplitudes."""
    f1, f2, amps = [], [], []
    for i in range(F0Table.size):
        F0 = F0Table[i]
        f1.append(F0)
        f2.append(F0)
        amps.append(_odgd_amplitudes(F0, np.double(Ot), np.floor((Fs / 2) / F0)))
        for c in range(perF0 - 1):
            F2 = F0 * (2 ** ((c + 1.0) * depthChirpInSemiTone / (12.0 * (perF0 - 1.0))))
            F1 = 2.0 * F0 - F2
            f1.append(np.double(F1))
            f2.append(np.double(F2))
            amps.append(_odgd_amplitudes(np.double(F1 + F2) / 2.0, np.double(Ot),
                                         np.floor((Fs / 2) / np.max([F1, F2]))))
    ncol = len(f1)
    npart = np.array([a.size for a in amps], dtype=np.int32)
    pmax = max(1, int(npart.max()))
    A = np.zeros((ncol, pmax), dtype=np.complex128)
    for j, a in enumerate(amps):
        A[j, :a.size] = a
    return (np.ascontiguousarray(f1, dtype=np.float64), np.ascontiguousarray(f2, dtype=np.float64),
            npart, pmax, A)


def _f0_table(minF0, maxF0, stepNotes):
    """The F0 grid of the WF0 generators (:312-315, :817-820)."""
    minF0, maxF0, stepNotes = np.double(minF0), np.double(maxF0), np.double(stepNotes)
    numberOfF0 = np.ceil(12.0 * stepNotes * np.log2(maxF0 / minF0)) + 1
    return minF0 * (2 ** (np.arange(numberOfF0, dtype=np.double) / (12 * stepNotes)))


def _wf0_cqt(transform, F0Table, Fs, Ot, perF0, depthChirpInSemiTone, lengthWindow):
    """WF0 on a CQT / MinQT transform: the combs of lengthWindow samples
    through the GPU transform, the column nearest the middle kept (:485-489,
    :840-846; dict_wf0_cqt, include/fasst_cqt.h)."""
    k = transform.cqtkernel
    f1a, f2a, npart, pmax, A = _comb_columns(F0Table, Fs, Ot, perF0, depthChirpInSemiTone)
    # the transform's geometry for a signal of lengthWindow samples and
    # the reference's midindex = argmin (datalen_init / 2 - time_stamps)^2
    F, W, nfr = transform._shape(lengthWindow)
    maxBlock = int(k.FFTLen * (2 ** (transform.octaveNr - 1)))
    time_stamps = (np.arange(nfr[0] * k.winNr) * k.atomHOP +
                   k.first_center * 2 ** (transform.octaveNr - 1) - maxBlock)
    mid = int(np.argmin((lengthWindow / 2. - time_stamps) ** 2))
    WF0 = np.empty((F, f1a.size))
    check(lib.dict_wf0_cqt(transform._context(), f1a.size, dptr(f1a), dptr(f2a),
                           _lib.iptr(npart), pmax, dptr(A), float(Fs), int(lengthWindow), mid,
                           dptr(WF0)), "dict_wf0_cqt")
    return WF0


def generate_WF0_TR_chirped(transform, minF0, maxF0, stepNotes=4, Ot=0.5, perF0=1,
                            depthChirpInSemiTone=0.5, loadWF0=True, verbose=False,
                            device=None):
    """F0Table, WF0, transform = generate_WF0_TR_chirped(...)
    (separateLeadFunctions.py:696-886).

    WF0[:, j] = |transform(odgd_j)[:, middle frame]|^2, the KLGLOTT88 comb
    odgd_j synthesised on the GPU.  For the STFT transform
    (SeparateLeadProcess' default tfrepresentation 'stft') one workgroup per
    column synthesises and transforms only the middle frame (dict_wf0_stft,
    include/fasst_dict.h).  For a CQT / MinQT transform (tfrepresentation
    'cqt' / 'minqt' / 'mqt') the whole comb of FFTLen * 2^(octaveNr-1)
    samples goes through the GPU transform and the middle column is kept
    (dict_wf0_cqt, include/fasst_cqt.h).  The cache file holds F0Table and
    WF0 only (the reference also pickles the transform object)."""
    import os
    cqt = hasattr(transform, 'cqtkernel')
    if cqt:
        k = transform.cqtkernel
        if hasattr(transform, 'octaveNr'):                          # :742-744
            lengthWindow = int(k.FFTLen * (2 ** (transform.octaveNr - 1)))
        else:
            lengthWindow = int(k.linFTLen)
        geo = '_'.join(['atomhopfactor-%s' % str(transform.atomHopFactor),
                        'bins-%s' % str(transform.bins), 'fmax-%s' % str(transform.fmax),
                        'fmin-%s' % str(transform.fmin), 'freqbins-%s' % str(transform.freqbins),
                        'fs-%s' % str(transform.fs),
                        getattr(transform.winFunc, '__name__', 'w')])
    else:
        lengthWindow = (transform.freqbins - 1) * 2 * 2
        geo = '_'.join(['fs-%s' % str(transform.fs), 'ftlen-%d' % transform.ftlen,
                        'hop-%d' % transform.fthop,
                        'win-%s' % getattr(transform.winFunc, '__name__', 'w')])
    filename = ''.join(['wf0gpu_%s_' % transform.transformname, '_minF0-', str(minF0),
                        '_maxF0-', str(maxF0), '_stepNotes-', str(int(stepNotes)),
                        '_Ot-', str(Ot), '_perF0-', str(int(perF0)),
                        '_depthChirp-', str(depthChirpInSemiTone),
                        '_lengthWindow-%d' % lengthWindow, '_', geo, '.npz'])
    if os.path.isfile(filename) and loadWF0:
        struc = np.load(filename)
        return struc['F0Table'], struc['WF0'], transform
    Fs = np.double(transform.fs)
    F0Table = _f0_table(minF0, maxF0, stepNotes)
    if cqt:
        WF0 = _wf0_cqt(transform, F0Table, Fs, Ot, perF0, depthChirpInSemiTone, lengthWindow)
    else:
        f1a, f2a, npart, pmax, A = _comb_columns(F0Table, Fs, Ot, perF0, depthChirpInSemiTone)
        ncol = f1a.size
        # the middle frame of the transform's STFT of an lengthWindow-sample
        # signal (STFT.computeTransform, :838-847 with stft.py:3-69, :383-385)
        hop = int(transform.fthop)
        nfr = int(np.ceil(lengthWindow / np.double(hop))) + 2
        time_stamps = np.arange(nfr) * hop / np.double(transform.fs)
        time_stamps *= transform.fs
        mid = int(np.argmin((lengthWindow / 2. - time_stamps) ** 2))
        window = np.ascontiguousarray(transform.window, dtype=np.float64)
        frame_start = mid * hop - window.size // 2
        WF0 = np.empty((transform.freqbins, ncol))
        dev = _dev(device if device is not None else getattr(transform, 'device', None))
        check(lib.dict_wf0_stft(dev, ncol, dptr(f1a), dptr(f2a), _lib.iptr(npart), pmax, dptr(A),
                                float(Fs), int(lengthWindow), dptr(window), window.size,
                                int(transform.ftlen), int(frame_start), dptr(WF0)),
              "dict_wf0_stft")
    try:
        np.savez(filename, F0Table=F0Table, WF0=WF0)
    except OSError:
        pass
    return F0Table, WF0, transform


# dict_odgd's transform is an in-LDS radix-2 FFT (include/fasst_dict.h)
_ODGD_NFFT_MAX = 8192


def _odgd_nfft(Nfft, who):
    """Nfft as dict_odgd takes it; refused before anything is uploaded."""
    n = int(Nfft)
    if n != Nfft or n < 2 or n > _ODGD_NFFT_MAX or n & (n - 1):
        raise NotImplementedError(
            "%s: Nfft=%r; the GPU transform takes a power of two from 2 to %d"
            % (who, Nfft, _ODGD_NFFT_MAX))
    return n


def _odgd_window(analysisWindowType, lengthOdgd, names, array=False):
    """The analysis window of the ODGD generators (:905-915, :969-977,
    :1030-1038): one of `names`, or (array=True) lengthOdgd values."""
    from ..tools.utils import hann
    if isinstance(analysisWindowType, str):
        if analysisWindowType in names:
            if analysisWindowType == 'sinebell':
                return sinebell(lengthOdgd)
            if analysisWindowType == 'rectangular':
                return np.ones(lengthOdgd)
            return hann(lengthOdgd)
    elif array and len(analysisWindowType) == lengthOdgd:
        return np.asarray(analysisWindowType, dtype=np.float64)
    raise ValueError("Analysis window not understood.")


def _dict_odgd(device, f1, f2, npart, pmax, amps, t_offset, Fs, lengthOdgd, windows, window_sel,
               nfft, odgd=False, spectrum=False, power=False):
    """One dict_odgd launch (include/fasst_dict.h); returns the requested
    arrays (odgd [cols, lengthOdgd], spectrum [cols, nfft], power [nfft, cols])."""
    ncol = f1.size
    windows = np.ascontiguousarray(np.atleast_2d(windows), dtype=np.float64)
    sel = np.ascontiguousarray(window_sel, dtype=np.int32)
    toff = np.ascontiguousarray(t_offset, dtype=np.float64)
    out_o = np.empty((ncol, lengthOdgd), dtype=np.complex128) if odgd else None
    out_s = np.empty((ncol, nfft), dtype=np.complex128) if spectrum else None
    out_p = np.empty((nfft, ncol)) if power else None
    check(lib.dict_odgd(_dev(device), ncol, dptr(f1), dptr(f2), _lib.iptr(npart), pmax,
                        dptr(amps), dptr(toff), float(Fs), int(lengthOdgd), windows.shape[0],
                        dptr(windows), _lib.iptr(sel), nfft,
                        None if out_o is None else dptr(out_o),
                        None if out_s is None else dptr(out_s),
                        None if out_p is None else dptr(out_p)), "dict_odgd")
    return out_o, out_s, out_p


def _odgd_one(F1, F2, F0, partialMax, Fs, lengthOdgd, nfft, Ot, t0, window, device):
    """odgd, odgdSpectrum of one comb (F1 == F2) or chirp."""
    amps = _odgd_amplitudes(F0, Ot, partialMax)
    A = np.zeros((1, max(1, amps.size)), dtype=np.complex128)
    A[0, :amps.size] = amps
    odgd, spec, _ = _dict_odgd(device, np.array([F1], dtype=np.float64),
                               np.array([F2], dtype=np.float64),
                               np.array([amps.size], dtype=np.int32), A.shape[1], A,
                               [t0 / F0], Fs, lengthOdgd, window, [0], nfft,
                               odgd=True, spectrum=True)
    return odgd[0], spec[0]


def generate_ODGD_spec(F0, Fs, lengthOdgd=2048, Nfft=2048, Ot=0.5, t0=0.0,
                       analysisWindowType='sinebell', device=None):
    """odgd, odgdSpectrum = generate_ODGD_spec(...)  (separateLeadFunctions.py:888-949).

    The KLGLOTT88 comb of F0 over lengthOdgd samples starting at t0 / F0, and
    np.fft.fft(np.real(odgd * window), n=Nfft), both synthesised on the GPU
    (dict_odgd, include/fasst_dict.h).  analysisWindowType: 'sinebell',
    'hanning', 'rectangular' or an array of lengthOdgd values."""
    nfft = _odgd_nfft(Nfft, "generate_ODGD_spec")
    F0, Fs, Ot, t0 = np.double(F0), np.double(Fs), np.double(Ot), np.double(t0)
    lengthOdgd = int(lengthOdgd)
    window = _odgd_window(analysisWindowType, lengthOdgd, ('sinebell', 'hanning', 'rectangular'),
                          array=True)
    return _odgd_one(F0, F0, F0, np.floor((Fs / 2) / F0), Fs, lengthOdgd, nfft, Ot, t0, window,
                     device)


def generate_ODGD_spec_inharmo(F0, Fs, lengthOdgd=2048, Nfft=2048, Ot=0.5, t0=0.0,
                               analysisWindowType='sinebell', inharmonicity=0.5, device=None):
    """odgd, odgdSpectrum = generate_ODGD_spec_inharmo(...)  (:951-1008).

    The reference never reads `inharmonicity`: its body is generate_ODGD_spec
    without the array-window branch, and so is this one.  The argument is
    accepted and ignored."""
    nfft = _odgd_nfft(Nfft, "generate_ODGD_spec_inharmo")
    F0, Fs, Ot, t0 = np.double(F0), np.double(Fs), np.double(Ot), np.double(t0)
    lengthOdgd = int(lengthOdgd)
    window = _odgd_window(analysisWindowType, lengthOdgd, ('sinebell', 'hanning', 'rectangular'))
    return _odgd_one(F0, F0, F0, np.floor((Fs / 2) / F0), Fs, lengthOdgd, nfft, Ot, t0, window,
                     device)


def generate_ODGD_spec_chirped(F1, F2, Fs, lengthOdgd=2048, Nfft=2048, Ot=0.5, t0=0.0,
                               analysisWindowType='sinebell', device=None):
    """odgd, odgdSpectrum = generate_ODGD_spec_chirped(...)  (:1010-1072).

    The comb gliding from F1 to F2 over the lengthOdgd samples; F0 =
    (F1 + F2) / 2 gives the amplitudes and the start t0 / F0, max(F1, F2) the
    number of partials.  F1 == F2 is the plain comb.  analysisWindowType:
    'sinebell', 'hanning' or 'hann', 'rectangular'."""
    nfft = _odgd_nfft(Nfft, "generate_ODGD_spec_chirped")
    F1, F2 = np.double(F1), np.double(F2)
    F0 = np.double(F1 + F2) / 2.0
    Fs, Ot, t0 = np.double(Fs), np.double(Ot), np.double(t0)
    lengthOdgd = int(lengthOdgd)
    window = _odgd_window(analysisWindowType, lengthOdgd,
                          ('sinebell', 'hanning', 'hann', 'rectangular'))
    return _odgd_one(F1, F2, F0, np.floor((Fs / 2) / np.max([F1, F2])), Fs, lengthOdgd, nfft, Ot,
                     t0, window, device)


def generate_WF0_chirped(minF0, maxF0, Fs, Nfft=2048, stepNotes=4, lengthWindow=2048, Ot=0.5,
                         perF0=1, depthChirpInSemiTone=0.5, loadWF0=True,
                         analysisWindow='hanning', device=None):
    """F0Table, WF0 = generate_WF0_chirped(...)  (separateLeadFunctions.py:237-345).

    WF0[:, i * perF0] = |fft(window * Re odgd(F0_i), Nfft)|^2 and the perF0 - 1
    chirps around F0_i after it: all Nfft rows, one dict_odgd launch, only the
    power leaves the GPU.  As in the reference the comb columns use
    `analysisWindow` and the chirp columns generate_ODGD_spec_chirped's default
    'sinebell' (:335-339 pass no window).  The cache file is the reference's
    name with the wf0gpu_ prefix."""
    nfft = _odgd_nfft(Nfft, "generate_WF0_chirped")
    filename = ''.join(['wf0gpu_', '_minF0-', str(minF0), '_maxF0-', str(maxF0), '_Fs-', str(Fs),
                        '_Nfft-', str(Nfft), '_stepNotes-', str(stepNotes), '_Ot-', str(Ot),
                        '_perF0-', str(perF0), '_depthChirp-', str(depthChirpInSemiTone),
                        '_analysisWindow-', analysisWindow, '.npz'])
    if os.path.isfile(filename) and loadWF0:
        struc = np.load(filename)
        return struc['F0Table'], struc['WF0']
    lengthWindow, perF0 = int(lengthWindow), int(perF0)
    windows = np.stack([_odgd_window(analysisWindow, lengthWindow,
                                     ('sinebell', 'hanning', 'rectangular')),
                        sinebell(lengthWindow)])
    Fs = np.double(Fs)
    F0Table = _f0_table(minF0, maxF0, stepNotes)
    f1a, f2a, npart, pmax, A = _comb_columns(F0Table, Fs, Ot, perF0, depthChirpInSemiTone)
    sel = np.ones(f1a.size, dtype=np.int32)
    sel[::perF0] = 0
    WF0 = _dict_odgd(device, f1a, f2a, npart, pmax, A, np.zeros(f1a.size), Fs, lengthWindow,
                     windows, sel, nfft, power=True)[2]
    try:
        np.savez(filename, F0Table=F0Table, WF0=WF0)
    except OSError:
        pass
    return F0Table, WF0


def generate_WF0_MinQT_chirped(minF0, maxF0, cqtfmax, cqtfmin, cqtbins=48., Fs=44100., Nfft=2048,
                               stepNotes=4, lengthWindow=2048, Ot=0.5, perF0=1,
                               depthChirpInSemiTone=0.5, loadWF0=True, analysisWindow='hanning',
                               atomHopFactor=0.25, cqtWinFunc=np.hanning, verbose=False,
                               device=None):
    """F0Table, WF0, mqt = generate_WF0_MinQT_chirped(...)
    (separateLeadFunctions.py:347-521).

    Builds the MinQTransfo of :408-416 (perfRast=1) and keeps, for every comb
    of max(lengthWindow, FFTLen * 2^(octaveNr-1)) samples, the transform's
    column nearest the middle (:487): the path generate_WF0_TR_chirped takes
    for a CQT-type transform.  `analysisWindow` only enters the file name, as
    in the reference (its spectrum is computed and dropped there).  The cache
    file holds F0Table and WF0; the transform is rebuilt."""
    from ..tftransforms.minqt import MinQTransfo
    bins = int(cqtbins) if float(cqtbins) == int(cqtbins) else cqtbins
    mqt = MinQTransfo(linFTLen=Nfft, fmin=cqtfmin, fmax=cqtfmax, bins=bins, fs=Fs, perfRast=1,
                      verbose=verbose, winFunc=cqtWinFunc, atomHopFactor=atomHopFactor,
                      device=device)
    lengthWindow = int(np.maximum(lengthWindow,
                                  mqt.cqtkernel.FFTLen * (2 ** (mqt.octaveNr - 1))))
    filename = ''.join(['wf0gpu_minqt_', '_minF0-', str(minF0), '_maxF0-', str(maxF0),
                        '_cqtfmax-', str(cqtfmax), '_cqtfmin-', str(cqtfmin),
                        '_cqtbins-', str(cqtbins), '_Fs-', str(int(Fs)), '_Nfft-', str(int(Nfft)),
                        '_atomHopFactor-%.2f' % (atomHopFactor),
                        '_stepNotes-', str(int(stepNotes)), '_Ot-', str(Ot),
                        '_perF0-', str(int(perF0)), '_depthChirp-', str(depthChirpInSemiTone),
                        '_analysisWindow-', analysisWindow,
                        '_lengthWindow-%d' % lengthWindow,
                        '_cqtwinfunc-', cqtWinFunc.__name__, '.npz'])
    if os.path.isfile(filename) and loadWF0:
        struc = np.load(filename)
        return struc['F0Table'], struc['WF0'], mqt
    F0Table = _f0_table(minF0, maxF0, stepNotes)
    WF0 = _wf0_cqt(mqt, F0Table, np.double(Fs), Ot, int(perF0), depthChirpInSemiTone,
                   lengthWindow)
    try:
        np.savez(filename, F0Table=F0Table, WF0=WF0)
    except OSError:
        pass
    return F0Table, WF0, mqt


def generate_WF0_NSGTMinQT_chirped(minF0, maxF0, cqtfmax, cqtfmin, cqtbins=48., Fs=44100.,
                                   Nfft=2048, stepNotes=4, lengthWindow=2048, Ot=0.5, perF0=1,
                                   depthChirpInSemiTone=0.5, loadWF0=True,
                                   analysisWindow='hanning', atomHopFactor=0.25,
                                   cqtWinFunc=np.hanning, verbose=False):
    """The reference's function (separateLeadFunctions.py:523-694) cannot run:
    it builds its transform with `nsgt.nsgtMinQT` (:630), which the nsgt
    package does not define, so there is no result to reproduce."""
    raise NotImplementedError(
        "generate_WF0_NSGTMinQT_chirped: the reference's function cannot run "
        "(separateLeadFunctions.py:630 calls nsgt.nsgtMinQT, which is not defined), so no "
        "result exists to reproduce; use generate_WF0_MinQT_chirped")


def generateHannBasis(numberFrequencyBins, sizeOfFourier, Fs, frequencyScale='linear',
                      numberOfBasis=20, overlap=.75):
    """WGAMMA: overlapping Hann bumps along the frequency axis
    (separateLeadFunctions.py:1074-1146; a few hundred host-side numbers)."""
    if frequencyScale != 'linear':
        print("The desired feature for frequencyScale is not recognized yet...")
        return 0
    numberOfWindowsForUnit = np.ceil(1.0 / (1.0 - overlap))
    overlap = 1.0 - 1.0 / np.double(numberOfWindowsForUnit)
    lengthSineWindow = np.ceil(numberFrequencyBins / ((1.0 - overlap) * (numberOfBasis - 1) + 1 -
                                                      2.0 * overlap))
    lengthSineWindow = 2.0 * np.floor(lengthSineWindow / 2.0)
    mappingFrequency = np.arange(numberFrequencyBins)
    sizeBigWindow = 2.0 * numberFrequencyBins
    firstWindowCenter = -numberOfWindowsForUnit + 1
    lastWindowCenter = numberOfBasis - numberOfWindowsForUnit + 1
    sineCenters = np.round(np.arange(firstWindowCenter, lastWindowCenter) * (1 - overlap) *
                           np.double(lengthSineWindow) + lengthSineWindow / 2.0)
    prototypeSineWindow = np.hanning(int(lengthSineWindow))
    bigWindow = np.zeros([int(sizeBigWindow * 2), 1])
    bigWindow[int(sizeBigWindow - lengthSineWindow / 2.0):
              int(sizeBigWindow + lengthSineWindow / 2.0)] = np.vstack(prototypeSineWindow)
    WGAMMA = np.zeros([numberFrequencyBins, numberOfBasis])
    for p in np.arange(numberOfBasis):
        WGAMMA[:, p] = np.hstack(bigWindow[np.int32(mappingFrequency - sineCenters[p] +
                                                    sizeBigWindow)])
    return WGAMMA
