"""NumPy restatement of the ODGD / WF0 dictionary family of
SeparateLeadStereo/separateLeadFunctions.py, and the cases its tests share.

TEST INFRASTRUCTURE ONLY (the checker, never the product).

  generate_ODGD_spec           :888-949    KLGLOTT88 comb of one F0 and the
                                           FFT of its windowed real part
  generate_ODGD_spec_inharmo   :951-1008   the same body (`inharmonicity` is
                                           never read), no array window
  generate_ODGD_spec_chirped   :1010-1072  the comb gliding from F1 to F2
  generate_WF0_chirped         :237-345    WF0 = |odgdSpectrum|^2 per F0 and
                                           chirp, all Nfft rows
  generate_WF0_MinQT_chirped   :347-521    WF0 on a MinQT transform (through
                                           oracle/cqt_ref.py and dict_ref.py)

Pinned against the reference's own numbers (tests/golden/dict_family.npz,
written by tests/golden/make_golden_dict_family.py) by
tests/test_dict_family_ref_golden.py.

`odgd_longdouble` / `spectrum_longdouble` evaluate the same expressions in
np.longdouble (the inputs, np.pi included, are the float64 values): the
yardstick of the float64 evaluation error, DESIGN.md section 7.10.
"""
import numpy as np


def sinebell(lengthWindow):
    """utils.py:41-53"""
    return np.sin((np.pi * (np.arange(lengthWindow))) / (1.0 * lengthWindow))


def hann(args):
    """utils.py:55-61"""
    return np.hanning(args)


def _window(analysisWindowType, lengthOdgd, names, array):
    if isinstance(analysisWindowType, str):
        if analysisWindowType == 'sinebell' and 'sinebell' in names:
            return sinebell(lengthOdgd)
        if analysisWindowType in ('hanning', 'hann') and analysisWindowType in names:
            return hann(lengthOdgd)
        if analysisWindowType == 'rectangular' and 'rectangular' in names:
            return np.ones(lengthOdgd)
    elif array and len(analysisWindowType) == lengthOdgd:
        return analysisWindowType
    raise ValueError("Analysis window not understood.")


def odgd_amplitudes(F0, Ot, partialMax):
    """:918-933"""
    frequency_numbers = np.arange(1, partialMax + 1)
    temp_array = 1j * 2.0 * np.pi * frequency_numbers * Ot
    amplitudes = F0 * 27 / 4 \
        * (np.exp(-temp_array)
           + (2 * (1 + 2 * np.exp(-temp_array)) / temp_array)
           - (6 * (1 - np.exp(-temp_array))
              / (temp_array ** 2))) \
        / temp_array
    return frequency_numbers, amplitudes


def generate_ODGD_spec(F0, Fs, lengthOdgd=2048, Nfft=2048, Ot=0.5, t0=0.0,
                       analysisWindowType='sinebell', _array=True):
    """:888-949"""
    F0 = np.double(F0)
    Fs = np.double(Fs)
    Ot = np.double(Ot)
    t0 = np.double(t0)
    analysisWindow = _window(analysisWindowType, lengthOdgd,
                             ('sinebell', 'hanning', 'rectangular'), _array)
    partialMax = np.floor((Fs / 2) / F0)
    frequency_numbers, amplitudes = odgd_amplitudes(F0, Ot, partialMax)
    timeStamps = np.arange(lengthOdgd) / Fs + t0 / F0
    odgd = np.exp(np.outer(2.0 * 1j * np.pi * F0 * frequency_numbers,
                           timeStamps)) \
        * np.outer(amplitudes, np.ones(lengthOdgd))
    odgd = np.sum(odgd, axis=0)
    odgdSpectrum = np.fft.fft(np.real(odgd * analysisWindow), n=Nfft)
    return odgd, odgdSpectrum


def generate_ODGD_spec_inharmo(F0, Fs, lengthOdgd=2048, Nfft=2048, Ot=0.5, t0=0.0,
                               analysisWindowType='sinebell', inharmonicity=0.5):
    """:951-1008 (`inharmonicity` is not read there either)"""
    return generate_ODGD_spec(F0, Fs, lengthOdgd=lengthOdgd, Nfft=Nfft, Ot=Ot, t0=t0,
                              analysisWindowType=analysisWindowType, _array=False)


def generate_ODGD_spec_chirped(F1, F2, Fs, lengthOdgd=2048, Nfft=2048, Ot=0.5, t0=0.0,
                               analysisWindowType='sinebell'):
    """:1010-1072"""
    F1 = np.double(F1)
    F2 = np.double(F2)
    F0 = np.double(F1 + F2) / 2.0
    Fs = np.double(Fs)
    Ot = np.double(Ot)
    t0 = np.double(t0)
    analysisWindow = _window(analysisWindowType, lengthOdgd,
                             ('sinebell', 'hanning', 'hann', 'rectangular'), False)
    partialMax = np.floor((Fs / 2) / np.max([F1, F2]))
    frequency_numbers, amplitudes = odgd_amplitudes(F0, Ot, partialMax)
    timeStamps = np.arange(lengthOdgd) / Fs + t0 / F0
    odgd = np.exp(2.0 * 1j * np.pi
                  * (np.outer(F1 * frequency_numbers, timeStamps)
                     + np.outer((F2 - F1)
                                * frequency_numbers, timeStamps ** 2)
                     / (2 * lengthOdgd / Fs))) \
        * np.outer(amplitudes, np.ones(lengthOdgd))
    odgd = np.sum(odgd, axis=0)
    odgdSpectrum = np.fft.fft(np.real(odgd * analysisWindow), n=Nfft)
    return odgd, odgdSpectrum


def f0_table(minF0, maxF0, stepNotes):
    """:307-315"""
    minF0 = np.double(minF0)
    maxF0 = np.double(maxF0)
    stepNotes = np.double(stepNotes)
    numberOfF0 = np.ceil(12.0 * stepNotes * np.log2(maxF0 / minF0)) + 1
    return minF0 * (2 ** (np.arange(numberOfF0, dtype=np.double) / (12 * stepNotes)))


def generate_WF0_chirped(minF0, maxF0, Fs, Nfft=2048, stepNotes=4, lengthWindow=2048, Ot=0.5,
                         perF0=1, depthChirpInSemiTone=0.5, analysisWindow='hanning'):
    """:237-345 without the cache file.  The chirps are generated without a
    window argument (:335-339): 'sinebell', whatever analysisWindow says."""
    Fs = np.double(Fs)
    F0Table = f0_table(minF0, maxF0, stepNotes)
    numberOfF0 = F0Table.size
    numberElementsInWF0 = numberOfF0 * perF0
    WF0 = np.zeros([Nfft, numberElementsInWF0], dtype=np.double)
    for fundamentalFrequency in np.arange(numberOfF0):
        odgd, odgdSpec = generate_ODGD_spec(F0Table[fundamentalFrequency], Fs,
                                            Ot=Ot, lengthOdgd=lengthWindow,
                                            Nfft=Nfft, t0=0.0,
                                            analysisWindowType=analysisWindow)
        WF0[:, fundamentalFrequency * perF0] = np.abs(odgdSpec) ** 2
        for chirpNumber in np.arange(perF0 - 1):
            F2 = F0Table[fundamentalFrequency] \
                * (2 ** ((chirpNumber + 1.0) * depthChirpInSemiTone
                         / (12.0 * (perF0 - 1.0))))
            F1 = 2.0 * F0Table[fundamentalFrequency] - F2
            odgd, odgdSpec = generate_ODGD_spec_chirped(F1, F2, Fs,
                                                        Ot=Ot,
                                                        lengthOdgd=lengthWindow,
                                                        Nfft=Nfft, t0=0.0)
            WF0[:, fundamentalFrequency * perF0 + chirpNumber + 1] = np.abs(odgdSpec) ** 2
    return F0Table, WF0


def generate_WF0_MinQT_chirped(minF0, maxF0, cqtfmax, cqtfmin, cqtbins=48., Fs=44100., Nfft=2048,
                               stepNotes=4, lengthWindow=2048, Ot=0.5, perF0=1,
                               depthChirpInSemiTone=0.5, atomHopFactor=0.25, cqtWinFunc=np.hanning):
    """:347-521 without the cache file: the MinQTransfo of :408-416 (the
    oracle's cqt_ref.RefCQT), lengthWindow raised to the transform's largest
    block (:420-422), every comb through the transform and the column nearest
    the middle kept (:485-489)."""
    import cqt_ref
    import dict_ref
    t = cqt_ref.RefCQT('mqt', fmin=cqtfmin, fmax=cqtfmax, bins=cqtbins, fs=Fs, linFTLen=Nfft,
                       atomHopFactor=atomHopFactor, winFunc=cqtWinFunc)
    maxBlock = int(t.k.FFTLen * (2 ** (t.octaveNr - 1)))
    if lengthWindow > maxBlock:
        raise NotImplementedError("restated for lengthWindow <= the transform's largest block")
    F0Table, WF0 = dict_ref.generate_wf0_tr_chirped_cqt(t, minF0, maxF0, stepNotes=stepNotes, Ot=Ot,
                                                        perF0=perF0,
                                                        depthChirpInSemiTone=depthChirpInSemiTone)
    return F0Table, WF0, t


# ------------------------------------------------------------------- cases
# generate_ODGD_spec / _inharmo: name -> (function, kwargs).  lengthOdgd / Nfft
# cropped (129 / 64), zero-padded (129 / 256), equal (128 / 128), the largest
# Nfft, the smallest; one, zero and 565 partials; t0 = 0 and 0.37; every window.
def _array_window(n):
    return 0.25 + np.hanning(n + 2)[1:-1] ** 2


ODGD_CASES = {
    'crop': ('spec', dict(F0=220., Fs=8000., lengthOdgd=129, Nfft=64, Ot=0.5, t0=0.0,
                          analysisWindowType='sinebell')),
    'pad_t0': ('spec', dict(F0=220., Fs=8000., lengthOdgd=129, Nfft=256, Ot=0.5, t0=0.37,
                            analysisWindowType='hanning')),
    'equal': ('spec', dict(F0=317.3, Fs=8000., lengthOdgd=128, Nfft=128, Ot=0.3, t0=0.0,
                           analysisWindowType='rectangular')),
    'nfft8192': ('spec', dict(F0=1000., Fs=44100., lengthOdgd=300, Nfft=8192, Ot=0.5, t0=0.37,
                              analysisWindowType='sinebell')),
    'nfft2': ('spec', dict(F0=220., Fs=8000., lengthOdgd=129, Nfft=2, Ot=0.5, t0=0.0,
                           analysisWindowType='sinebell')),
    'one_partial': ('spec', dict(F0=0.3 * 8000., Fs=8000., lengthOdgd=129, Nfft=256, Ot=0.5,
                                 t0=0.37, analysisWindowType='sinebell')),
    'zero_partials': ('spec', dict(F0=0.6 * 8000., Fs=8000., lengthOdgd=129, Nfft=256, Ot=0.5,
                                   t0=0.0, analysisWindowType='sinebell')),
    'many_partials': ('spec', dict(F0=39., Fs=44100., lengthOdgd=129, Nfft=256, Ot=0.5, t0=0.37,
                                   analysisWindowType='hanning')),
    'array_window': ('spec', dict(F0=220., Fs=8000., lengthOdgd=129, Nfft=256, Ot=0.5, t0=0.0,
                                  analysisWindowType=_array_window(129))),
    'inharmo': ('inharmo', dict(F0=220., Fs=8000., lengthOdgd=129, Nfft=64, Ot=0.5, t0=0.37,
                                analysisWindowType='hanning', inharmonicity=0.2)),
}

# generate_ODGD_spec_chirped: F1 < F2, F1 > F2, F1 == F2
CHIRP_CASES = {
    'up': dict(F1=210., F2=233., Fs=8000., lengthOdgd=129, Nfft=256, Ot=0.5, t0=0.0,
               analysisWindowType='sinebell'),
    'down_t0': dict(F1=233., F2=210., Fs=8000., lengthOdgd=129, Nfft=64, Ot=0.5, t0=0.37,
                    analysisWindowType='hann'),
    'flat': dict(F1=220., F2=220., Fs=8000., lengthOdgd=128, Nfft=128, Ot=0.5, t0=0.37,
                 analysisWindowType='hanning'),
    'many_partials': dict(F1=38., F2=40., Fs=44100., lengthOdgd=129, Nfft=256, Ot=0.5, t0=0.37,
                          analysisWindowType='rectangular'),
}

# generate_WF0_chirped: 7 F0s x 3 (21 columns, two windows interleaved), the
# same with one window for all, and a single column
WF0_CASES = {
    'mixed': dict(minF0=200, maxF0=280, Fs=8000, Nfft=256, stepNotes=1, lengthWindow=200, Ot=0.5,
                  perF0=3, depthChirpInSemiTone=0.5, analysisWindow='hanning'),
    'sinebell': dict(minF0=200, maxF0=280, Fs=8000, Nfft=256, stepNotes=1, lengthWindow=200,
                     Ot=0.5, perF0=3, depthChirpInSemiTone=0.5, analysisWindow='sinebell'),
    'single': dict(minF0=300, maxF0=300, Fs=8000, Nfft=256, stepNotes=4, lengthWindow=200, Ot=0.5,
                   perF0=1, depthChirpInSemiTone=0.5, analysisWindow='hanning'),
}


def run_odgd_case(name, mod=None):
    """odgd, odgdSpectrum of ODGD_CASES[name] by `mod` (default: this restatement)."""
    mod = mod or _THIS
    fn, kw = ODGD_CASES[name]
    return (mod.generate_ODGD_spec if fn == 'spec' else mod.generate_ODGD_spec_inharmo)(**kw)


def run_chirp_case(name, mod=None):
    return (mod or _THIS).generate_ODGD_spec_chirped(**CHIRP_CASES[name])


# ---------------------------------------------------------- the yardstick
def odgd_longdouble(F1, F2, Fs, lengthOdgd, Ot, t0, chirp):
    """The waveform of the comb (chirp False: :941-944) or the chirp (:1061-1067)
    with phase, exponential and sum in np.longdouble.  F0, amplitudes, time
    stamps and np.pi are the float64 values the float64 code starts from."""
    ld = np.longdouble
    F1, F2, Fs, Ot, t0 = np.double(F1), np.double(F2), np.double(Fs), np.double(Ot), np.double(t0)
    F0 = np.double(F1 + F2) / 2.0 if chirp else F1
    partialMax = np.floor((Fs / 2) / (np.max([F1, F2]) if chirp else F0))
    frequency_numbers, amplitudes = odgd_amplitudes(F0, Ot, partialMax)
    timeStamps = (np.arange(lengthOdgd) / Fs + t0 / F0).astype(ld)
    h = frequency_numbers.astype(ld)
    two_pi = ld(2.0) * ld(np.pi)
    if chirp:
        theta = two_pi * (np.outer(ld(F1) * h, timeStamps)
                          + np.outer(ld(F2 - F1) * h, timeStamps ** 2)
                          / (ld(2 * lengthOdgd) / ld(Fs)))
    else:
        theta = np.outer(two_pi * ld(F0) * h, timeStamps)
    a_re, a_im = amplitudes.real.astype(ld)[:, None], amplitudes.imag.astype(ld)[:, None]
    c, s = np.cos(theta), np.sin(theta)
    return np.sum(c * a_re - s * a_im, axis=0), np.sum(c * a_im + s * a_re, axis=0)


def spectrum_longdouble(x, Nfft):
    """The DFT of the real longdouble signal x (cropped or zero-padded to
    Nfft), summed directly in np.longdouble; returns (real, imag)."""
    ld = np.longdouble
    x = np.asarray(x, dtype=ld)[:Nfft]
    m = np.arange(Nfft)
    pi_ld = ld(4) * np.arctan(ld(1))
    ang = ld(2) * pi_ld * m.astype(ld) / ld(Nfft)
    cw, sw = np.cos(ang), np.sin(ang)
    kn = np.outer(m, np.arange(x.size)) % Nfft
    return cw[kn].dot(x), -(sw[kn].dot(x))


def float64_deviation():
    """Largest deviation of the float64 restatement from its np.longdouble
    evaluation over ODGD_CASES and CHIRP_CASES, relative to each column's
    largest magnitude: (waveform, spectrum)."""
    dev_w = dev_s = 0.0
    runs = []
    for name in sorted(ODGD_CASES):
        kw = ODGD_CASES[name][1]
        runs.append((run_odgd_case(name), kw['F0'], kw['F0'], False, kw,
                     ('sinebell', 'hanning', 'rectangular'), True))
    for name in sorted(CHIRP_CASES):
        kw = CHIRP_CASES[name]
        runs.append((run_chirp_case(name), kw['F1'], kw['F2'], True, kw,
                     ('sinebell', 'hanning', 'hann', 'rectangular'), False))
    for (odgd, spec), F1, F2, chirp, kw, names, array in runs:
        re, im = odgd_longdouble(F1, F2, kw['Fs'], kw['lengthOdgd'], kw['Ot'], kw['t0'], chirp)
        peak = float(np.max(np.hypot(re, im))) if re.size else 0.0
        if peak > 0:
            dev_w = max(dev_w, float(np.max(np.hypot(odgd.real - re, odgd.imag - im))) / peak)
        win = np.asarray(_window(kw['analysisWindowType'], kw['lengthOdgd'], names, array))
        sre, sim = spectrum_longdouble(re * win.astype(np.longdouble), kw['Nfft'])
        peak = float(np.max(np.hypot(sre, sim)))
        if peak > 0:
            dev_s = max(dev_s, float(np.max(np.hypot(spec.real - sre, spec.imag - sim))) / peak)
    return dev_w, dev_s


# Bounds of the complex waveform and the complex spectrum against this
# restatement and the golden file, relative to each column's largest magnitude:
# ten times float64_deviation() as measured (the factor
# ten covers another summation order and another sincos).  Pinned to the
# measurement by tests/test_dict_family_ref_golden.py.
MEASURED_WAVEFORM_DEVIATION = 1.91e-14   # 1.9023e-14 with an 80-bit np.longdouble
MEASURED_SPECTRUM_DEVIATION = 6.03e-15   # 6.0221e-15
WAVEFORM_BOUND = 10 * MEASURED_WAVEFORM_DEVIATION
SPECTRUM_BOUND = 10 * MEASURED_SPECTRUM_DEVIATION
# |spectrum|^2 columns: the bound of dict_wf0_stft against tests/golden/wf0.npz
# (tests/test_gpu_dict.py), the same synthesis and transform
POWER_BOUND = 1e-10


def colrel(a, b):
    """max |a - b| over the largest magnitude of b (1 where b is all zero)."""
    a, b = np.asarray(a), np.asarray(b)
    den = float(np.max(np.abs(b))) if b.size else 0.0
    return float(np.max(np.abs(a - b))) / (den if den > 0 else 1.0) if b.size else 0.0


import sys  # noqa: E402
_THIS = sys.modules[__name__]
