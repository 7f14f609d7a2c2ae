"""NumPy restatement of the non-sliced NSGT (test infrastructure only): the
planning (scales, Hann windows, window positions, canonical duals), the
forward transform and the inverse, on numpy.fft.  tests/golden/nsgt_*.npz pins
it to the reference; the GPU tests compare the device against it live.
"""
import warnings

import numpy as np

# case -> what to build; mirrors tests/golden/make_golden_nsgt.py
OCT = dict(kind="oct", fmin=50, fmax=4000, bins=12, fs=8000)
CASES = {
    "prime": dict(OCT, Ls=1009, real=True),
    "even": dict(OCT, Ls=3000, real=False),
    "pow2": dict(OCT, Ls=4096, real=True),
    "wideband": dict(kind="oct", fmin=50, fmax=3000, bins=12, fs=44100, Ls=12000, real=True),
    "matrix0": dict(OCT, Ls=3000, real=True, matrixform=True, reducedform=0),
    "matrix1": dict(OCT, Ls=3000, real=True, matrixform=True, reducedform=1),
    "matrix2": dict(OCT, Ls=3000, real=True, matrixform=True, reducedform=2),
    "stereo": dict(OCT, Ls=1009, real=True, nch=2),
    "melscale": dict(kind="mel", fmin=100, fmax=3500, bnds=24, fs=8000, Ls=3000, real=True),
}


def signal(name):
    c = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    x = rs.randn(c.get("nch", 1), c["Ls"])
    return x if "nch" in c else x[0]


# ------------------------------------------------------------------- scales
def oct_scale(fmin, fmax, bpo):
    bnds = int(np.ceil(np.log2(float(fmax) / fmin) * bpo)) + 1
    r = 2 ** (1. / int(bpo))
    q = np.sqrt(r) / (r - 1.) / 2.
    f = np.array([float(fmin) * r ** b for b in range(bnds)], dtype=float)
    return f, np.array([q] * bnds, dtype=float)


def mel_scale(fmin, fmax, bnds):
    to_mel = lambda f: np.log10(f / 700. + 1.) * 2595.
    to_hz = lambda m: (np.power(10., m / 2595.) - 1.) * 700.
    m0, m1 = to_mel(float(fmin)), to_mel(float(fmax))
    step = (m1 - m0) / (bnds - 1)
    F = lambda b: to_hz(b * step + m0)
    d = 1.e-8
    f = np.array([F(b) for b in range(bnds)], dtype=float)
    q = np.array([F(b) * d / (F(b + d) - F(b - d)) for b in range(bnds)], dtype=float)
    return f, q


def scale_of(c):
    if c["kind"] == "oct":
        return oct_scale(c["fmin"], c["fmax"], c["bins"])
    return mel_scale(c["fmin"], c["fmax"], c["bnds"])


# ----------------------------------------------------------------- planning
def hann(l):
    return (np.cos(np.arange(l, dtype=float) * (np.pi * 2. / l)) + 1.) * 0.5


def q_too_high(f, q, sr, Ls):
    """Frequencies the planner warns about (Q above f Ls / (8 sr))."""
    nf = sr / 2.
    keep = (f > 0) & (f < nf)
    return f[keep][q[keep] >= f[keep] * (Ls / (8. * sr))]


def windows(f, q, sr, Ls, min_win=4):
    """g, rfbas, M of the non-sliced planner."""
    nf = sr / 2.
    lim = np.argmax(f > 0)
    if lim != 0:
        f, q = f[lim:], q[lim:]
    lim = np.argmax(f >= nf)
    if lim != 0:
        f, q = f[:lim], q[:lim]
    lbas = len(f)
    frqs = np.concatenate(((0.,), f, (nf,)))
    fbas = np.concatenate((frqs, sr - frqs[-2:0:-1]))
    fbas *= float(Ls) / sr
    M = np.zeros(fbas.shape, int)
    M[0] = np.round(2 * fbas[1])
    M[1:2 * lbas + 1] = np.round(fbas[2:2 * lbas + 2] - fbas[0:2 * lbas])
    M[-1] = np.round(Ls - fbas[-2])
    M = np.maximum(M, min_win)
    g = [hann(m) for m in M]
    fbas[lbas] = (fbas[lbas - 1] + fbas[lbas + 1]) / 2
    fbas[lbas + 2] = Ls - fbas[lbas]
    return g, np.round(fbas).astype(int), M


def win_ranges(g, rfbas, Ls):
    shift = np.concatenate(((np.mod(-rfbas[-1], Ls),), np.diff(rfbas)))
    pos = np.cumsum(shift)
    nn = int(pos[-1])
    pos = pos - shift[0]
    return [np.arange(-(len(gi) // 2) + p, len(gi) - (len(gi) // 2) + p, dtype=int) % nn
            for gi, p in zip(g, pos)], nn


def duals(g, wins, nn, M):
    diag = np.zeros(nn)
    for gi, m, w in zip(g, M, wins):
        sq = np.square(np.fft.fftshift(gi))
        sq *= m
        diag[w] += sq
    return [gi / np.fft.ifftshift(diag[w]) for gi, w in zip(g, wins)]


class Plan(object):
    def __init__(self, f, q, fs, Ls, real=True, matrixform=False, reducedform=0):
        self.Ls, self.real, self.reducedform = Ls, real, reducedform
        self.g, self.rfbas, self.M = windows(f, q, fs, Ls)
        if matrixform:
            nb = len(self.M)
            self.M[:] = (self.M[reducedform:nb // 2 + 1 - reducedform] if reducedform
                         else self.M).max()
        self.wins, self.nn = win_ranges(self.g, self.rfbas, Ls)
        self.gd = duals(self.g, self.wins, self.nn, self.M)

    @property
    def used(self):
        nb = len(self.g)
        return slice(self.reducedform, nb // 2 + 1 - self.reducedform) if self.real else slice(0, nb)

    # nsgtf: window the spectrum, fold to M points, inverse DFT
    def forward(self, s):
        ft = np.fft.fft(s)
        if self.nn > len(ft):
            ft = np.concatenate((ft, np.zeros(self.nn - len(ft), dtype=ft.dtype)))
        out = []
        for m, gi, w in zip(self.M[self.used], self.g[self.used], self.wins[self.used]):
            Lg = len(gi)
            col = -(-Lg // m)
            temp = np.zeros(col * m, dtype=complex)
            ftw = ft[w]
            temp[:(Lg + 1) // 2] = gi[:(Lg + 1) // 2] * ftw[Lg // 2:]
            temp[col * m - Lg // 2:] = gi[Lg - Lg // 2:] * ftw[:Lg // 2]
            if col > 1:
                temp = np.sum(temp.reshape((m, -1)), axis=1)
            out.append(np.fft.ifft(temp))
        return out

    # nsigtf: DFT of each band, dual window, overlap-add, inverse FFT
    def backward(self, c):
        nb = len(self.gd)
        fc = [np.fft.fft(ci) for ci in c]
        if self.real:
            assert len(c) == nb // 2 + 1 - 2 * self.reducedform
            r = self.reducedform
            mirror = lambda x: np.hstack((x[0], x[-1:0:-1])).conj()
            fc = fc + [mirror(x) for x in (fc[::-1] if r else fc[-2:0:-1])]
            bands = list(range(r, nb // 2 + 1 - r)) + list(range(nb // 2 + (r or 1),
                                                                nb + 1 - (r or 1)))
        else:
            bands = list(range(nb))
        assert len(bands) == len(fc)
        fr = np.zeros(self.nn, dtype=complex)
        for t, k in zip(fc, bands):
            gdi, w = self.gd[k], self.wins[k]
            Lg = len(gdi)
            temp = np.zeros(Lg, dtype=complex)
            temp[:(Lg + 1) // 2] = t[:(Lg + 1) // 2]
            temp[Lg - Lg // 2:] = t[len(t) - Lg // 2:]
            temp *= gdi
            temp *= len(t)
            fr[w[:Lg // 2]] += temp[Lg - Lg // 2:]
            fr[w[Lg - (Lg + 1) // 2:]] += temp[:(Lg + 1) // 2]
        if self.real:
            sig = np.fft.irfft(fr[:self.nn // 2 + 1], n=self.nn)
        else:
            sig = np.fft.ifft(fr)
        return sig[:self.Ls]


def plan_of(name):
    c = CASES[name]
    f, q = scale_of(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Plan(f, q, c["fs"], c["Ls"], real=c["real"], matrixform=c.get("matrixform", False),
                    reducedform=c.get("reducedform", 0))


def folded_plan():
    """The plan of `even` with fewer time channels than window points in every
    band of 8 points or more, M = 3 Lg // 4 (so Lg/2 <= M < Lg): the forward
    transform folds two columns, the inverse's two slices of a band overlap.
    Not a frame any more; only parity between implementations is meant."""
    p = plan_of("even")
    Lg = np.array([len(gi) for gi in p.g])
    p.M = np.where(Lg >= 8, (3 * Lg) // 4, Lg)
    p.gd = duals(p.g, p.wins, p.nn, p.M)
    return p
