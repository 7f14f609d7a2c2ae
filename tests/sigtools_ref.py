"""NumPy restatement of the reference's tools/signalTools.py (prinComp2D,
medianFilter, f0detectionFunction, invHermMat2D, sortSpectrum), the cases the
fixture tests/golden/sigtools.npz records, and the bounds of DESIGN.md §7.4.

The restatement follows the reference line by line with two differences:
prinComp2D's window sums are direct sums in ascending frame order (the
reference uses fftconvolve) and the means the reference computes and drops are
not computed.  tests/test_sigtools_ref_golden.py pins it to the fixture.
"""
import numpy as np

# ------------------------------------------------------------------- bounds
# 1e-10 (the golden yardstick) x the output's measured move
# under a 1e-15 relative input perturbation / 1.4e-15 (nmf.npz's), rounded up
# to one digit.  lambdaM, lambdam: max |diff| / max lambdaM.  vM, vm: max
# |diff| over the points whose reference den exceeds DEN_MIN x max lambdaM.
# hs: max |diff| / max |hs|.  `sensitivity()` below measures the moves.
# Measured moves: lambdaM 3.1e-15, lambdam 6.8e-16, vM 8.6e-15, vm 8.1e-15,
# hs 2.3e-15; the restatement is within 8.4e-15 of the reference everywhere.
BOUND = {'lambdaM': 3e-10, 'lambdam': 5e-11, 'vM': 7e-10, 'vm': 6e-10, 'hs': 2e-10}
DEN_MIN = 1e-3
EXCLUDED_MAX = 0.01


# -------------------------------------------------------------- restatement
def median_filter(x, length=10):
    x = np.asarray(x)
    N = x.size
    out = np.zeros_like(x)
    for n in range(N):
        w = x[max(n - length, 0):min(n + length, N - 1)]
        m = np.nan
        if w.size and not np.any(np.isnan(w)):
            s = np.sort(w)
            m = s[w.size // 2] if w.size % 2 else (s[w.size // 2 - 1] + s[w.size // 2]) / 2
        out[n] = x[n] if np.isnan(m) else m
    return out


def window_sums(a, nb):
    L = a.shape[1] - nb + 1
    s = np.zeros((a.shape[0], L), dtype=a.dtype)
    for k in range(nb):
        s += a[:, k:k + L]
    return s


def prin_comp_2d(X0, X1, neighborNb=10, with_den=False):
    if X0.shape != X1.shape:
        raise ValueError("X1 and X2 of size " + str(X0.shape) + ' and ' + str(X1.shape))
    F, N = X0.shape
    lenCov = N - neighborNb + 1
    if lenCov < 1:
        raise ValueError("negative dimensions are not allowed")
    with np.errstate(all='ignore'):
        cov0_2 = np.abs(window_sums(np.abs(X0) ** 2, neighborNb)) / (neighborNb - 1.)
        cov1_2 = np.abs(window_sums(np.abs(X1) ** 2, neighborNb)) / (neighborNb - 1.)
        cov01 = window_sums(X0 * np.conj(X1), neighborNb) / (neighborNb - 1.)
        traSig = cov0_2 + cov1_2
        detSig = cov0_2 * cov1_2 - np.abs(cov01) ** 2
        delta = np.sqrt(traSig ** 2 - 4 * detSig)
        lambdaM = .5 * (traSig + delta)
        lambdam = .5 * (traSig - delta)
        vM = np.zeros([2, F, lenCov], dtype=complex)
        vm = np.zeros([2, F, lenCov], dtype=complex)
        denM = np.sqrt(np.abs(cov01) ** 2 + np.abs(lambdaM - cov0_2) ** 2)
        vM[0] = cov01 / denM
        vM[1] = (lambdaM - cov0_2) / denM
        vM[0][denM == 0] = 1
        vM[1][denM == 0] = 0
        denm = np.sqrt(np.abs(cov01) ** 2 + np.abs(lambdam - cov0_2) ** 2)
        vm[0] = cov01 / denm
        vm[1] = (lambdam - cov0_2) / denm
        vm[0][denm == 0] = 0
        vm[1][denm == 0] = 1
    if with_den:
        return lambdaM, lambdam, vM, vm, denM, denm
    return lambdaM, lambdam, vM, vm


def inv_herm_2d(a_00, a_01, a_11):
    with np.errstate(all='ignore'):
        det = a_00 * a_11 - np.abs(a_01) ** 2
        return a_11 / det, -a_01 / det, a_00 / det


def f0_detection(TFmatrix, freqs=None, samplingrate=44100, fouriersize=2048, f0min=80,
                 f0max=3000, stepnote=16, numberHarmonics=20, threshold=0.5, detectFunc=np.sum,
                 weightFreqs=None):
    if TFmatrix.ndim == 1:
        nframes, nfreqs = 1, TFmatrix.size
    else:
        nfreqs, nframes = TFmatrix.shape
    if freqs is None:
        freqs = np.arange(nfreqs) * samplingrate / np.double(fouriersize)
    if weightFreqs is None:
        weightFreqs = np.ones(nfreqs)
    F0number = np.ceil((12. * stepnote) * np.log2(f0max / f0min))
    F0Table = f0min * (2. ** (np.arange(F0number) / (12. * stepnote)))
    TFmatrixSum = TFmatrix.sum(axis=0)
    hs = np.zeros([int(F0number), nframes])
    for nf0, f0 in enumerate(F0Table):
        rows = []
        for nh in range(1, numberHarmonics + 1):
            with np.errstate(divide='ignore'):
                sel = (np.abs(12 * np.log2(freqs / (nh * f0)))) < threshold
            if sel.sum() == 0:
                continue
            if TFmatrix.ndim == 1:
                if sel.sum() > 1:
                    raise ValueError("one-dimensional input, several bins for a harmonic")
                rows.append(weightFreqs[sel] * TFmatrix[sel])
            else:
                rows.append((np.vstack(weightFreqs[sel]) * TFmatrix[sel]).max(axis=0))
        if rows:
            hs[nf0] = detectFunc(np.vstack(rows) / TFmatrixSum, axis=0)
    return hs, F0Table


def sort_spectrum(spectrum, numberHarmonicsHS=50, numberHarmonicsHP=1, **kwargs):
    hs, f0t = f0_detection(spectrum, numberHarmonics=numberHarmonicsHS, detectFunc=np.sum, **kwargs)
    hp, _ = f0_detection(spectrum, numberHarmonics=numberHarmonicsHP, detectFunc=np.prod, **kwargs)
    f0s = f0t[np.argmax(hs * hp, axis=0)]
    indsort = np.argsort(f0s)
    return spectrum[:, indsort], f0s[indsort], hs, hp, f0t


# -------------------------------------------------------------------- cases
# name: (F, N, neighborNb, seed)
PCA_CASES = {
    'odd': (5, 37, 10, 11),
    'one_window': (3, 10, 10, 12),
    'pair': (3, 33, 2, 13),
    'chunks': (4, 700, 20, 14),
    'wide': (2, 129, 64, 15),
    'zero_row': (3, 20, 5, 16),
    'rank1': (2, 30, 6, 17),
}
PCA_TABLE = ('odd', 'one_window', 'pair', 'chunks', 'wide')
RANK1_C = 0.6 - 1.3j


def pca_inputs(name):
    """White complex noise plus one coherent source on both channels."""
    F, N, nb, seed = PCA_CASES[name]
    r = np.random.RandomState(seed)
    cn = lambda: (r.randn(F, N) + 1j * r.randn(F, N)) / np.sqrt(2.)
    s, n0, n1 = cn(), cn(), cn()
    X0 = n0 + 1.5 * s
    X1 = n1 + (0.8 - 0.9j) * s
    if name == 'zero_row':
        X0[1] = 0
        X1[1] = 0
    if name == 'rank1':
        X1 = RANK1_C * X0
    return X0, X1, nb


# name: (N, length)
MEDIAN_CASES = {
    'n1': (1, 10), 'n2': (2, 10), 'n50': (50, 10), 'len1': (20, 1), 'len_ge_n': (15, 40),
    'nan_mid': (40, 5), 'ties': (60, 7), 'n3000': (3000, 300),
}


def median_input(name):
    N, length = MEDIAN_CASES[name]
    r = np.random.RandomState(100 + N)
    x = r.randn(N)
    if name == 'nan_mid':
        x[N // 2] = np.nan
    if name == 'ties':
        x = r.randint(0, 5, N).astype(np.float64)
    return x, length


HS_GRID = dict(samplingrate=44100, fouriersize=128, f0min=300., f0max=2500., stepnote=2,
               numberHarmonics=12)
# name: (kwargs, one-dimensional input)
HS_CASES = {
    'sum': (dict(HS_GRID, detectFunc=np.sum), False),
    'prod': (dict(HS_GRID, detectFunc=np.prod), False),
    'wide_thr': (dict(HS_GRID, detectFunc=np.sum, threshold=1.5), False),
    'weights': (dict(HS_GRID, detectFunc=np.sum, threshold=1.5, weightFreqs='ramp'), False),
    'one_d': (dict(HS_GRID, detectFunc=np.sum, f0max=1200., numberHarmonics=4), True),
}
SORT_KW = dict(samplingrate=44100, fouriersize=512, f0min=300., f0max=2500., stepnote=1,
               threshold=0.5)
SORT_HS, SORT_HP = 10, 1


def hs_input(name):
    kw, one_d = HS_CASES[name]
    kw = dict(kw)
    r = np.random.RandomState(7)
    TF = np.abs(r.randn(65, 7)) + 0.05
    if kw.get('weightFreqs', None) == 'ramp':
        kw['weightFreqs'] = 0.5 + np.arange(65) / 64.
    return (TF[:, 3].copy() if one_d else TF), kw


def sort_input():
    """Seven frames, each a comb on its own F0 (distinct salience maxima)."""
    f0s = np.array([1500., 420., 980., 2100., 610., 330., 1250.])
    fr = np.arange(257) * 44100 / 512.
    S = np.full((257, 7), 1e-3)
    for t, f0 in enumerate(f0s):
        for h in range(1, 11):
            S[:, t] += np.exp(-0.5 * ((fr - h * f0) / 60.) ** 2) / h
    return S


def inv_inputs():
    r = np.random.RandomState(5)
    a01 = r.randn(3, 5) + 1j * r.randn(3, 5)
    a00 = np.abs(a01) + r.rand(3, 5) + 0.1
    a11 = np.abs(a01) + r.rand(3, 5) + 0.1
    return {'field': (a00, a01, a11), 'scalar': (2.0, 0.3 - 0.4j, 1.5),
            'real_scalar': (2.0, 0.7, 1.5)}


# -------------------------------------------------------------- comparisons
def pca_errors(got, ref, den_M, den_m):
    """The four figures BOUND limits and the shares of points left out."""
    scale = np.max(ref[0])
    keepM, keepm = den_M > DEN_MIN * scale, den_m > DEN_MIN * scale
    dv = lambda a, b, k: float(np.max(np.abs(a - b)[:, k])) if k.any() else 0.
    return {'lambdaM': float(np.max(np.abs(got[0] - ref[0])) / scale),
            'lambdam': float(np.max(np.abs(got[1] - ref[1])) / scale),
            'vM': dv(got[2], ref[2], keepM), 'vm': dv(got[3], ref[3], keepm),
            'excluded': max(1. - keepM.mean(), 1. - keepm.mean())}


def hs_error(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def sensitivity(draws=5, rel=1e-15):
    """Largest move of the restatement's outputs under a `rel` relative
    perturbation of its inputs (DESIGN.md §7.2's method), over the cases."""
    out = {k: 0. for k in BOUND}
    r = np.random.RandomState(0)
    for name in PCA_TABLE + ('rank1',):
        X0, X1, nb = pca_inputs(name)
        ref = prin_comp_2d(X0, X1, nb, with_den=True)
        for _ in range(draws):
            p = lambda X: X * (1 + rel * r.randn(*X.shape))
            e = pca_errors(prin_comp_2d(p(X0), p(X1), nb), ref[:4], ref[4], ref[5])
            for k in ('lambdaM', 'lambdam', 'vM', 'vm'):
                out[k] = max(out[k], e[k])
    for name in HS_CASES:
        TF, kw = hs_input(name)
        ref = f0_detection(TF, **kw)[0]
        for _ in range(draws):
            got = f0_detection(TF * (1 + rel * r.randn(*TF.shape)), **kw)[0]
            out['hs'] = max(out['hs'], hs_error(got, ref))
    return out


if __name__ == "__main__":
    print(sensitivity())
