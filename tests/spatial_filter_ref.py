"""NumPy restatement of the reference's time-invariant spatial filter and
GCC-PHAT (test infrastructure only), in the reference's order of operations,
and the loader of the tests/golden/spatial_<case>*.npz fixtures."""
import glob
import os

import numpy as np

eps = 1e-10   # tools/signalTools.py:11
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("spatial_conv", "spatial_conv_j1", "spatial_mqt")


def covariances(params):
    """R_n of each 'conv' component, params[n] = [rank, 2, F] (audioModel.py:974-981)."""
    d0 = np.array([(np.abs(p[:, 0]) ** 2).sum(axis=0) for p in params])
    d1 = np.array([(np.abs(p[:, 1]) ** 2).sum(axis=0) for p in params])
    off = np.array([(p[:, 0] * np.conj(p[:, 1])).sum(axis=0) for p in params])
    return d0, d1, off


def gains(params, normalise=True):
    """WG [J, 2, 2, F] (audioModel.py:983-1004)."""
    d0, d1, off = covariances(params)
    a0, a1, ao = np.mean(d0, axis=0), np.mean(d1, axis=0), np.mean(off, axis=0)
    det = a0 * a1 - np.abs(ao) ** 2                     # tools/signalTools.py:182-194
    det = np.sign(det + eps) * np.maximum(np.abs(det), eps)
    i0, i1, io = a1 / det, a0 / det, -ao / det
    WG = np.zeros([len(params), 2, 2, d0.shape[1]], dtype=complex)
    for n in range(len(params)):                        # audioModel.py:1453-1465
        WG[n, 0, 0] = off[n] * np.conj(io)
        WG[n, 1, 1] = np.conj(WG[n, 0, 0])
        WG[n, 0, 0] += d0[n] * i0
        WG[n, 1, 1] += d1[n] * i1
        WG[n, 0, 1] = d0[n] * io + off[n] * i1
        WG[n, 1, 0] = np.conj(off[n]) * i0 + d1[n] * np.conj(io)
        if normalise:                                   # audioModel.py:1003-1004
            WG[n] /= [[np.real(WG[n, 0, 0] + WG[n, 1, 1])]]
    return WG


def images(WG, X):
    """S [J, 2, F, T] = sum_c2 WG[n, c, c2] X[c2] (audioModel.py:1022-1029)."""
    S = np.zeros((WG.shape[0], 2) + X[0].shape, dtype=complex)
    for n in range(WG.shape[0]):
        for c in range(2):
            for c2 in range(2):
                S[n, c] += np.vstack(WG[n, c, c2]) * X[c2]
    return S


def gcc_phat(Cx01, nfft):
    """audioModel.py:1322-1324"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.fft.irfft(Cx01 / np.abs(Cx01), n=nfft, axis=0)


def cond_max(params):
    """max over the bins of cond(R_aa(f))."""
    d0, d1, off = covariances(params)
    a0, a1, ao = d0.mean(axis=0), d1.mean(axis=0), off.mean(axis=0)
    R = np.array([[a0, ao], [np.conj(ao), a1]]).transpose(2, 0, 1)
    return float(np.max(np.linalg.cond(R)))


def load_fixture(case):
    """One case's arrays, merged over spatial_<case>.npz and its .part<k> files."""
    g = {}
    for fn in [os.path.join(GOLDEN, case + ".npz")] + \
            sorted(glob.glob(os.path.join(GOLDEN, case + ".part*.npz"))):
        with np.load(fn) as z:
            g.update({k: z[k] for k in z.files})
    J = sum(k.startswith('params_') for k in g)
    g['params'] = [g['params_%d' % j] for j in range(J)]
    g['images'] = np.array([g['images_%d' % j] for j in range(J)])
    return g
