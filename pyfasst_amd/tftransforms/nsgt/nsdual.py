"""Canonical dual windows of a painless non-stationary Gabor frame (host
NumPy, FP64).

When every band has at least as many time channels as its window has points,
the frame operator is diagonal in the frequency domain: bin b carries
S[b] = sum over the bands covering b of M[k] g_k[b]^2.  The dual window is
then g_k / S under the window.  Windows are stored in FFT order (peak first),
the bins under them in ascending order, hence the fftshift pair.
"""
import numpy as np

from .util import chkM


def nsdual(g, wins, nn, M=None):
    M = chkM(M, g)
    diag = np.zeros(nn)
    for k, bins in enumerate(wins):
        diag[bins] += np.fft.fftshift(g[k]) ** 2 * M[k]
    return [g[k] / np.fft.ifftshift(diag[bins]) for k, bins in enumerate(wins)]
