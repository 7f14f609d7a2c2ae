"""Window and index helpers of the NSGT planner (host NumPy, FP64).  The
function names are the reference package's; the code is this project's."""
import numpy as np


def hannwin(l):
    """Hann window of l points in FFT order: w[n] = (1 + cos(2 pi n / l)) / 2,
    so the peak is at n = 0 and the window wraps around the end."""
    phase = np.arange(l, dtype=float) * (2. * np.pi / l)
    return (np.cos(phase) + 1.) * 0.5


def blackharr(n):
    """Blackman-Harris window of n points in FFT order (the 4-term window with
    coefficients 0.35872, 0.48832, 0.14128, 0.01168 over a period of n rounded
    down to even): the peak is at index 0, the second half wraps to the front."""
    period = (n // 2) * 2
    k = np.arange(n)
    w = (0.35872 - 0.48832 * np.cos(k * (2 * np.pi / period))
         + 0.14128 * np.cos(k * (4 * np.pi / period))
         - 0.01168 * np.cos(k * (6 * np.pi / period)))
    half = (n + 1) // 2
    return np.concatenate((w[n - half:], w[:n - half]))


def chkM(M, g):
    """Time channels per band as an array: the window lengths when M is None,
    one number repeated for every band, or the given sequence."""
    if M is None:
        return np.fromiter((len(w) for w in g), dtype=int, count=len(g))
    if np.ndim(M) == 0:
        return np.full(len(g), M)
    return M


def calcwinrange(g, rfbas, Ls):
    """Which spectrum bins each window covers.

    Band k is centred on bin rfbas[k] - rfbas[0].  The bands tile a circle of
    nn bins: from the first centre round to the last, plus the step that
    brings the last band back to the first, (-rfbas[-1]) mod Ls.  Window k of
    Lg points covers centre - Lg//2 ... centre + Lg - Lg//2 - 1, taken mod nn.
    Returns (list of index vectors, nn).
    """
    rfbas = np.asarray(rfbas)
    centres = rfbas - rfbas[0]
    nn = centres[-1] + np.mod(-rfbas[-1], Ls)
    wins = []
    for w, c in zip(g, centres):
        first = c - len(w) // 2
        wins.append(np.arange(first, first + len(w), dtype=int) % nn)
    return wins, nn
