"""Functional form of the inverse transform on given dual windows (one-off plan)."""
import numpy as np

from . import _device


def nsigtf(c, gd, wins, nn, Ls=None, real=False, reducedform=0, measurefft=False):
    """Signal of length Ls from the coefficient bands c: DFT of each band, dual
    window, overlap-add at wins, one inverse FFT of length nn."""
    Ls = nn if Ls is None else Ls
    nb = len(gd)
    M = np.zeros(nb, dtype=int)
    sl = _device.band_slice(nb, real, reducedform)
    M[sl] = [len(ci) for ci in c]
    if real:   # the mirrored bands borrow the lengths of their sources
        for k in range(nb // 2 + 1, nb):
            M[k] = M[nb - k]
    M = np.maximum(M, 1)
    plan = _device.DevicePlan(gd, gd, wins, nn, M, Ls, real, reducedform)
    buf = np.concatenate([np.asarray(ci, dtype=np.complex128) for ci in c])[None]
    return plan.backward(buf)[0]


def nsigtf_sl(*args, **kwargs):
    raise NotImplementedError("nsigtf_sl: the sliced transform is out of scope")
