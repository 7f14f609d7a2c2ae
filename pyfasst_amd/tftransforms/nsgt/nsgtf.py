"""Functional form of the forward transform on given windows (one-off plan)."""
import numpy as np

from . import _device
from .util import chkM


def nsgtf(f, g, wins, nn, M=None, real=False, reducedform=0, measurefft=False):
    """Coefficients of signal f under the windows g at bins wins: for each kept
    band, the inverse DFT of length M[k] of the windowed spectrum."""
    M = chkM(M, g)
    plan = _device.DevicePlan(g, g, wins, nn, M, len(f), real, reducedform)
    c = plan.forward(np.asarray(f, dtype=np.float64)[None])[0]
    o = plan.offsets
    return [c[o[j]:o[j + 1]].copy() for j in range(len(o) - 1)]


def nsgtf_sl(*args, **kwargs):
    raise NotImplementedError("nsgtf_sl: the sliced transform is out of scope")
