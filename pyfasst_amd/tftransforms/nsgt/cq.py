"""NSGT / CQ_NSGT: the non-stationary Gabor transform of a whole signal,
planned on the host (windows, positions, dual windows: vectors of a few
hundred entries) and computed on the GPU (include/fasst_nsgt.h).

forward(s) returns the list of per-band complex128 coefficient vectors (a list
of such lists with multichannel=True); backward(c) returns the signal of
length Ls.  A torch tensor on the GPU goes in and comes out as tensors:
forward gives (coefficient buffer, offsets) with band j of the kept bands at
buffer[..., offsets[j]:offsets[j+1]], backward takes that pair (or the buffer
alone), and nothing crosses to the host.
"""
import numpy as np

from . import _device
from .fscale import OctScale
from .nsdual import nsdual
from .nsgfwin_sl import nsgfwin
from .util import calcwinrange


def _refuse_above_ceiling(what, n):
    if int(n) > _device.NSGT_MAX_N:
        raise NotImplementedError("NSGT: %s = %d is above the device FFT's ceiling of %d points"
                                  % (what, n, _device.NSGT_MAX_N))


class NSGT(object):
    """The transform of signals of exactly Ls samples at rate fs on `scale`.

    real         the signal is real: only the bands from DC to Nyquist are
                 kept, less `reducedform` bands at either end (0, 1 or 2)
    matrixform   every kept band gets the same number of time channels, the
                 largest among them, so the coefficients stack into a matrix
    multichannel forward takes [nch, Ls] and returns one list per channel
    measurefft   accepted and ignored (there is no FFT planner to tune)
    """

    def __init__(self, scale, fs, Ls, real=True, measurefft=False, matrixform=False, reducedform=0,
                 multichannel=False):
        if not (fs > 0 and Ls > 0):
            raise ValueError("NSGT: fs and Ls must be positive, got %r and %r" % (fs, Ls))
        if reducedform not in (0, 1, 2):
            raise ValueError("NSGT: reducedform is 0, 1 or 2, got %r" % (reducedform,))
        _refuse_above_ceiling("Ls", Ls)
        self.scale, self.fs, self.Ls = scale, fs, Ls
        self.real, self.reducedform, self.multichannel = real, reducedform, multichannel
        self.measurefft = measurefft

        self.frqs, self.q = scale()
        self.g, rfbas, self.M = nsgfwin(self.frqs, self.q, fs, Ls, sliced=False)
        if matrixform:
            kept = self.M[_device.band_slice(len(self.M), True, reducedform)] if reducedform \
                else self.M
            self.M[:] = kept.max()
        self.wins, self.nn = calcwinrange(self.g, rfbas, Ls)
        self.gd = nsdual(self.g, self.wins, self.nn, self.M)
        _refuse_above_ceiling("nn", self.nn)
        _refuse_above_ceiling("the largest M", self.M.max())
        self._plan = None

    @property
    def plan(self):
        """The device plan, built at the first transform and kept."""
        if self._plan is None:
            self._plan = _device.DevicePlan(self.g, self.gd, self.wins, self.nn, self.M, self.Ls,
                                            self.real, self.reducedform)
        return self._plan

    def _split(self, row):
        o = self.plan.offsets
        return [row[o[j]:o[j + 1]].copy() for j in range(len(o) - 1)]

    def forward(self, s):
        'transform'
        if _device._is_tensor(s):
            x = s if self.multichannel else s[None]
            c = self.plan.forward_tensor(x.reshape(x.shape[0], -1))
            return (c if self.multichannel else c[0]), self.plan.offsets
        x = np.asarray(s, dtype=np.float64)
        x = x if self.multichannel else x[None]
        c = self.plan.forward(x.reshape(x.shape[0], -1))
        out = [self._split(row) for row in c]
        return out if self.multichannel else out[0]

    def backward(self, c):
        'inverse transform'
        if isinstance(c, tuple) and len(c) == 2 and _device._is_tensor(c[0]):
            c = c[0]
        if _device._is_tensor(c):
            y = self.plan.backward_tensor(c if self.multichannel else c[None])
            return y if self.multichannel else y[0]
        chans = c if self.multichannel else (c,)
        n = len(self.plan.M_used)
        for ch in chans:
            assert len(ch) == n
        buf = np.array([np.concatenate([np.asarray(b, dtype=np.complex128) for b in ch])
                        for ch in chans])
        y = self.plan.backward(buf)
        return list(y) if self.multichannel else y[0]


class CQ_NSGT(NSGT):
    """NSGT on the constant-Q scale of `bins` bands per octave from fmin to
    fmax."""

    def __init__(self, fmin, fmax, bins, fs, Ls, real=True, measurefft=False, matrixform=False,
                 reducedform=0, multichannel=False):
        if not (0 < fmin < fmax and bins > 0):
            raise ValueError("CQ_NSGT: need 0 < fmin < fmax and bins > 0, got %r, %r, %r"
                             % (fmin, fmax, bins))
        self.fmin, self.fmax, self.bins = fmin, fmax, bins
        NSGT.__init__(self, OctScale(fmin, fmax, bins), fs, Ls, real=real, measurefft=measurefft,
                      matrixform=matrixform, reducedform=reducedform, multichannel=multichannel)
