"""Frequency scales of the non-stationary Gabor transform (host NumPy, FP64).

A scale places `bnds` bands on the frequency axis.  Band b (an index, not
necessarily an integer) has the centre frequency F(b) and the quality factor
Q(b) = F(b) / (2 dF/db): the ratio of the centre to the distance between its
two neighbours.  Calling a scale returns the two vectors (F, Q) over the
integer bands, which is all the window planner reads.

The public names (OctScale, LogScale, LinScale, MelScale, F, Q, len, call) are
those of the NSGT package of T. Grill that the reference ships; the code is
this project's.  The vectors are evaluated one band at a time on Python
scalars: `x ** b` of a float and an int is not the same rounding as NumPy's
array power, and the planner's integer window lengths are pinned bit for bit.
"""
import numpy as np

_DIFF_STEP = 1.e-8   # half-width of the central difference behind a numerical Q


class Scale(object):
    """Base of the scales.  A subclass gives F; Q falls back to a central
    difference of F when the subclass has no closed form."""

    def __init__(self, bnds):
        self.bnds = int(bnds)

    def __len__(self):
        return self.bnds

    def _bands(self, bnd):
        return np.arange(self.bnds) if bnd is None else bnd

    def F(self, bnd=None):
        raise NotImplementedError("a scale defines F")

    def Q(self, bnd=None):
        b = self._bands(bnd)
        h = _DIFF_STEP
        spread = self.F(b + h) - self.F(b - h)      # = 2 h dF/db
        return self.F(b) * h / spread

    def __call__(self):
        per_band = lambda fn: np.fromiter((fn(b) for b in range(self.bnds)), dtype=float,
                                          count=self.bnds)
        return per_band(self.F), per_band(self.Q)


class _Geometric(Scale):
    """F(b) = fmin ratio^b.  A band reaches from F / sqrt(ratio) to
    F sqrt(ratio), so Q = F / (2 width) = sqrt(ratio) / (2 (ratio - 1)),
    the same for every band."""

    def __init__(self, fmin, fmax, bnds, ratio):
        Scale.__init__(self, bnds)
        self.fmin, self.fmax = float(fmin), float(fmax)
        self.pow2n = ratio
        self.q = np.sqrt(ratio) / (ratio - 1.) / 2.

    def F(self, bnd=None):
        return self.fmin * self.pow2n ** self._bands(bnd)

    def Q(self, bnd=None):
        return self.q


class OctScale(_Geometric):
    """`bpo` bands per octave starting at fmin; as many bands as it takes to
    reach fmax."""

    def __init__(self, fmin, fmax, bpo):
        octaves = np.log2(float(fmax) / fmin)
        self.bpo = int(bpo)
        _Geometric.__init__(self, fmin, fmax, int(np.ceil(octaves * bpo)) + 1, 2 ** (1. / self.bpo))


class LogScale(_Geometric):
    """Exactly `bnds` bands, geometrically spaced, the first at fmin and the
    last at fmax."""

    def __init__(self, fmin, fmax, bnds):
        octaves_per_band = np.log2(float(fmax) / float(fmin)) / (int(bnds) - 1)
        _Geometric.__init__(self, fmin, fmax, bnds, 2 ** octaves_per_band)


class LinScale(Scale):
    """`bnds` equidistant bands from fmin to fmax; Q grows with the frequency."""

    def __init__(self, fmin, fmax, bnds):
        Scale.__init__(self, bnds)
        self.fmin, self.fmax = float(fmin), float(fmax)
        self.df = (self.fmax - self.fmin) / (self.bnds - 1)

    def F(self, bnd=None):
        return self._bands(bnd) * self.df + self.fmin

    def Q(self, bnd=None):
        return self.F(bnd) / (self.df * 2)


def _hz_to_mel(f):
    return np.log10(f / 700. + 1.) * 2595.


def _mel_to_hz(m):
    return (np.power(10., m / 2595.) - 1.) * 700.


class MelScale(Scale):
    """`bnds` bands equidistant in mel (2595 log10(1 + f / 700)) from fmin to
    fmax.  Q is the base class's central difference."""

    def __init__(self, fmin, fmax, bnds):
        Scale.__init__(self, bnds)
        self.fmin, self.fmax = float(fmin), float(fmax)
        self.mmin, self.mmax = _hz_to_mel(self.fmin), _hz_to_mel(self.fmax)
        self.mbnd = (self.mmax - self.mmin) / (self.bnds - 1)

    def F(self, bnd=None):
        return _mel_to_hz(self._bands(bnd) * self.mbnd + self.mmin)
