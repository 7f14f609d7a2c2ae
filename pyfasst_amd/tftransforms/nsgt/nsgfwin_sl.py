"""Windows of the NSGT for a frequency scale (host NumPy, FP64).  The name
and signature of nsgfwin are the reference package's; the code is this
project's.  Only the non-sliced arm exists here; the sliced planner is
pyfasst_amd.tftransforms.slicq.nsgfwin_sliced.

The two-sided spectrum of Ls bins gets one band at DC, one per scale
frequency inside (0, sr/2), one at Nyquist, and the mirror images of the scale
bands.  With p[k] the band positions in bins, band k gets a Hann window as wide
as the distance between its neighbours, M[k] = round(p[k+1] - p[k-1]) (the DC
band twice its distance to the first band, the last band up to Ls), never
narrower than min_win.
"""
from warnings import warn

import numpy as np

from .util import hannwin


def _inside_band(f, q, nyquist):
    """The scale frequencies in (0, nyquist): leading non-positive ones and
    everything from the first one at or above Nyquist on are dropped."""
    positive = np.flatnonzero(f > 0)
    if positive.size == 0:
        raise ValueError("nsgfwin: no positive frequency in the scale")
    lo = positive[0]
    above = np.flatnonzero(f[lo:] >= nyquist)
    hi = lo + above[0] if above.size and above[0] > 0 else len(f)
    return f[lo:hi], q[lo:hi]


def nsgfwin(f, q, sr, Ls, sliced=False, min_win=4, Qvar=1, dowarn=True):
    """Returns (g, rfbas, M): the windows, the rounded band positions in bins
    and the window lengths, 2 (len(f) + 1) bands."""
    if sliced:
        raise NotImplementedError("nsgfwin(sliced=True) refuses: the sliced planner is "
                                  "pyfasst_amd.tftransforms.slicq.nsgfwin_sliced")
    nyquist = sr / 2.
    f, q = _inside_band(np.asarray(f), np.asarray(q), nyquist)
    if len(f) != len(q) or np.any(np.diff(f) <= 0) or np.any(q <= 0):
        raise ValueError("nsgfwin: frequencies must increase and every Q be positive")

    # a band narrower than 8 bins per unit of Q cannot hold its window
    too_sharp = q >= f * (Ls / (8. * sr))
    if dowarn and np.any(too_sharp):
        warn("Q-factor too high for frequencies %s"
             % ",".join("%.2f" % x for x in f[too_sharp]))

    nscale = len(f)
    hz = np.concatenate(((0.,), f, (nyquist,), sr - f[::-1]))
    pos = hz * (float(Ls) / sr)

    width = np.empty(len(pos))
    width[0] = 2 * pos[1]
    width[1:-1] = pos[2:] - pos[:-2]
    width[-1] = Ls - pos[-2]
    M = np.maximum(np.rint(width).astype(int), min_win)
    g = [hannwin(m) for m in M]

    # the highest scale band moves midway between its lower neighbour and
    # Nyquist, and its mirror image with it
    top = nscale
    pos[top] = (pos[top - 1] + pos[top + 1]) / 2
    pos[top + 2] = Ls - pos[top]
    return g, np.rint(pos).astype(int), M
