"""pyfasst_amd.tftransforms.nsgt: the non-stationary Gabor transform (the
constant-Q transform with exact reconstruction of Holighaus, Velasco, Doerfler
and Grill) on the GPU.  Planning is host NumPy; the transforms run in
libfasst_hip.so (include/fasst_nsgt.h).

The public names and signatures are those of the NSGT package by Thomas Grill
(after the MATLAB toolbox of NUHAG, University of Vienna) that the reference
ships; the code here is this project's own, written from the papers' formulas.

The sliced transform (NSGT_sliced, CQ_NSGT_sliced, the sliced planner) is
pyfasst_amd.tftransforms.slicq; the names of this package still refuse with
NotImplementedError and say so.  Out of scope, refusing likewise: the audio
file helpers; nothing here is wired into FASST, DEMIX or SeparateLeadProcess.
"""
from .cq import NSGT, CQ_NSGT
from .slicq import NSGT_sliced, CQ_NSGT_sliced
from .fscale import Scale, OctScale, LogScale, LinScale, MelScale
from .nsgfwin_sl import nsgfwin
from .nsdual import nsdual
from .util import calcwinrange, chkM, hannwin

__all__ = ["NSGT", "CQ_NSGT", "NSGT_sliced", "CQ_NSGT_sliced", "Scale", "OctScale", "LogScale",
           "LinScale", "MelScale", "nsgfwin", "nsdual", "calcwinrange", "chkM", "hannwin",
           "NonStatGaborT", "NSGMinQT", "SndReader", "SndWriter"]


def _no_audio(name):
    class _Refuse(object):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("%s: the audio file helpers (audio.py) are out of scope; read "
                                      "the file with pyfasst_amd.audioObject" % name)
    _Refuse.__name__ = name
    return _Refuse


SndReader = _no_audio("SndReader")
SndWriter = _no_audio("SndWriter")


class NonStatGaborT(object):
    """An NSGT behind the interface the transforms of tftransforms.tft share:
    computeTransform(data) on monophonic data keeps the coefficients in
    `transfo`, invertTransform() returns the signal from them, and a signal of
    another length rebuilds the plan.  matrixform is on by default.  (The
    reference's invertTransform reads a name that is not defined and cannot
    run; this one inverts the stored coefficients.)"""
    transformname = 'nsgt'
    _passed_on = ('measurefft', 'multichannel')   # NSGT options taken from **kwargs

    def __init__(self, scale, fs, datalength, real=True, matrixform=1, reducedform=0, **kwargs):
        self.fs = fs
        self.kwargs = dict(kwargs, real=real, matrixform=matrixform, reducedform=reducedform)
        self._build(scale, datalength)
        self.freqbins = len(scale.F()) + 2          # the scale's bands, DC and Nyquist

    def _build(self, scale, datalength):
        options = dict((k, v) for k, v in self.kwargs.items()
                       if k in self._passed_on + ('real', 'matrixform', 'reducedform'))
        self.nsgt = NSGT(scale, self.fs, datalength, **options)

    def checkDataLength(self, datalength):
        if datalength != self.nsgt.Ls:
            self._build(self.nsgt.scale, datalength)

    def computeTransform(self, data):
        self.checkDataLength(data.size)
        self.transfo = self.nsgt.forward(data)

    def invertTransform(self):
        return self.nsgt.backward(self.transfo)

    @property
    def transfo(self):
        return self._transfo

    @transfo.setter
    def transfo(self, value):
        self._transfo = value

    @transfo.deleter
    def transfo(self):
        del self._transfo


class NSGMinQT(NonStatGaborT):
    transformname = 'nsgminqt'

    def __init__(self, fmin, fmax, bins, linFTLen, fs, datalength=None, **kwargs):
        raise NotImplementedError(
            "NSGMinQT: the reference's constructor calls super(nsgtMinQT, self).__init__, and "
            "nsgtMinQT is not defined anywhere (nsgt/__init__.py:120): it raises NameError for "
            "every argument, so there is no behaviour to reproduce")
