"""Constant-Q / minimum-Q transforms on the GPU (tftransforms/minqt.py of the reference).

Same classes, constructor arguments and attributes as the reference:
`CQTKernel` (minqt.py:31-233), `MinQTKernel` (:309-335), `CQTransfo`
(:402-1070) and `MinQTransfo` (:1369-1550).  Both modes run on the GPU
(pyfasst_amd/csrc/fasst_cqt.hip, C ABI include/fasst_cqt.h):

perfRast=1, which FASST builds (audioModel.py:206-214): the rasterised
transform; `_spCQT` is the primary state and `cellCQT` a re-indexing view of
it (spCQT2CellCQT, :949-1011), derived when asked for.

perfRast=0, the constructors' default: the plain Schoerkhuber-Klapuri
transform.  `cellCQT` ({0..octaveNr-1: [bins*winNr, nframes_i], 'linear':
[linBins, nframes_0*winNr]}, host arrays) is the primary state, as in the
reference: computeTransform fills it and leaves no `_spCQT`; the `spCQT` /
`transfo` getters build the interpolated raster from the cells on first use
(cellCQT2spCQT, :870-947); assigning `transfo` / `spCQT` stores the matrix and
re-derives the cells at once (:648-658, :731-735); `del transfo` removes both
(:665-669), so a getter after it raises AttributeError, while `del t._spCQT`
alone makes the next getter rebuild the raster; invertTransform inverts
`cellCQT` (invertFromCellCQT, :1013-1055, plus invertLinearPart, :1452-1485).
The cells are packed into one buffer for each device call, so arrays the
caller replaced or edited in `cellCQT` are what the device sees.

Host side (setup constants only, as the reference designs them): the
one-octave spectral kernel (a few hundred FFTs of single atoms, thresholded
at `thresh` -- computed with NumPy so that the thresholding and the
normalisation weight are the reference's to the bit) and the anti-aliasing
Butterworth filter (scipy.signal.butter / lfilter_zi).

Deliberate deviation: `lowPassCoeffs=(B, A)` is used
as the anti-aliasing filter (the reference accepts the argument but then
never defines B, A and fails at the first octave).
"""
import ctypes

import numpy as np
import scipy.signal as spsig

from .. import _lib
from .._lib import check, dptr, lib
from ..tools.utils import nextpow2, sqrt_blackmanharris


def _dev(device):
    return _lib.default_device() if device is None else device


class CQTKernel(object):
    """One-octave CQT kernel (minqt.py:95-227), computed on the host."""

    def __init__(self, fmax, bins, fs, q=1, atomHopFactor=0.25, thresh=0.0005,
                 winFunc=sqrt_blackmanharris, perfRast=0):
        if fmax >= fs / 2.:
            raise ValueError("fmax (%s) is too big for fs (%s)" % (str(fmax), str(fs)))
        fmin = (fmax / 2.) * (2 ** (1. / bins))
        Q = 1. / (2 ** (1. / bins) - 1)
        Q = Q * q
        Nk_max = np.round(Q * fs / fmin)
        Nk_min = np.round(Q * fs / (fmin * (2 ** ((bins - 1.) / bins))))
        atomHOP = nextpow2(Nk_min * atomHopFactor) // 2
        first_center = np.ceil(Nk_max / 2.)
        first_center = atomHOP * np.ceil(first_center * 1. / atomHOP)
        FFTLen = nextpow2(first_center + np.ceil(Nk_max / 2.))
        winNr = np.floor((FFTLen - np.ceil(Nk_max / 2.) - first_center) / atomHOP) + 1
        if perfRast and winNr == 0:
            FFTLen = FFTLen * 2
            winNr = np.floor((FFTLen - np.ceil(Nk_max / 2.) - first_center) / atomHOP)
        last_center = first_center + (winNr - 1.) * atomHOP
        fftHOP = (last_center + atomHOP) - first_center
        fftOLP = (FFTLen - fftHOP) * (1. / FFTLen) * 100.
        sparKernel = np.zeros([int(bins * winNr), int(FFTLen)], dtype=complex)
        frequencies = []
        for k in np.arange(bins):
            Nk = np.round(Q * fs / (fmin * (2 ** ((k * 1.) / bins))))
            winFct = winFunc(int(Nk))
            fk = fmin * (2 ** ((k * 1.) / bins))
            frequencies.append(fk)
            atom = (winFct * 1. / Nk) * np.exp(2 * np.pi * 1j * fk * np.arange(Nk) / fs)
            atomOffset = first_center - np.ceil(Nk / 2.)
            for i in np.arange(winNr):
                shift = atomOffset + i * atomHOP
                tempKernel = np.zeros(int(FFTLen), dtype=complex)
                tempKernel[int(shift):int(Nk + shift)] = atom
                specKernel = np.fft.fft(tempKernel)
                specKernel[np.abs(specKernel) <= thresh] = 0
                sparKernel[int(i + k * winNr)] = specKernel
        sparKernel = (sparKernel.T) * 1. / FFTLen
        wx1 = np.argmax(sparKernel[:, 0])
        wx2 = np.argmax(sparKernel[:, -1])
        wK = sparKernel[wx1:wx2, :]
        wK = np.diag(np.dot(wK, np.conjugate(wK.T)))
        wK = wK[int(np.round(1. / q)):int(len(wK) - np.round(1. / q) - 1)]
        weight = 1. / np.mean(np.abs(wK))
        weight *= (fftHOP * 1. / FFTLen)
        weight = np.sqrt(weight)
        sparKernel *= weight
        self.sparKernel = np.ascontiguousarray(sparKernel)
        self.weight = weight
        self.atomHOP = atomHOP
        self.FFTLen = FFTLen
        self.fftOLP = fftOLP
        self.fftHOP = fftHOP
        self.bins = bins
        self.winNr = winNr
        self.Nk_max = Nk_max
        self.Q = Q
        self.fmin = fmin
        self.fmax = fmax
        self.frequencies = frequencies
        self.perfRast = perfRast
        self.first_center = first_center
        self.fs = fs
        self.winFunc = winFunc
        self.thresh = thresh
        self.q = q

    def __str__(self):
        description = "CQT Kernel structure, containing:\n"
        for k, v in self.__dict__.items():
            description += str(k) + ': ' + str(v) + '\n'
        return description


class MinQTKernel(CQTKernel):
    """MinQT kernel (minqt.py:312-335): CQT up to the frequency where the
    linear FFT bins of linFTLen are as dense as the CQT bins."""

    def __init__(self, bins, fmax, fs, linFTLen=2048, **kwargs):
        Q = 1. / (2 ** (1. / bins) - 1)
        Kmax = int(np.ceil(Q))
        fmax = 2 ** (-1. / bins) * Kmax * fs * 1. / linFTLen
        self.Q = Q
        self.Kmax = Kmax
        self.linFTLen = linFTLen
        self.fs = fs
        self.fmax = fmax
        self.bins = bins
        super(MinQTKernel, self).__init__(fmax=self.fmax, fs=self.fs, bins=self.bins, **kwargs)
        self.linBins = linFTLen // 2 - Kmax + 1
        self.linWindow = self.winFunc(linFTLen)


class CQTransfo(object):
    """Constant-Q transform (minqt.py:402-1070), on the GPU in both modes."""
    transformname = 'cqt'

    def __init__(self, fmin, fmax, bins, fs, q=1, atomHopFactor=0.25, thresh=0.0005,
                 winFunc=sqrt_blackmanharris, perfRast=0, cqtkernel=None, lowPassCoeffs=None,
                 data=None, verbose=0, device=None, **kwargs):
        self.verbose = verbose
        self.device = device
        self.fmin = fmin
        self.fmax = fmax
        self.bins = bins
        self.bpo = bins
        self.fs = fs
        self.q = q
        self.atomHopFactor = atomHopFactor
        self.thresh = thresh
        if winFunc is None:
            winFunc = sqrt_blackmanharris
        self.winFunc = winFunc
        self.perfRast = perfRast
        self.octaveNr = np.ceil(np.log2(fmax * 1. / fmin))
        self.freqbins = bins * self.octaveNr
        self.fmin = (fmax / (2 ** self.octaveNr)) * 2 ** (1. / bins)
        if lowPassCoeffs is None:
            self.LPorder = 6
            self.cutoff = 0.5
            self.B, self.A = spsig.butter(N=self.LPorder, Wn=self.cutoff, btype='low')
        else:
            self.B, self.A = (np.asarray(c, dtype=np.float64) for c in lowPassCoeffs)
        if cqtkernel is None:
            self.cqtkernel = CQTKernel(fmax=fmax, bins=bins, fs=fs, q=q,
                                       atomHopFactor=atomHopFactor, thresh=thresh,
                                       winFunc=winFunc, perfRast=perfRast)
        else:
            self.cqtkernel = cqtkernel
        self._h = None
        if data is not None:
            self.computeTransform(data=data)

    # ---------------------------------------------------------------- device
    def _context(self):
        if self._h is not None:
            return self._h
        k = self.cqtkernel
        B = np.ascontiguousarray(self.B, dtype=np.float64)
        A = np.ascontiguousarray(self.A, dtype=np.float64)
        if B.size != 7 or A.size != 7:
            raise NotImplementedError("the GPU filtfilt handles 6th-order anti-aliasing filters")
        B, A = B / A[0], A / A[0]
        zi = np.ascontiguousarray(spsig.lfilter_zi(B, A), dtype=np.float64)
        spar = np.ascontiguousarray(k.sparKernel, dtype=np.complex128)
        lin = getattr(k, 'linFTLen', 0) if isinstance(self, MinQTransfo) else 0
        lw = (np.ascontiguousarray(k.linWindow, dtype=np.float64) if lin
              else np.zeros(1))
        h = ctypes.c_void_p()
        check(lib.cqt_create(_dev(self.device), int(k.bins), int(self.octaveNr), int(k.winNr),
                             int(k.FFTLen), int(k.fftHOP), int(k.atomHOP), int(k.first_center),
                             dptr(spar), dptr(B), dptr(A), dptr(zi), int(lin),
                             int(getattr(k, 'Kmax', 0)) if lin else 0,
                             int(getattr(k, 'linBins', 0)) if lin else 0, dptr(lw),
                             ctypes.byref(h)), "cqt_create")
        self._h = h
        return h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and lib is not None:
            lib.cqt_destroy(h)
            self._h = None

    def _shape(self, L):
        F, W = ctypes.c_int(0), ctypes.c_int(0)
        nfr = np.zeros(int(self.octaveNr), dtype=np.int32)
        check(lib.cqt_shape(self._context(), L, ctypes.byref(F), ctypes.byref(W),
                            _lib.iptr(nfr)), "cqt_shape")
        return F.value, W.value, nfr

    # ---------------------------------------------------------------- forward
    def computeTransform(self, data):
        """Computes the desired transform (minqt.py:466-469)."""
        return self.computeCQT(data)

    def computeCQT(self, data):
        """CQT of data on the GPU (minqt.py:471-646): the raster with
        perfRast=1, the per-octave cells with perfRast=0."""
        if hasattr(self, '_spCQT'):
            del self._spCQT
        if hasattr(self, 'cellCQT'):
            del self.cellCQT
        if not self.perfRast:
            return self._compute_cells(data)
        x = np.ascontiguousarray(np.asarray(data, dtype=np.float64).ravel())
        F, W = self._bookkeeping(x.size)
        sp = np.empty((F, W), dtype=np.complex128)
        check(lib.cqt_forward(self._context(), dptr(x), x.size, dptr(sp)), "cqt_forward")
        self._spCQT = sp

    def _bookkeeping(self, L):
        """The attributes computeCQT leaves for a signal of L samples
        (minqt.py:523-556), without the transform; returns (freqbins, width)."""
        k = self.cqtkernel
        F, W, nfr = self._shape(int(L))
        self.datalen_init = int(L)
        self.maxBlock = int(k.FFTLen * (2 ** (self.octaveNr - 1)))
        self.suffixZeros = self.maxBlock
        self.prefixZeros = self.maxBlock
        self.nframes = [np.float64(n) for n in nfr]
        return F, W

    def prepare_resident(self, L):
        """State as after computeTransform() of a signal of L samples whose
        transform stays on the device (FASST.comp_transf_Cx): the frame
        bookkeeping is set, no host copy of the transform exists.  Returns
        (freqbins, width).  Needs perfRast=1."""
        if not self.perfRast:
            raise NotImplementedError("the device-resident transform is the rasterised one")
        F, W = self._shape(int(L))[:2]    # raises before any attribute moves
        for attr in ('_spCQT', 'cellCQT'):
            if hasattr(self, attr):
                delattr(self, attr)
        return self._bookkeeping(L)

    def batch_info(self):
        """(signals, kernel launches) of the last forward / inverse chain on
        this transform's device context (cqt_batch_info)."""
        n, k = ctypes.c_int(0), ctypes.c_long(0)
        check(lib.cqt_batch_info(self._context(), ctypes.byref(n), ctypes.byref(k)),
              "cqt_batch_info")
        return n.value, k.value

    # ------------------------------------------------------ perfRast=0 cells
    def _cell_layout(self):
        """Shapes of the packed cells of a signal of datalen_init samples."""
        k = self.cqtkernel
        nfr = np.zeros(int(self.octaveNr), dtype=np.int32)
        lin = ctypes.c_int(0)
        check(lib.cqt_cell_shape(self._context(), int(self.datalen_init), _lib.iptr(nfr),
                                 ctypes.byref(lin)), "cqt_cell_shape")
        M = int(k.bins * k.winNr)
        shapes = [(noct, (M, int(n))) for noct, n in enumerate(nfr)]
        if lin.value:
            shapes.append(('linear', (int(k.linBins), lin.value)))
        return nfr, shapes

    def _unpack_cells(self, buf, shapes):
        cells, off = {}, 0
        for key, shp in shapes:
            n = shp[0] * shp[1]
            cells[key] = buf[off:off + n].reshape(shp)
            off += n
        return cells

    def _pack_cells(self):
        """self.cellCQT as the one buffer the device calls take."""
        _, shapes = self._cell_layout()
        parts = []
        for key, shp in shapes:
            c = np.asarray(self.cellCQT[key])
            if c.shape != shp:
                raise ValueError("cellCQT[%r] has shape %s instead of %s" % (key, c.shape, shp))
            parts.append(np.asarray(c, dtype=np.complex128).ravel())
        return np.ascontiguousarray(np.concatenate(parts)), shapes

    def _compute_cells(self, data):
        """computeCQT, non-raster branch (minqt.py:495-522), and for MinQT the
        linear cell of computeLinearPart (:1410-1435), in one GPU pass."""
        x = np.ascontiguousarray(np.asarray(data, dtype=np.float64).ravel())
        k = self.cqtkernel
        self.datalen_init = x.shape[0]
        self.maxBlock = int(k.FFTLen * (2 ** (self.octaveNr - 1)))
        self.suffixZeros = self.maxBlock
        self.prefixZeros = self.maxBlock
        nfr, shapes = self._cell_layout()
        self.nframes = [np.float64(n) for n in nfr]
        buf = np.empty(sum(a * b for _, (a, b) in shapes), dtype=np.complex128)
        check(lib.cqt_forward_cells(self._context(), dptr(x), x.size, dptr(buf)),
              "cqt_forward_cells")
        self.cellCQT = self._unpack_cells(buf, shapes)

    def cellCQT2spCQT(self):
        """The full matrix from self.cellCQT (minqt.py:870-947; for MinQT with
        linCellCQT2LinSpCQT, :1527-1549), on the GPU."""
        if self.perfRast:
            raise NotImplementedError("with perfRast=1 the raster is the transform itself")
        buf, _ = self._pack_cells()
        F, W, _ = self._shape(int(self.datalen_init))
        sp = np.empty((F, W), dtype=np.complex128)
        check(lib.cqt_cells_to_raster(self._context(), dptr(buf), int(self.datalen_init),
                                      dptr(sp)), "cqt_cells_to_raster")
        self._spCQT = sp

    def _cells_from_raster(self):
        """spCQT2CellCQT (minqt.py:949-1011, 1500-1525) on the GPU."""
        F, W, _ = self._shape(int(self.datalen_init))
        sp = np.ascontiguousarray(self._spCQT, dtype=np.complex128)
        if sp.shape != (F, W):
            raise ValueError("spCQT has shape %s instead of %s" % (sp.shape, (F, W)))
        _, shapes = self._cell_layout()
        buf = np.empty(sum(a * b for _, (a, b) in shapes), dtype=np.complex128)
        check(lib.cqt_raster_to_cells(self._context(), dptr(sp), int(self.datalen_init),
                                      dptr(buf)), "cqt_raster_to_cells")
        self.cellCQT = self._unpack_cells(buf, shapes)
        return self.cellCQT

    def invertFromCellCQT(self):
        """Inverse of self.cellCQT's octaves (minqt.py:1019-1055), on the GPU."""
        return self._invert_cells(linear=False)

    def _invert_cells(self, linear):
        self._check_attr_inversion()
        buf, shapes = self._pack_cells()
        if shapes[-1][0] == 'linear' and not linear:
            buf[-shapes[-1][1][0] * shapes[-1][1][1]:] = 0
        y = np.empty(int(self.datalen_init))
        check(lib.cqt_inverse_cells(self._context(), dptr(buf), y.size, dptr(y)),
              "cqt_inverse_cells")
        return y

    # ---------------------------------------------------------------- transfo
    def _set_transfo(self, X):
        if X.shape[0] == self.freqbins:
            self._spCQT = np.copy(X)
            if not self.perfRast:
                self.spCQT2CellCQT()
            elif hasattr(self, 'cellCQT'):
                del self.cellCQT
        else:
            raise ValueError('Transfo not of the right size: ' + str(X.shape) +
                             ' instead of ' + str(self.freqbins))

    def _get_transfo(self):
        return self._get_spCQT()

    def _del_transfo(self):
        del self._spCQT
        if not self.perfRast:
            del self.cellCQT     # "erasing everything" (minqt.py:665-669)
        elif hasattr(self, 'cellCQT'):
            del self.cellCQT

    transfo = property(fget=_get_transfo, fdel=_del_transfo, fset=_set_transfo,
                       doc="returns the computed transform")

    def _get_spCQT(self):
        if not hasattr(self, '_spCQT'):
            if self.perfRast or not hasattr(self, 'cellCQT'):
                raise AttributeError("Some CQT should be computed before getting it.")
            self.cellCQT2spCQT()     # minqt.py:722-729
        return self._spCQT

    def _set_spCQT(self, value):
        self._spCQT = value
        if not self.perfRast:
            self.spCQT2CellCQT()     # minqt.py:731-735
        elif hasattr(self, 'cellCQT'):
            del self.cellCQT

    spCQT = property(fget=_get_spCQT, fset=_set_spCQT,
                     doc="spCQT: the constant Q transform, in a readable format.")

    def spCQT2CellCQT(self):
        """Per-octave cells from spCQT (minqt.py:949-1011): re-indexing only."""
        if not self.perfRast:
            return self._cells_from_raster()
        k = self.cqtkernel
        bins, winNr = int(k.bins), int(k.winNr)
        emptyHops = k.first_center * 1. / k.atomHOP
        self.cellCQT = {}
        for noct in range(int(self.octaveNr)):
            dropped = emptyHops * (2. ** (self.octaveNr - noct - 1) - 1)
            X = self._spCQT[int(bins * (self.octaveNr - noct - 1)):
                            int(bins * (self.octaveNr - noct)), ::int(2 ** noct)]
            X = np.hstack([np.zeros([bins, int(dropped)]), X])
            X = np.hstack([X, np.zeros([bins, int(np.ceil(X.shape[1] / winNr) * winNr -
                                                  X.shape[1])])])
            if winNr > 1:
                cell = np.zeros([bins * winNr, int(np.ceil(X.shape[1] / winNr))], dtype=complex)
                for nbin in range(bins):
                    cell[nbin * winNr:(nbin + 1) * winNr, :] = X[nbin].reshape(
                        winNr, X.shape[1] // winNr, order='F')
            else:
                cell = np.copy(X)
            self.cellCQT[noct] = np.ascontiguousarray(cell[:, :int(self.nframes[noct])])
        return self.cellCQT

    def _get_time_stamps(self):
        nframes = self.nframes[0] * self.cqtkernel.winNr
        return (np.arange(nframes) * self.cqtkernel.atomHOP +
                self.cqtkernel.first_center * 2 ** (self.octaveNr - 1) - self.prefixZeros)

    time_stamps = property(fget=_get_time_stamps, doc="time stamps for spCQT")

    def _compute_frequencies(self):
        return (self.cqtkernel.fmin *
                2 ** (np.arange(self.cqtkernel.bins * self.octaveNr) / self.cqtkernel.bins -
                      (self.octaveNr - 1)))

    freq_stamps = property(fget=lambda self: self._compute_frequencies(),
                           doc="frequency stamps for spCQT")

    qValues = property(fget=lambda self: self.freq_stamps[:-1] / np.diff(self.freq_stamps),
                       doc="$Q$ values, approximated")

    # ---------------------------------------------------------------- inverse
    def _check_attr_inversion(self):
        for attr in ['datalen_init', 'prefixZeros', 'suffixZeros', 'octaveNr']:
            if not hasattr(self, attr):
                raise AttributeError("Missing attribute to compute the inverse "
                                     "transform: %s." % attr)
        return True

    def _invert(self):
        self._check_attr_inversion()
        sp = np.ascontiguousarray(self._spCQT, dtype=np.complex128)
        y = np.empty(int(self.datalen_init))
        check(lib.cqt_inverse(self._context(), dptr(sp), y.size, dptr(y)), "cqt_inverse")
        return y

    def invertTransform(self):
        """invertFromCellCQT (minqt.py:1013-1055), on the GPU."""
        if not self.perfRast:
            return self.invertFromCellCQT()
        return self._invert()


class MinQTransfo(CQTransfo):
    """Minimum-Q transform (minqt.py:1369-1550): CQT below the split
    frequency, linear STFT bins above; on the GPU in both modes."""
    transformname = 'minqt'

    def __init__(self, fmax, bins, linFTLen, fs, fmin=70, **kwargs):
        data = kwargs.pop('data', None)
        super(MinQTransfo, self).__init__(fmax=fmax, fs=fs, bins=bins, cqtkernel=0, fmin=fmin,
                                          **kwargs)
        self.cqtkernel = MinQTKernel(linFTLen=linFTLen, fmax=fmax, bins=bins, fs=fs, q=self.q,
                                     atomHopFactor=self.atomHopFactor, thresh=self.thresh,
                                     winFunc=self.winFunc, perfRast=self.perfRast)
        self.octaveNr = np.ceil(np.log2(self.cqtkernel.fmax * 1. / fmin))
        self.fmin = (self.cqtkernel.fmax / (2. ** self.octaveNr)) * 2 ** (1. / bins)
        self.freqbins = self.octaveNr * self.cqtkernel.bins + self.cqtkernel.linBins
        if data is not None:
            self.computeTransform(data)

    def computeTransform(self, data):
        """CQT part and linear part in one GPU pass (minqt.py:1404-1450)."""
        super(MinQTransfo, self).computeTransform(data)
        self.offsetSTFT = self.cqtkernel.first_center

    def prepare_resident(self, L):
        out = super(MinQTransfo, self).prepare_resident(L)
        self.offsetSTFT = self.cqtkernel.first_center
        return out

    def computeLinearPart(self, data):
        """cellCQT['linear'] of data (minqt.py:1410-1435).  computeTransform
        already fills it; this recomputes it alone, as the reference allows."""
        if self.perfRast:
            raise NotImplementedError("with perfRast=1 the linear rows are part of spCQT")
        if not hasattr(self, 'cellCQT'):
            raise AttributeError("computeCQT should be called before computeLinearPart")
        cells = self.cellCQT
        self._compute_cells(data)
        cells['linear'] = self.cellCQT['linear']
        self.cellCQT = cells
        self.offsetSTFT = self.cqtkernel.first_center

    def invertTransform(self):
        """perfRast=1: invertFromSpCQTRast + invertLinearPart; perfRast=0:
        invertFromCellCQT + invertLinearPart (minqt.py:1452-1485), on the GPU."""
        if not self.perfRast:
            return self._invert_cells(linear=True)
        return self._invert()

    def invertLinearPart(self):
        """Inverse of cellCQT['linear'] alone (minqt.py:1469-1485), on the GPU."""
        if self.perfRast:
            raise NotImplementedError("with perfRast=1 the linear rows are inverted with spCQT")
        saved = self.cellCQT
        try:
            self.cellCQT = dict(saved)
            for noct in range(int(self.octaveNr)):
                self.cellCQT[noct] = np.zeros_like(saved[noct])
            return self._invert_cells(linear=True)
        finally:
            self.cellCQT = saved

    def linCellCQT2LinSpCQT(self):
        """cellCQT['linear'] into the linear rows of spCQT (minqt.py:1534-1549);
        cellCQT2spCQT does both parts in one device call."""
        if self.perfRast:
            raise NotImplementedError("with perfRast=1 the linear rows are part of spCQT")
        self.cellCQT2spCQT()

    def _compute_frequencies(self):
        freqs = super(MinQTransfo, self)._compute_frequencies()
        linfreqs = (np.arange(self.cqtkernel.Kmax, self.cqtkernel.Kmax + self.cqtkernel.linBins,
                              dtype=np.float64) * self.cqtkernel.fs / self.cqtkernel.linFTLen)
        return np.concatenate([freqs, linfreqs])

    def spCQT2CellCQT(self):
        """CQT cells plus the linear part (minqt.py:1500-1525): re-indexing only."""
        if not self.perfRast:
            return self._cells_from_raster()
        super(MinQTransfo, self).spCQT2CellCQT()
        k = self.cqtkernel
        emptyHops = k.first_center * 1. / k.atomHOP
        dropped = emptyHops * (2. ** (self.octaveNr - 1) - 1)
        X = self._spCQT[int(k.bins * self.octaveNr):int(k.bins * self.octaveNr + k.linBins)]
        X = np.hstack([np.zeros([int(k.linBins), int(dropped)]), X])
        self.cellCQT['linear'] = np.ascontiguousarray(X[:, :int(self.nframes[0] * k.winNr)])
        return self.cellCQT
