"""NumPy restatement of the reference CQT / MinQT with perfRast=0
(tftransforms/minqt.py), the constructors' default mode.

TEST INFRASTRUCTURE ONLY.  The one-octave kernel, the filtfilt, the STFT and
the spCQT -> cell re-indexing are oracle/cqt_ref.py's; this module adds what
perfRast=0 does differently:

  RefCells.forward()        computeCQT, non-raster branch    minqt.py:495-522
                            + computeLinearPart              minqt.py:1410-1435
  RefCells.cells_to_sp()    cellCQT2spCQT                    minqt.py:870-947
                            + linCellCQT2LinSpCQT            minqt.py:1534-1549
  RefCells.sp_to_cells()    spCQT2CellCQT                    minqt.py:949-1011, 1500-1525
  RefCells.inverse()        invertFromCellCQT                minqt.py:1019-1055
                            + invertLinearPart               minqt.py:1469-1485

Pinned against the reference's own outputs (tests/golden/cqt_cells.npz, made
by tests/golden/make_golden_cqt_cells.py) in tests/test_cqt_cells_ref_golden.py.

Quirks kept: the filter and decimation the reference also runs after the last
octave (its guard `i != self.octaveNr` is always true) feed nothing and are
left out; the drop alignment leaves the last int(drop*nshifts) columns of a
row at their pre-alignment values when winNr > 1 and at zero when winNr == 1;
the interpolated columns hold real magnitudes, the populated ones stay complex.

emptyHops = first_center / atomHOP is an integer by construction
(first_center = atomHOP * ceil(.), minqt.py:127-128), so `drop` never has a
fractional part and int(drop * nshifts) never floors for a kernel the
constructors build.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "oracle"))
import cqt_ref  # noqa: E402

# name -> (kind, constructor kwargs, signal length); the smallest geometries
# at which each index rule can go wrong (see tests/golden/make_golden_cqt_cells.py)
CASES = {
    # nshifts 1, 2, 4 (1 and 3 interpolated columns), winNr = 5, odd length
    "cqt12": ("cqt", dict(fmin=400, fmax=3000, bins=12, fs=8000), 2001),
    # 4 octaves, winNr = 7, W = 252; the last octave has 3 frames: the
    # fill_value = 0 tail and a populated column count (32) that is no
    # multiple of winNr
    "cqt24": ("cqt", dict(fmin=250, fmax=3900, bins=24, fs=8000), 101),
    # the linear cell, its drop, invertLinearPart; winNr = 1 (minqt.py:915-926)
    "mqt12": ("mqt", dict(fmin=120, fmax=3000, bins=12, fs=8000, linFTLen=256), 1501),
    # 48 bins: a kernel of more rows than one pass of k_cqt_band's 256 threads
    "mqt48": ("mqt", dict(fmin=700, fmax=3900, bins=48, fs=8000, linFTLen=256), 1777),
}
# cases whose raster is modified, re-assigned and inverted
ROUNDTRIP = ("cqt12", "mqt12")


def signal(name):
    _, _, n = CASES[name]
    rs = np.random.RandomState(sorted(CASES).index(name) + 11)
    t = np.arange(n)
    return rs.randn(n) * (0.3 + np.sin(t / 97.0) ** 2) + np.sin(2 * np.pi * 0.11 * t)


def modify(name, sp, bins):
    """The edit of the round-trip cases: rows scaled by a ramp, the octave
    above the lowest zeroed."""
    out = sp * np.linspace(0.5, 1.5, sp.shape[0])[:, None]
    out[bins:2 * bins] = 0
    return out


def interp_magnitudes(y, ns, width):
    """What interp1d(x=arange(0, width, ns), y, kind='linear',
    bounds_error=False, fill_value=0)(arange(width)) evaluates for a float64
    1-D y: scipy hands the work to numpy.interp, whose operation order is
        slope = (y_hi - y_lo) / (x_hi - x_lo);  slope * (x - x_lo) + y_lo
    and zero past the last sample point."""
    x = np.arange(width)
    lo = x // ns
    out = np.zeros(width)
    ok = lo + 1 < y.size
    slope = (y[lo[ok] + 1] - y[lo[ok]]) / np.float64(ns)
    out[ok] = slope * (x[ok] - lo[ok] * ns).astype(np.float64) + y[lo[ok]]
    on = (x % ns == 0)
    out[on] = y[lo[on]]
    return out


class RefCells(cqt_ref.RefCQT):
    """CQTransfo / MinQTransfo with perfRast=0."""

    def __init__(self, kind, fmin, fmax, bins, fs, linFTLen=2048, atomHopFactor=0.25):
        super(RefCells, self).__init__(kind, fmin=fmin, fmax=fmax, bins=bins, fs=fs,
                                       linFTLen=linFTLen, atomHopFactor=atomHopFactor)
        kw = dict(q=1, atomHopFactor=atomHopFactor, thresh=0.0005,
                  winFunc=cqt_ref.sqrt_blackmanharris, perfRast=0)
        if kind == 'cqt':
            self.k = cqt_ref.cqt_kernel(fmax=fmax, bins=bins, fs=fs, **kw)
        else:
            self.k = cqt_ref.minqt_kernel(bins=bins, fmax=fmax, fs=fs, linFTLen=linFTLen, **kw)

    def scalars(self):
        k = self.k
        return np.array([k.atomHOP, k.first_center, k.winNr, k.fftHOP, k.FFTLen, self.octaveNr],
                        dtype=np.float64)

    # ------------------------------------------------------------ forward
    def forward(self, data):
        k = self.k
        data = np.asarray(data, dtype=np.float64)
        self.datalen_init = data.shape[0]
        self.maxBlock = int(k.FFTLen * (2 ** (self.octaveNr - 1)))
        self.prefixZeros = self.suffixZeros = self.maxBlock
        x = np.concatenate([np.zeros(self.prefixZeros), data, np.zeros(self.suffixZeros)])
        xpad = x
        K = np.ascontiguousarray(np.conjugate(k.sparKernel.T))
        N = int(k.FFTLen)
        self.nframes = []
        cells = {}
        oct_n = int(self.octaveNr)
        for i in range(oct_n):
            nframes = np.floor(((x.size - k.FFTLen) / k.fftHOP) + 1)
            self.nframes.append(nframes)
            cell = np.zeros([int(self.bins * k.winNr), int(nframes)], dtype=complex)
            for n in range(int(nframes)):
                a = int(n * k.fftHOP)
                cell[:, n] = np.dot(K, np.fft.fft(x[a:a + N], n=N))
            cells[i] = cell
            if i != oct_n - 1:      # the reference also filters after the last octave: unused
                x = cqt_ref.spsig.filtfilt(self.B, self.A, x)[::2]
        if self.kind != 'cqt':
            self.offsetSTFT = k.first_center
            X = cqt_ref.stft(xpad[int(self.offsetSTFT):], k.linWindow, k.atomHOP, k.linFTLen)
            cells['linear'] = X[k.Kmax:, :int(self.nframes[0] * k.winNr)]
        return cells

    # ------------------------------------------------------------ raster
    def cells_to_sp(self, cells):
        k = self.k
        atomNr = int(k.winNr)
        W = cells[0].shape[1] * atomNr
        sp = np.zeros([int(self.bins * self.octaveNr), W], dtype=complex)
        emptyHops = k.first_center * 1. / k.atomHOP
        for noct in range(int(self.octaveNr)):
            drop = emptyHops * (2 ** (self.octaveNr - noct - 1)) - emptyHops
            r0 = int(self.bins * (self.octaveNr - noct - 1))
            ns = int(2 ** noct)
            cell = cells[noct]
            d = int(drop * ns)
            if atomNr > 1:
                for nb in range(self.bins):
                    for a in range(atomNr):
                        sp[r0 + nb, a * ns:cell.shape[1] * atomNr * ns:atomNr * ns] = \
                            cell[nb * atomNr + a]
                    sp[r0 + nb, :W - d] = sp[r0 + nb, d:].copy()
            else:
                sp[r0:r0 + self.bins, :int((cell.shape[1] - drop) * ns):ns] = cell[:, int(drop):]
            if noct > 0:
                for nb in range(self.bins):
                    row = sp[r0 + nb]
                    kept = row[::ns].copy()
                    row[:] = interp_magnitudes(np.abs(kept), ns, W)
                    row[::ns] = kept
        sp = np.ascontiguousarray(sp[:, :int(self.nframes[0] * k.winNr)])
        if self.kind != 'cqt':
            Wc = sp.shape[1]
            sp = np.vstack([sp, np.zeros([int(k.linBins), Wc], dtype=complex)])
            drop = int(emptyHops * (2 ** (self.octaveNr - 1) - 1))
            sp[int(self.bins * self.octaveNr):, :Wc - drop] = cells['linear'][:, drop:]
        return sp

    def sp_to_cells(self, sp):
        cells = {noct: self.sp_to_cell(sp, noct) for noct in range(int(self.octaveNr))}
        if self.kind != 'cqt':
            cells['linear'] = self.linear_cell(sp)
        return cells

    # ------------------------------------------------------------ inverse
    def inverse(self, cells):
        k = self.k
        K = np.ascontiguousarray(k.sparKernel)
        N = int(k.FFTLen)
        y = np.zeros(int(np.ceil(self.datalen_init / (2. ** (self.octaveNr - 1)))))
        for noct in range(int(self.octaveNr) - 1, -1, -1):
            Y = np.dot(K, cells[noct])
            nframes = cells[noct].shape[1]
            ylen = int(k.fftHOP * (nframes - 1) + k.FFTLen)
            if ylen > y.size:
                y = np.concatenate([y, np.zeros(ylen - y.size)])
            for n in range(nframes):
                a = int(n * k.fftHOP)
                y[a:a + N] += 2. * np.real(np.fft.ifft(Y[:, n], n=N))
            if noct != 0:
                y = self._upsample(y)
        y = y[int(self.prefixZeros):][:int(self.datalen_init)]
        if self.kind != 'cqt':
            y = y + self.inverse_linear(cells)
        return y

    def inverse_linear(self, cells):
        k = self.k
        Y = np.zeros([k.linFTLen // 2 + 1, cells['linear'].shape[1]], dtype=complex)
        Y[k.Kmax:] = cells['linear']
        y = cqt_ref.istft(Y, k.linWindow, k.atomHOP, k.linFTLen)
        y = y[int(self.prefixZeros - self.offsetSTFT):]
        return y[:int(self.datalen_init)]

    def time_stamps(self):
        k = self.k
        return (np.arange(self.nframes[0] * k.winNr) * k.atomHOP +
                k.first_center * 2 ** (self.octaveNr - 1) - self.prefixZeros)
