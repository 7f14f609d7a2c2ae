"""pyfasst_amd.tftransforms.slicq: the sliced NSGT (sliCQ), a constant-Q
transform of a stream of any length with exact reconstruction, on the GPU.

The stream is cut into half-overlapping slices of sl_len samples under a Tukey
window (transitions of tr_area samples); the same small NSGT (a plan with
Ls = sl_len) runs on every slice, each slice one more channel of a batched
device call (include/fasst_nsgt.h); the inverse adds the overlapping halves
back.  Planning is host NumPy, FP64.

The names, signatures, defaults and attributes are those of the NSGT package
by Thomas Grill that the reference ships (slicq.py, slicing.py, unslicing.py,
nsgfwin_sl.py); the code is this project's, written from the formulas.

forward(sig) takes an iterable of blocks of any lengths (1-D arrays, or
[nchan, n] with multichannel=True) and returns a generator with one item per
slice: the list of per-band complex128 vectors (with multichannel=True a tuple
of such lists, one per channel).  The input is consumed lazily,
slices_per_call slices per device call.  A stream of L samples gives
(ceil(L / hhop) + 1) // 2 + 1 slices, hhop = sl_len / 4.

backward(cseq) takes such items and returns a generator of blocks of 2 hhop
samples, one per slice, the two leading padding quarter-blocks already dropped:
concatenated and cut to L they are the signal.

multichannel=True is the single-channel transform applied to each channel (the
reference's own multichannel arm cannot run: its coefficient rotation asserts
one channel).

A torch tensor on the GPU, [L] or [nchan, L], goes in whole: forward returns
(buffer [nslices, (nchan,) coef_len], offsets), band j of a slice at
buffer[..., offsets[j]:offsets[j+1]]; backward of that pair (or of the buffer)
returns a tensor of 2 hhop nslices samples per channel.  Nothing crosses to
the host.
"""
import ctypes
from warnings import warn

import numpy as np

from .._lib import check, dptr, iptr, lib
from .nsgt import _device
from .nsgt.fscale import OctScale
from .nsgt.nsdual import nsdual
from .nsgt.nsgfwin_sl import _inside_band
from .nsgt.util import blackharr, calcwinrange, chkM, hannwin

__all__ = ["NSGT_sliced", "CQ_NSGT_sliced", "nsgfwin_sliced", "nsgtf_sl", "nsigtf_sl",
           "slicing_window", "synthesis_window"]

MAX_PER_CALL = 65535   # slices x channels of one device call (a grid dimension)


# ------------------------------------------------------------------- planning
def nsgfwin_sliced(f, q, sr, sl_len, min_win=16, Qvar=1, dowarn=True):
    """Returns (g, rfbas, M) of the sliced transform: Blackman-Harris windows
    on the two-sided spectrum of sl_len bins, 2 (len(f) + 1) bands.

    Band widths are neighbour distances (the first and last scale bands
    pos / q, the DC band twice the first position), scaled by Qvar / 4,
    rounded, times 4, never below min_win.  A DC or Nyquist band wider than
    its neighbour is a plateau of ones with a Hann window of the neighbour's
    length in its middle.  Positions are rounded to even bins."""
    nyquist = sr / 2.
    f, q = _inside_band(np.asarray(f), np.asarray(q), nyquist)
    if len(f) != len(q) or np.any(np.diff(f) <= 0) or np.any(q <= 0):
        raise ValueError("nsgfwin_sliced: frequencies must increase and every Q be positive")
    too_sharp = q >= f * (sl_len / (8. * sr))
    if dowarn and np.any(too_sharp):
        warn("Q-factor too high for frequencies %s" % ",".join("%.2f" % x for x in f[too_sharp]))

    n = len(f)                       # scale bands; DC at 0, Nyquist at n + 1
    hz = np.concatenate(((0.,), f, (nyquist,), sr - f[::-1]))
    pos = hz * (float(sl_len) / sr)

    width = np.zeros(len(pos))
    width[0] = 2 * pos[1]
    width[1] = pos[1] / q[0]
    inner = list(range(2, n)) + [n + 1]
    for k in inner:
        width[k] = pos[k + 1] - pos[k - 1]
    width[n] = pos[n] / q[n - 1]
    width[n + 2:] = width[n:0:-1]    # the mirror images
    width *= Qvar / 4.
    M = np.maximum(np.round(width).astype(int) * 4, min_win)

    g = [blackharr(m) for m in M]
    for edge, neighbour in ((0, 1), (n + 1, n + 2)):
        if M[edge] > M[neighbour]:
            w = np.ones(M[edge])
            mid, m = M[edge] // 2, M[neighbour]
            w[mid - m // 2:mid + (m + 1) // 2] = hannwin(m)
            g[edge] = w
    rfbas = np.round(pos / 2.).astype(int) * 2
    return g, rfbas, M


def slicing_window(sl_len, tr_area):
    """The Tukey window of one slice: zeros, a rising half-Hann of tr_area
    samples centred on sl_len/4, ones, the falling half centred on 3 sl_len/4,
    zeros."""
    hhop, htr = sl_len // 4, tr_area // 2
    tw = np.zeros(sl_len)
    tw[hhop + htr:3 * hhop - htr] = 1
    if tr_area:
        w = hannwin(2 * tr_area)
        tw[hhop - htr:hhop + htr] = w[tr_area:]
        tw[3 * hhop - htr:3 * hhop + htr] = w[:tr_area]
    return tw


def synthesis_window(sl_len, tr_area):
    """The window of recwnd=True: ones over the slicing window's support,
    half-Hann slopes of min(sl_len/2 - tr_area, 2 tr_area) / 2 samples outside."""
    hhop, htr = sl_len // 4, tr_area // 2
    htr2 = min(2 * hhop - tr_area, 2 * tr_area) // 2
    tw = np.zeros(sl_len)
    tw[hhop - htr:3 * hhop + htr] = 1
    if htr2:
        hw = hannwin(2 * htr2)
        tw[hhop - htr - htr2:hhop - htr] = hw[htr2:]
        tw[3 * hhop + htr:3 * hhop + htr + htr2] = hw[:htr2]
    return tw


# --------------------------------------------------------------------- device
class SlicedDevicePlan(_device.DevicePlan):
    """The plan of one slice (Ls = sl_len) with the slicing and synthesis
    windows, and the batched calls over slices."""

    def __init__(self, g, gd, wins, nn, M, sl_len, tr_area, real, reducedform, recwnd, device=None):
        self.sl_len, self.tr_area, self.hhop = int(sl_len), int(tr_area), int(sl_len) // 4
        self._slwnd = np.ascontiguousarray(slicing_window(sl_len, tr_area))
        self._recwnd = np.ascontiguousarray(synthesis_window(sl_len, tr_area)) if recwnd else None
        _device.DevicePlan.__init__(self, g, gd, wins, nn, M, sl_len, real, reducedform, device)

    def _create(self, nb, Mi, Lg, start, gp, gdp, reducedform):
        check(lib.fasst_nsgt_sliced_plan_create(
            self.device, self.sl_len, self.tr_area, self.nn, nb, iptr(Mi), iptr(Lg), iptr(start),
            dptr(gp), dptr(gdp), int(self.real), reducedform, dptr(self._slwnd),
            dptr(self._recwnd) if self._recwnd is not None else None, ctypes.byref(self._h)),
            "fasst_nsgt_sliced_plan_create")

    @property
    def out_dtype(self):
        return np.float64 if self.real else np.complex128

    # NumPy route
    def slices_forward(self, blocks, first):
        """blocks [nchan, (2 n + 2) hhop]: the stream's quarter-blocks 2 first
        .. 2 (first + n) + 1  ->  [n, nchan, coef_len]"""
        blocks = np.ascontiguousarray(blocks, dtype=np.float64)
        nchan, n = blocks.shape[0], blocks.shape[1] // (2 * self.hhop) - 1
        c = np.empty((n, nchan, self.coef_len), dtype=np.complex128)
        check(lib.fasst_nsgt_sliced_forward(self._h, nchan, n, int(first), dptr(blocks),
                                            blocks.shape[1], 0, dptr(c)),
              "fasst_nsgt_sliced_forward")
        return c

    def slices_backward(self, c, carry, first):
        """c [n, nchan, coef_len], carry [nchan, 2 hhop] (updated in place)  ->
        [nchan, 2 n hhop]: the stream's quarter-blocks 2 first .. 2 (first + n) - 1"""
        c = np.ascontiguousarray(c, dtype=np.complex128)
        if c.ndim != 3 or c.shape[2] != self.coef_len:
            raise ValueError("sliced backward: coefficients of shape %s, expected [n, nchan, %d]"
                             % (tuple(c.shape), self.coef_len))
        n, nchan = c.shape[:2]
        y = np.empty((nchan, 2 * n * self.hhop), dtype=self.out_dtype)
        check(lib.fasst_nsgt_sliced_backward(self._h, nchan, n, int(first), dptr(c), dptr(carry), 0,
                                             dptr(y), y.shape[1]),
              "fasst_nsgt_sliced_backward")
        return y

    # tensor route: views of whole-stream tensors, addressed by pointer and stride
    def slices_forward_tensor(self, padded, coef, first, n):
        torch = self._tensor_device(padded)
        nchan, stride = padded.shape[0], padded.stride(0)
        ptr = padded.data_ptr() + 8 * 2 * first * self.hhop
        torch.cuda.current_stream(padded.device).synchronize()
        check(lib.fasst_nsgt_sliced_forward(
            self._h, nchan, n, int(first), ctypes.cast(ctypes.c_void_p(ptr), _DP), stride, 1,
            _device._dev_ptr(coef[first])), "fasst_nsgt_sliced_forward")

    def slices_backward_tensor(self, coef, carry, out, first, n):
        torch = self._tensor_device(coef)
        nchan, stride = out.shape[0], out.stride(0)
        ptr = out.data_ptr() + out.element_size() * 2 * first * self.hhop
        torch.cuda.current_stream(coef.device).synchronize()
        check(lib.fasst_nsgt_sliced_backward(
            self._h, nchan, n, int(first), _device._dev_ptr(coef[first]), _device._dev_ptr(carry), 1,
            ctypes.cast(ctypes.c_void_p(ptr), _DP), stride), "fasst_nsgt_sliced_backward")


_DP = ctypes.POINTER(ctypes.c_double)


def _chunks(it, n):
    """Lists of up to n consecutive items of an iterable, lazily."""
    group = []
    for x in it:
        group.append(x)
        if len(group) == n:
            yield group
            group = []
    if group:
        yield group


# -------------------------------------------------------------------- surface
class NSGT_sliced(object):
    """The sliced transform on `scale` at rate fs: slices of sl_len samples
    (a multiple of 4), Tukey transitions of tr_area samples (even, below
    sl_len / 2).

    min_win      the narrowest window, in bins; where it binds it must be a
                 multiple of 4 (every M is: the slices' band rotations by M/4
                 and 3M/4 undo each other only then)
    Qvar         scales every band's width
    real         the signal is real: only the bands from DC to Nyquist are
                 kept, less `reducedform` bands at either end (0, 1 or 2)
    recwnd       the inverse multiplies each slice by a synthesis window before
                 the overlapping halves are added (default: plain addition)
    matrixform   every kept band gets the largest number of time channels
    multichannel blocks are [nchan, n]; the single-channel transform of each
                 channel, items are tuples over the channels
    measurefft   accepted and ignored (there is no FFT planner to tune)
    slices_per_call  slices of one device call; results do not depend on it
    """

    def __init__(self, scale, sl_len, tr_area, fs, min_win=16, Qvar=1, real=False, recwnd=False,
                 matrixform=False, reducedform=0, multichannel=False, measurefft=False, *,
                 slices_per_call=256):
        if not (fs > 0 and sl_len > 0 and min_win > 0):
            raise ValueError("NSGT_sliced: fs, sl_len and min_win must be positive, got %r, %r, %r"
                             % (fs, sl_len, min_win))
        if sl_len % 4:
            raise ValueError("NSGT_sliced: sl_len = %r is not a multiple of 4 (the slices are cut "
                             "in quarters)" % (sl_len,))
        if tr_area < 0 or tr_area % 2 or sl_len <= 2 * tr_area:
            raise ValueError("NSGT_sliced: tr_area = %r must be even, not negative and below "
                             "sl_len / 2 = %r" % (tr_area, sl_len // 2))
        if reducedform not in (0, 1, 2):
            raise ValueError("NSGT_sliced: reducedform is 0, 1 or 2, got %r" % (reducedform,))
        if int(slices_per_call) < 1:
            raise ValueError("NSGT_sliced: slices_per_call must be at least 1")
        if int(sl_len) > _device.NSGT_MAX_N:
            raise NotImplementedError("NSGT_sliced: sl_len = %d is above the device FFT's ceiling "
                                      "of %d points" % (sl_len, _device.NSGT_MAX_N))
        self.sl_len, self.tr_area, self.fs = sl_len, tr_area, fs
        self.real, self.measurefft, self.userecwnd = real, measurefft, recwnd
        self.reducedform, self.multichannel = reducedform, multichannel
        self.slices_per_call = int(slices_per_call)
        self.hhop = sl_len // 4

        self.scale = scale
        self.frqs, self.q = scale()
        self.g, self.rfbas, self.M = nsgfwin_sliced(self.frqs, self.q, fs, sl_len, min_win=min_win,
                                                    Qvar=Qvar)
        if matrixform:
            kept = self.M[_device.band_slice(len(self.M), True, reducedform)] if reducedform \
                else self.M
            self.M[:] = kept.max()
        if np.any(self.M % 4):
            raise ValueError("NSGT_sliced: band lengths M = %s are no multiples of 4 (min_win = %r "
                             "binds): rotating a band by M/4 and by 3M/4 would not undo each other"
                             % (sorted(set(int(m) for m in self.M[self.M % 4 != 0])), min_win))
        self.wins, self.nn = calcwinrange(self.g, self.rfbas, sl_len)
        self.gd = nsdual(self.g, self.wins, self.nn, self.M)
        if max(int(self.nn), int(self.M.max())) > _device.NSGT_MAX_N:
            raise NotImplementedError("NSGT_sliced: nn = %d or the largest M = %d is above the "
                                      "device FFT's ceiling of %d points"
                                      % (self.nn, self.M.max(), _device.NSGT_MAX_N))
        self._plan = None

    @property
    def plan(self):
        """The device plan, built at the first transform and kept."""
        if self._plan is None:
            self._plan = SlicedDevicePlan(self.g, self.gd, self.wins, self.nn, self.M, self.sl_len,
                                          self.tr_area, self.real, self.reducedform, self.userecwnd)
        return self._plan

    def nslices(self, L):
        """Slices of a stream of L samples."""
        return (-(-int(L) // self.hhop) + 1) // 2 + 1

    def _per_call(self, nchan):
        n = min(self.slices_per_call, MAX_PER_CALL // nchan)
        if n < 1:
            raise ValueError("NSGT_sliced: %d channels are above %d a call" % (nchan, MAX_PER_CALL))
        return n

    # ---------------------------------------------------------------- forward
    def forward(self, sig):
        'transform - sig: iterable of blocks (or one GPU tensor)'
        if _device._is_tensor(sig):
            return self._forward_tensor(sig)
        return self._forward_stream(sig)

    def _runs(self, sig):
        """The zero-padded stream in runs [nchan, (2 n + 2) hhop] of quarter-
        blocks, two of them shared by consecutive runs: (first slice, run)."""
        hhop = self.hhop
        pieces, have, L, nchan, first = [], 2 * hhop, 0, None, 0
        for blk in sig:
            blk = np.asarray(blk, dtype=np.float64)
            blk = blk if self.multichannel else blk[None]
            if blk.ndim != 2:
                raise ValueError("NSGT_sliced.forward: a block of shape %s" % (blk.shape,))
            if nchan is None:
                nchan = blk.shape[0]
                per = self._per_call(nchan)
                pieces.append(np.zeros((nchan, 2 * hhop)))
            elif blk.shape[0] != nchan:
                raise ValueError("NSGT_sliced.forward: a block of %d channels after blocks of %d"
                                 % (blk.shape[0], nchan))
            pieces.append(blk)
            have += blk.shape[1]
            L += blk.shape[1]
            if have >= (2 * per + 2) * hhop:
                buf = np.concatenate(pieces, axis=1)
                while buf.shape[1] >= (2 * per + 2) * hhop:
                    yield first, buf[:, :(2 * per + 2) * hhop]
                    first += per
                    buf = buf[:, 2 * per * hhop:]
                pieces, have = [buf], buf.shape[1]
        if not L:
            raise ValueError("NSGT_sliced.forward: the signal is empty")
        left = self.nslices(L) - first
        buf = np.zeros((nchan, (2 * left + 2) * hhop))
        tail = np.concatenate(pieces, axis=1)
        buf[:, :tail.shape[1]] = tail
        while left > 0:
            n = min(per, left)
            yield first, buf[:, :(2 * n + 2) * hhop]
            first += n
            left -= n
            buf = buf[:, 2 * n * hhop:]

    def _forward_stream(self, sig):
        o = self.plan.offsets
        for first, run in self._runs(sig):
            c = self.plan.slices_forward(run, first)
            for cs in c:
                item = tuple([row[o[j]:o[j + 1]].copy() for j in range(len(o) - 1)] for row in cs)
                yield item if self.multichannel else item[0]

    def _forward_tensor(self, x):
        import torch
        x = x if self.multichannel else x[None]
        if x.ndim != 2 or x.shape[1] < 1:
            raise ValueError("NSGT_sliced.forward: a tensor of shape %s" % (tuple(x.shape),))
        nchan, L = int(x.shape[0]), int(x.shape[1])
        N, per, hhop = self.nslices(L), self._per_call(nchan), self.hhop
        padded = torch.zeros((nchan, (2 * N + 2) * hhop), dtype=torch.float64, device=x.device)
        padded[:, 2 * hhop:2 * hhop + L] = x
        coef = torch.empty((N, nchan, self.plan.coef_len), dtype=torch.complex128, device=x.device)
        for first in range(0, N, per):
            self.plan.slices_forward_tensor(padded, coef, first, min(per, N - first))
        return (coef if self.multichannel else coef[:, 0]), self.plan.offsets

    # --------------------------------------------------------------- backward
    def backward(self, cseq):
        'inverse transform - cseq: iterable of per-slice coefficients (or a GPU tensor)'
        if isinstance(cseq, tuple) and len(cseq) == 2 and _device._is_tensor(cseq[0]):
            cseq = cseq[0]
        if _device._is_tensor(cseq):
            return self._backward_tensor(cseq)
        return self._backward_stream(cseq)

    def _backward_stream(self, cseq):
        hhop, nbands = self.hhop, len(self.plan.M_used)
        carry, first, per = None, 0, self.slices_per_call
        for group in _chunks(cseq, per):
            chans = [item if self.multichannel else (item,) for item in group]
            for it in chans:
                for ch in it:
                    if len(ch) != nbands:
                        raise ValueError("NSGT_sliced.backward: a slice of %d bands, expected %d"
                                         % (len(ch), nbands))
            c = np.array([[np.concatenate([np.asarray(b, dtype=np.complex128) for b in ch])
                           for ch in it] for it in chans])
            if carry is None:
                nchan = c.shape[1]
                sub = self._per_call(nchan)
                carry = np.zeros((nchan, 2 * hhop), dtype=self.plan.out_dtype)
            for a in range(0, len(c), sub):
                y = self.plan.slices_backward(c[a:a + sub], carry, first + a)
                for b in range(0 if first + a else 1, y.shape[1] // (2 * hhop)):
                    blk = y[:, 2 * b * hhop:2 * (b + 1) * hhop].copy()
                    yield blk if self.multichannel else blk[0]
            first += len(c)
        if carry is not None:
            yield carry if self.multichannel else carry[0]

    def _backward_tensor(self, coef):
        import torch
        coef = (coef if self.multichannel else coef[:, None]).to(torch.complex128).contiguous()
        if coef.ndim != 3 or coef.shape[2] != self.plan.coef_len:
            raise ValueError("NSGT_sliced.backward: coefficients of shape %s, expected "
                             "[nslices, nchan, %d]" % (tuple(coef.shape), self.plan.coef_len))
        N, nchan, hhop = int(coef.shape[0]), int(coef.shape[1]), self.hhop
        per = self._per_call(nchan)
        dt = torch.float64 if self.real else torch.complex128
        out = torch.empty((nchan, (2 * N + 2) * hhop), dtype=dt, device=coef.device)
        carry = torch.zeros((nchan, 2 * hhop), dtype=dt, device=coef.device)
        for first in range(0, N, per):
            self.plan.slices_backward_tensor(coef, carry, out, first, min(per, N - first))
        out[:, 2 * N * hhop:] = carry
        y = out[:, 2 * hhop:]
        return y if self.multichannel else y[0]


class CQ_NSGT_sliced(NSGT_sliced):
    """NSGT_sliced on the constant-Q scale of `bins` bands per octave from fmin
    to fmax."""

    def __init__(self, fmin, fmax, bins, sl_len, tr_area, fs, min_win=16, Qvar=1, real=False,
                 recwnd=False, matrixform=False, reducedform=0, multichannel=False,
                 measurefft=False, *, slices_per_call=256):
        if not (0 < fmin < fmax and bins > 0):
            raise ValueError("CQ_NSGT_sliced: need 0 < fmin < fmax and bins > 0, got %r, %r, %r"
                             % (fmin, fmax, bins))
        self.fmin, self.fmax, self.bins = fmin, fmax, bins
        NSGT_sliced.__init__(self, OctScale(fmin, fmax, bins), sl_len, tr_area, fs, min_win, Qvar,
                             real, recwnd, matrixform, reducedform, multichannel, measurefft,
                             slices_per_call=slices_per_call)


# ----------------------------------------------------------- functional forms
_BATCH = 256


def nsgtf_sl(f_slices, g, wins, nn, M=None, real=False, reducedform=0, measurefft=False):
    """Generator over already-cut slices (1-D arrays of one length): each
    slice's coefficient bands under the windows g, no rotation; up to 256
    slices share a device call."""
    M = chkM(M, g)
    plan = None
    for group in _chunks(f_slices, _BATCH):
        x = np.array([np.asarray(f, dtype=np.float64) for f in group])
        if plan is None:
            plan = _device.DevicePlan(g, g, wins, nn, M, x.shape[1], real, reducedform)
        o = plan.offsets
        for row in plan.forward(x):
            yield [row[o[j]:o[j + 1]].copy() for j in range(len(o) - 1)]


def nsigtf_sl(cseq, gd, wins, nn, Ls=None, real=False, reducedform=0, measurefft=False):
    """Generator over coefficient slices: each slice's signal of Ls samples
    under the dual windows gd, no rotation; up to 256 slices share a device
    call."""
    Ls = nn if Ls is None else Ls
    nb = len(gd)
    plan = None
    for group in _chunks(cseq, _BATCH):
        if plan is None:
            M = np.zeros(nb, dtype=int)
            M[_device.band_slice(nb, real, reducedform)] = [len(ci) for ci in group[0]]
            if real:   # the mirrored bands borrow the lengths of their sources
                for k in range(nb // 2 + 1, nb):
                    M[k] = M[nb - k]
            plan = _device.DevicePlan(gd, gd, wins, nn, np.maximum(M, 1), Ls, real, reducedform)
        buf = np.array([np.concatenate([np.asarray(ci, dtype=np.complex128) for ci in c])
                        for c in group])
        for y in plan.backward(buf):
            yield y.copy()
