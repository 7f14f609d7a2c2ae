"""STFT / iSTFT on the GPU (tftransforms/stft.py of the reference).

`stft` and `istft` keep the reference signatures and framing
(stft.py:3-69, :71-131): first frame centred on sample 0 (wlen/2 leading
zeros), ceil(L/hop)+2 frames, window-product normalised overlap-add.  The
FFTs are FP64 radix-2 transforms in LDS (pyfasst_amd/csrc/fasst_tf.hip).

`filter_stft` and `filter_conv_stft` (stft.py:133-227, :229-334) analyse,
filter and overlap-add frame by frame in one kernel
(pyfasst_amd/csrc/fasst_filter.hip); they frame with ceil(L/hop) frames and
return (frames-1) hop + wlen - wlen//2 rows.  torch tensors on the GPU go
through fasst_filter_stft_dev (include/fasst_filter.h) by their device
pointers and a tensor comes back.
"""
import ctypes

import numpy as np

from .. import _lib
from .._lib import check, dptr, lib
from ..tools.utils import sinebell


def _dev(device):
    return _lib.default_device() if device is None else device


def stft(data, window=sinebell(2048), hopsize=256.0, nfft=2048.0, fs=44100.0, device=None):
    """X, F, N = stft(data, window, hopsize, nfft, fs)  (stft.py:3-69)."""
    x = np.ascontiguousarray(np.asarray(data, dtype=np.float64).ravel())
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    nfft_i, hop_i = int(nfft), int(hopsize)
    T = ctypes.c_int(0)
    check(lib.fasst_stft(_dev(device), dptr(x), x.size, dptr(w), w.size, nfft_i, hop_i, None,
                         ctypes.byref(T)), "fasst_stft")
    X = np.empty((nfft_i // 2 + 1, T.value), dtype=np.complex128)
    check(lib.fasst_stft(_dev(device), dptr(x), x.size, dptr(w), w.size, nfft_i, hop_i, dptr(X),
                         ctypes.byref(T)), "fasst_stft")
    F = np.arange(nfft_i // 2 + 1) / np.double(nfft) * fs
    N = np.arange(T.value) * hopsize / np.double(fs)
    return X, F, N


def istft(X, window=sinebell(2048), analysisWindow=None, hopsize=256.0, nfft=2048.0,
          device=None):
    """data = istft(X, window, analysisWindow, hopsize, nfft)  (stft.py:71-131)."""
    if analysisWindow is None:
        analysisWindow = window
    X = np.ascontiguousarray(X, dtype=np.complex128)
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    aw = np.ascontiguousarray(np.asarray(analysisWindow, dtype=np.float64))
    nfft_i, hop_i = int(nfft), int(hopsize)
    if X.shape[0] != nfft_i // 2 + 1:
        raise ValueError("X has %d bins, nfft=%d needs %d" % (X.shape[0], nfft_i, nfft_i // 2 + 1))
    T = X.shape[1]
    y = np.empty(hop_i * (T - 1) + w.size - w.size // 2)
    check(lib.fasst_istft(_dev(device), dptr(X), T, dptr(w), dptr(aw), w.size, nfft_i, hop_i,
                          dptr(y)), "fasst_istft")
    return y


def _int_hop(hopsize):
    if float(hopsize) != int(hopsize):
        raise NotImplementedError("non-integer hopsize %r" % (hopsize,))
    return int(hopsize)


def _windows(analysisWindow, synthWindow):
    # stft.py:147-148, :260-261
    if analysisWindow is None or len(analysisWindow) != len(synthWindow):
        analysisWindow = synthWindow
    return analysisWindow, synthWindow


def _framing(ns, wlen, hop):
    """Frames of stft.py:155-168; the reference's tail padding of negative
    size is NumPy's ValueError."""
    nframes = -(-ns // hop)
    if wlen // 2 + ns > (nframes - 1) * hop + wlen:
        raise ValueError("negative dimensions are not allowed")
    return nframes


def _is_tensor(a):
    return type(a).__module__.split('.')[0] == 'torch'


def _w_frames(W, tv, nframes, frame_major):
    """Frames of a time-varying W; too few is the IndexError of W[..., n]."""
    if not tv:
        if frame_major:
            raise ValueError("w_frame_major needs a time-varying W")
        return 0
    nwf = int(W.shape[-2] if frame_major else W.shape[-1])
    if nwf < nframes:
        raise IndexError("index %d is out of bounds for axis %d with size %d"
                         % (nwf, W.ndim - 1, nwf))
    return nwf


def _dev_ptr(t):
    return ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_double))


def _filter_run_torch(data, n_in, n_out, W, tv, nwf, analysisWindow, synthWindow, hop, nfft,
                      frame_major):
    """The tensor route: every array stays where it lies on the GPU and goes to
    fasst_filter_stft_dev by its device pointer; the result is a tensor on
    that device.  The call waits for the tensors' pending work on torch's
    current stream, runs on the default stream and returns when it has
    finished."""
    import torch
    dev = data.device if _is_tensor(data) else W.device
    if dev.type != 'cuda':
        raise ValueError("filter_stft: torch tensors must be on the GPU, got %s" % (dev,))

    def put(a, dtype):
        if not _is_tensor(a):
            a = torch.as_tensor(np.asarray(a), device=dev)
        return a.to(device=dev, dtype=dtype).contiguous()
    x, w = put(data, torch.float64), put(W, torch.complex128)
    aw, sw = put(analysisWindow, torch.float64), put(synthWindow, torch.float64)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    args = (idx, _dev_ptr(x), int(x.shape[0]), n_in, n_out, _dev_ptr(w), int(tv), nwf, _dev_ptr(aw),
            _dev_ptr(sw), int(sw.shape[0]), nfft, hop)
    n = ctypes.c_int(0)
    check(lib.fasst_filter_stft_dev(*args, None, ctypes.byref(n), int(frame_major), None),
          "fasst_filter_stft")
    y = torch.empty((n.value, n_out), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    check(lib.fasst_filter_stft_dev(*args, _dev_ptr(y), ctypes.byref(n), int(frame_major), None),
          "fasst_filter_stft")
    return y


def _filter_run(data, n_in, n_out, W, tv, nwf, analysisWindow, synthWindow, hop, nfft, device,
                frame_major):
    """data [L, n_in] and W (entries [n_out][n_in], then [F] or [F, nwf], or
    [nwf, F] when frame_major) through fasst_filter_stft / _dev."""
    if _is_tensor(data) or _is_tensor(W):
        return _filter_run_torch(data, n_in, n_out, W, tv, nwf, analysisWindow, synthWindow, hop,
                                 nfft, frame_major)
    if frame_major:
        raise ValueError("w_frame_major is a layout of W on the GPU (a torch tensor)")
    x = np.ascontiguousarray(data, dtype=np.float64)
    w = np.ascontiguousarray(W, dtype=np.complex128)
    aw = np.ascontiguousarray(analysisWindow, dtype=np.float64)
    sw = np.ascontiguousarray(synthWindow, dtype=np.float64)
    n = ctypes.c_int(0)
    args = (_dev(device), dptr(x), int(x.shape[0]), n_in, n_out, dptr(w), int(tv), nwf, dptr(aw),
            dptr(sw), len(sw), nfft, hop)
    check(lib.fasst_filter_stft(*args, None, ctypes.byref(n)), "fasst_filter_stft")
    y = np.empty((n.value, n_out))
    check(lib.fasst_filter_stft(*args, dptr(y), ctypes.byref(n)), "fasst_filter_stft")
    return y


def filter_stft(data, W, analysisWindow=None, synthWindow=sinebell(2048), hopsize=256.0,
                nfft=2048.0, fs=44100.0, device=None, w_frame_major=False):
    """ndata = filter_stft(data, W, ...)  (stft.py:133-227).

    data [T, M]; W [M, M, F] or, one filter per frame, [M, M, F, N], real or
    complex: every frame is analysed, multiplied by W and overlap-added.
    Returns [(ceil(T/hop)-1) hop + wlen - wlen//2, M].

    `data` and `W` may be torch tensors on the GPU (float64; float64 or
    complex128): they are filtered where they lie and a tensor on that device
    is returned.  For those, `w_frame_major=True` says that a time-varying W
    is laid out [M, M, N, F] (each frame's bins contiguous), which spares the
    transpose.  torch must have initialised the GPU before this library's
    first device call in the process.
    """
    ns, nc = data.shape
    if nc != W.shape[0]:
        raise AttributeError("W does not have the right number of channels")
    analysisWindow, synthWindow = _windows(analysisWindow, synthWindow)
    hop, nfft_i = _int_hop(hopsize), int(nfft)
    nframes = _framing(int(ns), len(synthWindow), hop)
    fm = bool(w_frame_major)
    if nfft_i // 2 + 1 != W.shape[3 if fm and W.ndim == 4 else 2]:
        raise AttributeError("W not the right size")
    if W.ndim not in (3, 4):
        raise NotImplementedError("For W.ndim== 3 or 4" + str(W.ndim))
    nwf = _w_frames(W, W.ndim == 4, nframes, fm)
    return _filter_run(data, int(nc), int(W.shape[1]), W, W.ndim == 4, nwf, analysisWindow,
                       synthWindow, hop, nfft_i, device, fm)


def filter_conv_stft(data, W, analysisWindow=None, synthWindow=sinebell(2048), hopsize=256.0,
                     nfft=2048.0, fs=44100.0, verbose=0, device=None, w_frame_major=False):
    """ndata = filter_conv_stft(data, W, ...)  (stft.py:229-334).

    data [T] or [T, 1]; W [M, F] or [M, F, N]: the single channel filtered into
    M channels, [rows, M] as filter_stft.  Tensors on the GPU as in
    filter_stft; `w_frame_major`: W is [M, N, F].
    """
    if (data.ndim == 2 and data.shape[1] != 1) or data.ndim > 2:
        raise AttributeError("provided data should be single channel")
    data = data.reshape(-1, 1)
    nchanout = W.shape[0]
    if verbose:
        print("data.shape", tuple(data.shape), "W.shape", tuple(W.shape))
    analysisWindow, synthWindow = _windows(analysisWindow, synthWindow)
    hop, nfft_i = _int_hop(hopsize), int(nfft)
    nframes = _framing(int(data.shape[0]), len(synthWindow), hop)
    fm = bool(w_frame_major)
    if nfft_i // 2 + 1 != W.shape[2 if fm and W.ndim == 3 else 1]:
        raise AttributeError("W not the right size")
    if W.ndim not in (2, 3):
        raise ValueError("The provided filter does not have the right shape.")
    nwf = _w_frames(W, W.ndim == 3, nframes, fm)
    return _filter_run(data, 1, int(nchanout), W, W.ndim == 3, nwf, analysisWindow, synthWindow,
                       hop, nfft_i, device, fm)


class STFT(object):
    """STFT transform object (stft.py:339-394): computeTransform / invertTransform."""
    transformname = 'stft'

    def __init__(self, linFTLen=2048, atomHopFactor=0.25, winFunc=np.hanning, fs=44100,
                 synthWinFunc=None, device=None, **kwargs):
        fthop = int(linFTLen * atomHopFactor)
        self.ftlen = linFTLen
        self.freqbins = self.ftlen // 2 + 1
        self.atomHopFactor = atomHopFactor
        self.fthop = fthop
        if winFunc is None:
            winFunc = np.hanning
        self.winFunc = winFunc
        self.window = self.winFunc(self.ftlen)
        self.synthWinFunc = synthWinFunc if synthWinFunc is not None else self.winFunc
        self.synthWindow = self.synthWinFunc(self.ftlen)
        self.fs = fs
        self.device = device

    def computeTransform(self, data):
        self.transfo, self.freq_stamps, self.time_stamps = stft(
            data=data, window=self.window, hopsize=self.fthop, fs=self.fs, nfft=self.ftlen,
            device=self.device)
        self.datalen_init = np.asarray(data).size
        self.time_stamps *= self.fs

    def invertTransform(self):
        return istft(X=self.transfo, window=self.synthWindow, analysisWindow=self.window,
                     hopsize=self.fthop, nfft=self.ftlen, device=self.device)[:self.datalen_init]
