"""Device plan of one NSGT (include/fasst_nsgt.h): the windows, dual windows
and FFT tables resident on the GPU, and the two transforms on them."""
import ctypes

import numpy as np

from ..._lib import check, default_device, dptr, iptr, lib

NSGT_MAX_N = 1 << 23


def _is_tensor(a):
    return type(a).__module__.split('.')[0] == 'torch'


def _dev_ptr(t):
    return ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_double))


def band_slice(nbands, real, reducedform):
    """The bands a transform with these flags keeps."""
    if real:
        return slice(reducedform, nbands // 2 + 1 - reducedform)
    return slice(0, nbands)


class DevicePlan(object):
    def __init__(self, g, gd, wins, nn, M, Ls, real, reducedform, device=None):
        self.device = default_device() if device is None else int(device)
        self.Ls, self.nn, self.real = int(Ls), int(nn), bool(real)
        nb = len(g)
        sl = band_slice(nb, real, reducedform)
        self.M_used = np.asarray(M[sl], dtype=np.int64)
        self.offsets = np.concatenate(([0], np.cumsum(self.M_used)))
        Mi = np.ascontiguousarray(M, dtype=np.int32)
        Lg = np.array([len(gi) for gi in g], dtype=np.int32)
        start = np.array([int(w[0]) % self.nn for w in wins], dtype=np.int32)
        gp = np.ascontiguousarray(np.concatenate(g), dtype=np.float64)
        gdp = np.ascontiguousarray(np.concatenate(gd), dtype=np.float64)
        self._h = ctypes.c_void_p()
        self._create(nb, Mi, Lg, start, gp, gdp, int(reducedform))
        n = ctypes.c_long(0)
        check(lib.fasst_nsgt_coef_len(self._h, ctypes.byref(n)), "fasst_nsgt_coef_len")
        self.coef_len = n.value
        assert self.coef_len == int(self.offsets[-1])

    def _create(self, nb, Mi, Lg, start, gp, gdp, reducedform):
        check(lib.fasst_nsgt_plan_create(self.device, self.Ls, self.nn, nb, iptr(Mi), iptr(Lg),
                                         iptr(start), dptr(gp), dptr(gdp), int(self.real),
                                         reducedform, ctypes.byref(self._h)),
              "fasst_nsgt_plan_create")

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h and lib is not None:   # lib is gone when the interpreter shuts down
            lib.fasst_nsgt_plan_destroy(h)

    def _check_coef(self, c):
        if c.ndim != 2 or c.shape[1] != self.coef_len:
            raise ValueError("nsgt backward: coefficients of shape %s, expected [nch, %d]"
                             % (tuple(c.shape), self.coef_len))

    # ------------------------------------------------------------- NumPy route
    def forward(self, x):
        """x [nch, Ls] real -> [nch, coef_len] complex128"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        c = np.empty((x.shape[0], self.coef_len), dtype=np.complex128)
        check(lib.fasst_nsgt_forward(self._h, x.shape[0], dptr(x), 0, dptr(c)), "fasst_nsgt_forward")
        return c

    def backward(self, c):
        """c [nch, coef_len] complex -> [nch, Ls], real when the plan is"""
        c = np.ascontiguousarray(c, dtype=np.complex128)
        self._check_coef(c)
        y = np.empty((c.shape[0], self.Ls), dtype=np.float64 if self.real else np.complex128)
        check(lib.fasst_nsgt_backward(self._h, c.shape[0], dptr(c), 0, dptr(y)),
              "fasst_nsgt_backward")
        return y

    # ------------------------------------------------------------ tensor route
    def _tensor_device(self, t):
        import torch
        if t.device.type != 'cuda':
            raise ValueError("nsgt: torch tensors must be on the GPU, got %s" % (t.device,))
        idx = t.device.index if t.device.index is not None else torch.cuda.current_device()
        if idx != self.device:
            raise ValueError("nsgt: the plan lives on device %d, the tensor on %d" % (self.device, idx))
        return torch

    def forward_tensor(self, x):
        torch = self._tensor_device(x)
        x = x.to(torch.float64).contiguous()
        c = torch.empty((x.shape[0], self.coef_len), dtype=torch.complex128, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()
        check(lib.fasst_nsgt_forward(self._h, int(x.shape[0]), _dev_ptr(x), 1, _dev_ptr(c)),
              "fasst_nsgt_forward")
        return c

    def backward_tensor(self, c):
        torch = self._tensor_device(c)
        c = c.to(torch.complex128).contiguous()
        self._check_coef(c)
        y = torch.empty((c.shape[0], self.Ls), dtype=torch.float64 if self.real else torch.complex128,
                        device=c.device)
        torch.cuda.current_stream(c.device).synchronize()
        check(lib.fasst_nsgt_backward(self._h, int(c.shape[0]), _dev_ptr(c), 1, _dev_ptr(y)),
              "fasst_nsgt_backward")
        return y


def fft(x, sign=-1, device=None):
    """out[k] = sum_n x[n] exp(sign 2 pi i n k / N) on the GPU, any N up to the
    ceiling (fasst_nsgt_fft); no scaling."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    out = np.empty_like(x)
    check(lib.fasst_nsgt_fft(default_device() if device is None else int(device), x.size, int(sign),
                             dptr(x), dptr(out)), "fasst_nsgt_fft")
    return out


def launch_count():
    n = ctypes.c_long(0)
    check(lib.fasst_nsgt_launch_count(ctypes.byref(n)), "fasst_nsgt_launch_count")
    return n.value


def set_timing(on):
    check(lib.fasst_nsgt_set_timing(int(bool(on))), "fasst_nsgt_set_timing")


def last_ms():
    """Device time of this thread's last forward / backward: (total, the
    whole-signal FFT's share), in ms."""
    a, b = ctypes.c_double(0), ctypes.c_double(0)
    check(lib.fasst_nsgt_last_ms(ctypes.byref(a), ctypes.byref(b)), "fasst_nsgt_last_ms")
    return a.value, b.value
