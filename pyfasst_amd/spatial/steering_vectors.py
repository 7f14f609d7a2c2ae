"""Steering vectors for arrays of sensors and the Capon directivity diagram
(spatial/steering_vectors.py of the reference), on the GPU.

The reference module cannot run as shipped: it uses `np`, `soundCelerity` and
`inv_mat` without defining them.  Its two far-field functions were cut out of
audioModel.py, which has `import numpy as np` and `soundCelerity = 340.`
(audioModel.py:63), and `inv_mat(meanCx_diag, meanCx_off)` is called with the
signature and the three return values of tools.signalTools.inv_herm_mat_2d.
This port binds exactly those three names: NumPy, soundCelerity = 340. and
the clamped 2 x 2 Hermitian inverse.
"""
import ctypes

import numpy as np

from .. import _lib
from .._lib import check, dptr, lib
from ..engine import Engine

soundCelerity = 340.

KERNELS = ('k_steer_ula', 'k_steer_acous', 'k_cx_tmean', 'k_capon_diagram', 'k_ula_response',
           'k_mvdr_target')
MAX_SENSORS = 64   # FASST_SPATIAL_MAX_SENSORS, the ceiling of ula_response


def _dev(device):
    return _lib.default_device() if device is None else device


def launch_count():
    """{kernel: launches by this process so far} (k_cx_tmean counts its
    partial and its combine launch)."""
    n = (ctypes.c_long * len(KERNELS))()
    check(lib.fasst_spatial_launch_count(n), "fasst_spatial_launch_count")
    return dict(zip(KERNELS, n))


def last_ms():
    """{kernel: device time (HIP events) of its last launch}, without copies."""
    ms = np.zeros(len(KERNELS))
    check(lib.fasst_spatial_last_ms(dptr(ms)), "fasst_spatial_last_ms")
    return dict(zip(KERNELS, ms.tolist()))


def transfer_bytes():
    """Bytes the spatial calls have copied between host and device so far."""
    n = ctypes.c_long(0)
    check(lib.fasst_spatial_transfer_bytes(ctypes.byref(n)), "fasst_spatial_transfer_bytes")
    return n.value


def _model_engine(model):
    if model._engine is None:
        raise AttributeError("no observation: call comp_transf_Cx() first")
    return model._engine


def _sin_each(thetas):
    # one np.sin per angle, as the reference's loops take them
    return np.array([np.sin(t) for t in thetas], dtype=np.float64)


def steer_ula_batch(freqs, nchannels, thetas, distanceInterMic, device=None):
    """gen_steer_vec_far_src_uniform_linear_array for every angle of thetas in
    one launch: [ntheta, nchannels, nfreqs] complex."""
    freqs = np.ascontiguousarray(freqs, dtype=np.float64).ravel()
    s = _sin_each(np.asarray(thetas, dtype=np.float64).ravel())
    nch = int(nchannels)
    out = np.empty((s.size, max(nch, 0), freqs.size), dtype=np.complex128)
    if out.size == 0:
        return out
    check(lib.fasst_steer_ula(_dev(device), nch, freqs.size, s.size, dptr(freqs), dptr(s),
                              float(distanceInterMic / soundCelerity), dptr(out)),
          "fasst_steer_ula")
    return out


def gen_steer_vec_far_src_uniform_linear_array(freqs, nchannels, theta, distanceInterMic,
                                               device=None):
    """Steering vectors of a far source for a uniform linear array
    (steering_vectors.py:11-53): a (nchannels, nfreqs) complex ndarray,
    a[m, f] = exp(-2 pi i m freqs[f] (distanceInterMic / soundCelerity) sin(theta))."""
    return steer_ula_batch(freqs, nchannels, [theta], distanceInterMic, device)[0]


def gen_steer_vec_acous(freqs, dist_src_mic, device=None):
    """Steering vectors for given distances between the source and the
    microphones, with the 1 / (sqrt(4 pi) r) gains (steering_vectors.py:55-74)."""
    freqs = np.ascontiguousarray(freqs, dtype=np.float64).ravel()
    dist = np.ascontiguousarray(dist_src_mic, dtype=np.float64).ravel()
    out = np.empty((dist.size, freqs.size), dtype=np.complex128)
    if out.size == 0:
        return out
    check(lib.fasst_steer_acous(_dev(device), dist.size, freqs.size, dptr(freqs), dptr(dist),
                                float(soundCelerity), dptr(out)), "fasst_steer_acous")
    return out


def cx_tmean(Cx, device=None):
    """Time means of Cx[0], Re Cx[1], Im Cx[1] and Cx[2], [4, F]: a host
    [3, F, T] array is uploaded as a model's observation is and read by the
    same kernel; a FASST model's resident observation is read where it lies."""
    if hasattr(Cx, '_engine'):
        eng = _model_engine(Cx)
        return eng.cx_tmean()
    Cx = np.asarray(Cx)
    if Cx.ndim != 3 or Cx.shape[0] != 3:
        raise ValueError("Cx of shape (3, F, T) expected, got %s" % (Cx.shape,))
    eng = Engine(Cx.shape[1], Cx.shape[2], device)
    try:
        eng.set_cx(Cx)
        return eng.cx_tmean()
    finally:
        eng.close()


def dir_diag_stereo(Cx, nft=2048, ntheta=512, samplerate=44100, distanceInterMic=0.3,
                    device=None):
    """Capon directivity diagram of the second order statistics Cx
    (steering_vectors.py:76-160): returns (directivity_diagram [ntheta, nfreqs],
    theta), nfreqs = nft // 2 + 1.

    Cx is a [3, F, T] array as FASST.Cx hands it out, or a FASST model, whose
    resident observation is then used without moving a plane (nft and
    samplerate are still the caller's).  A singular mean covariance raises the
    reference's ValueError.
    """
    if hasattr(Cx, '_engine'):
        eng = _model_engine(Cx)
        return eng.dir_diag(ntheta, distanceInterMic, nft, samplerate)
    Cx = np.asarray(Cx)
    if Cx.ndim != 3 or Cx.shape[0] != 3:
        raise ValueError("Cx of shape (3, F, T) expected, got %s" % (Cx.shape,))
    eng = Engine(Cx.shape[1], Cx.shape[2], device)
    try:
        eng.set_cx(Cx)
        return eng.dir_diag(ntheta, distanceInterMic, nft, samplerate)
    finally:
        eng.close()
