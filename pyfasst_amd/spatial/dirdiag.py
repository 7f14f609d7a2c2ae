"""Directivity diagrams of spatial filters (spatial/dirdiag.py of the
reference), on the GPU.  Nothing is drawn: the plotting arguments are accepted
and ignored, and the two functions that only produce figures raise
NotImplementedError.
"""
import numpy as np

from .. import _lib
from .._lib import check, dptr, lib
from ..tools.utils import db
from . import steering_vectors as sv

sound_celerity = 300.  # m/s


def _dev(device):
    return _lib.default_device() if device is None else device


def make_MVDR_filter_target(steering_vec_target, steering_vec_interf, device=None):
    """MVDR spatial filter from estimated steering vectors (dirdiag.py:20-69):
    target [1, n_freqs, 2], interferers [n_interf, n_freqs, 2]; returns the
    [2, n_freqs] complex filter."""
    n_target, n_freqs, n_chans = steering_vec_target.shape
    n_interf, n_freq2, n_chan2 = steering_vec_interf.shape

    if n_freqs != n_freq2 or n_chans != n_chan2:
        raise ValueError("Not the right dim for the steering_vectors")

    if n_chans != 2:
        raise AttributeError("Program only for stereo filters.")

    if n_target != 1:
        raise AttributeError("For now, only for rank-1 spatial target source.")

    t = np.ascontiguousarray(steering_vec_target, dtype=np.complex128)
    s = np.ascontiguousarray(steering_vec_interf, dtype=np.complex128)
    w_filter = np.zeros([n_chans, n_freqs], dtype=np.complex128)
    if n_freqs:
        check(lib.fasst_mvdr_target(_dev(device), n_freqs, n_interf, dptr(t),
                                    dptr(s) if n_interf else None, dptr(w_filter)),
              "fasst_mvdr_target")
    return w_filter


def ula_response(w_filter, freqs, thetas, dist_inter_sensor, device=None):
    """diagram[theta, f] = |sum_m w_filter[m, f] a_m(f, theta) / sqrt(n)|^2 for
    the far-field steering vectors a of a uniform linear array of
    n = w_filter.shape[0] sensors (dirdiag.py:113-121), n <= sv.MAX_SENSORS."""
    w = np.ascontiguousarray(w_filter, dtype=np.complex128)
    freqs = np.ascontiguousarray(freqs, dtype=np.float64).ravel()
    s = sv._sin_each(np.asarray(thetas, dtype=np.float64).ravel())
    n = w.shape[0]
    if w.ndim != 2 or w.shape[1] != freqs.size:
        raise ValueError("w_filter does not have the correct shape.")
    diagram = np.zeros([s.size, freqs.size])
    if diagram.size == 0:
        return diagram
    check(lib.fasst_ula_response(_dev(device), n, freqs.size, s.size, dptr(w), dptr(freqs),
                                 dptr(s), float(dist_inter_sensor / sv.soundCelerity),
                                 dptr(diagram)), "fasst_ula_response")
    return diagram


def directivity_filter_diagram_ULA(n_sensors=2, dist_inter_sensor=.15,
                                   w_filter=None, theta_filter=0,
                                   freqs=None, thetas=None,
                                   nfreqs=256, nthetas=30,
                                   samplerate=8000., doplot='2d',
                                   fig=None, subplot_number=(1, 1, 1),
                                   dyn_func=db, device=None):
    """The directivity diagram of the filter `w_filter` (or of the steering
    vector towards `theta_filter`) for a uniform linear array
    (dirdiag.py:71-154): returns (thetas, freqs, diagram).  doplot, fig,
    subplot_number and dyn_func are accepted and nothing is drawn."""
    if freqs is None:
        freqs = np.arange(nfreqs) * samplerate / (2. * nfreqs)
    else:
        nfreqs = len(freqs)

    if thetas is None:
        thetas = np.arange(-nthetas, nthetas) * np.pi / (2. * nthetas)

    nthetas = len(thetas)

    if w_filter is None:
        w_filter = np.conjugate(sv.gen_steer_vec_far_src_uniform_linear_array(
            freqs=freqs,
            nchannels=n_sensors,
            theta=theta_filter,
            distanceInterMic=dist_inter_sensor, device=device)) / np.sqrt(n_sensors)
    else:
        if w_filter.shape != (n_sensors, nfreqs):
            print("w_filter.shape", w_filter.shape)
            print("expected shape", (n_sensors, nfreqs))
            raise ValueError("w_filter does not have the correct shape.")

    diagram = ula_response(w_filter, freqs, thetas, dist_inter_sensor, device)
    return thetas, freqs, diagram


def producePicDiagramAgainstDistNSensors(*args, **kwargs):
    """The reference's function only draws (dirdiag.py:156-205)."""
    raise NotImplementedError(
        "producePicDiagramAgainstDistNSensors draws with matplotlib, and plotting is outside "
        "this package; call directivity_filter_diagram_ULA() for the diagrams themselves")


def generate_steer_vec_thetas(n_sensors=2, dist_inter_sensors=0.15,
                              freqs=None, n_freqs=256,
                              thetas=None, n_thetas=30,
                              samplerate=8000., computeRaa=False, device=None):
    """A collection of steering vectors A [n_freqs, n_sensors, n_thetas] for the
    array and signal parameters (dirdiag.py:207-243), all angles in one
    launch; with computeRaa also Raa[f] = A[f] A[f]^H."""
    if freqs is None:
        freqs = np.arange(n_freqs) * samplerate / (2. * n_freqs)
    else:
        n_freqs = len(freqs)

    if thetas is None:
        thetas = np.arange(-n_thetas, n_thetas) * np.pi / (2. * n_thetas)

    n_thetas = len(thetas)

    a = sv.steer_ula_batch(freqs, n_sensors, thetas, dist_inter_sensors, device)
    A = np.zeros([n_freqs, n_sensors, n_thetas], dtype=np.complex128)
    for ntheta in range(n_thetas):
        A[:, :, ntheta] = (a[ntheta].T) / np.sqrt(n_sensors)

    if computeRaa:
        Raa = np.zeros([n_freqs, n_sensors, n_sensors], dtype=np.complex128)
        for nfreq in range(n_freqs):
            Raa[nfreq] = np.dot(A[nfreq], np.conjugate(A[nfreq]).T)
        return freqs, thetas, A, Raa
    return freqs, thetas, A


def produceMVDRplots(*args, **kwargs):
    """The reference's function draws, and inverts a rank-deficient Raa with
    numpy.linalg.inv (dirdiag.py:245-327): its filters are rounding noise, so
    there is nothing to reproduce."""
    raise NotImplementedError(
        "produceMVDRplots draws with matplotlib and inverts rank-deficient matrices with "
        "numpy.linalg.inv; use generate_steer_vec_thetas(), make_MVDR_filter_target() and "
        "directivity_filter_diagram_ULA()")
