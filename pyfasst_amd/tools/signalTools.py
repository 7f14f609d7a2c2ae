"""Signal tools on the GPU (tools/signalTools.py of the reference)."""
import ctypes
import warnings

import numpy as np

from .. import _lib
from .._lib import check, dptr, iptr, lib

eps = 1e-10  # signalTools.py:11


def _dev(device):
    return _lib.default_device() if device is None else device


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def launch_count():
    """Kernels of the signal tools launched by this process so far."""
    n = ctypes.c_long(0)
    check(lib.sig_launch_count(ctypes.byref(n)), "sig_launch_count")
    return n.value


def last_ms():
    """Device time (HIP events) of the kernels of the last call, without copies."""
    ms = np.zeros(1)
    check(lib.sig_last_ms(dptr(ms)), "sig_last_ms")
    return float(ms[0])


def medianFilter(inputArray, length=10, device=None):
    """Median filter (signalTools.py:13-24), on the GPU.

    The reference's windows with their quirks: output n is the median of
    inputArray[max(n - length, 0):min(n + length, N - 1)], so the last sample
    is in no window and N = 1 has an empty one; an empty window or one that
    holds a NaN returns the input sample.  Bit-equal to the reference for a
    float64 input.  Other real dtypes are filtered in float64 and converted
    back as the reference's assignment into zeros_like(inputArray) does
    (integers truncate); a float32 mean of two middle values can differ from
    the reference's in its last bit.  One-dimensional input and length >= 0
    only (the reference's slices mean something else otherwise).
    """
    x = np.asarray(inputArray)
    if x.ndim != 1 or np.iscomplexobj(x):
        raise ValueError("medianFilter: a real one-dimensional array, not %s %s"
                         % (x.dtype, x.shape))
    if int(length) != length or length < 0:
        raise ValueError("medianFilter: length %r is not an integer >= 0" % (length,))
    if x.size == 0:
        return np.zeros_like(x)
    return median_rows(x[None], length, device)[0].astype(x.dtype)


def median_rows(rows, length=10, device=None):
    """medianFilter of every row of a [R, N] array in one launch (float64)."""
    x = _f64(rows)
    if x.ndim != 2:
        raise ValueError("median_rows: a [R, N] array, not %s" % (x.shape,))
    out = np.empty_like(x)
    check(lib.sig_median(_dev(device), x.shape[0], x.shape[1], int(min(length, 2 ** 31 - 1)),
                         dptr(x), dptr(out)), "sig_median")
    return out


def prinComp2D(X0, X1, neighborNb=10, verbose=0, device=None):
    """Eigenvalues and eigenvectors of the 2 x 2 covariance of (X0, X1) over a
    temporal neighbourhood of neighborNb frames (signalTools.py:26-118), on
    the GPU.

    Returns (lambdaM, lambdam, vM, vm): [F, L] real and [2, F, L] complex,
    L = N - neighborNb + 1.  The window sums are direct sums where the
    reference uses fftconvolve; everything after them is the reference's
    closed form, den == 0 replacements included.  The reference's warnings
    for a negative eigenvalue are raised from two device flags (they name the
    count no more: the planes are not searched on the host).
    """
    X0 = np.asarray(X0)
    X1 = np.asarray(X1)
    if X0.ndim != 2 or X1.ndim != 2 or X0.shape != X1.shape:
        raise ValueError("X1 and X2 of size " + str(X0.shape) + ' and ' + str(X1.shape))
    F, N = X0.shape
    nb = int(neighborNb)
    if nb != neighborNb or nb < 1 or nb > N:
        # the reference's np.zeros([F, N - neighborNb + 1]) raises the same
        raise ValueError("prinComp2D: neighborNb %r outside 1 .. N = %d" % (neighborNb, N))
    L = N - nb + 1
    x0 = np.ascontiguousarray(X0, dtype=np.complex128)
    x1 = np.ascontiguousarray(X1, dtype=np.complex128)
    lambdaM = np.empty((F, L))
    lambdam = np.empty((F, L))
    vM = np.empty((2, F, L), dtype=np.complex128)
    vm = np.empty((2, F, L), dtype=np.complex128)
    flags = np.zeros(2, dtype=np.int32)
    if F > 0:
        check(lib.sig_pca2d(_dev(device), F, N, nb, dptr(x0), dptr(x1), dptr(lambdaM),
                            dptr(lambdam), dptr(vM), dptr(vm), iptr(flags)), "sig_pca2d")
    if flags[0]:
        warnings.warn("lambdaM is negative")
    if flags[1]:
        warnings.warn("lambdam is negative")
    return lambdaM, lambdam, vM, vm


def invHermMat2D(a_00, a_01, a_11, device=None):
    """Inverse of a set of 2 x 2 Hermitian matrices (signalTools.py:120-131),
    element-wise on the GPU: det = a_00 a_11 - |a_01|^2 with no floor (see
    inv_herm_mat_2d for the floored one), returns (a_11/det, -a_01/det,
    a_00/det), bit-equal to the reference.  The diagonals are real; a_01 may
    be real or complex, and the middle output has its kind.
    """
    a00, a01, a11 = np.asarray(a_00), np.asarray(a_01), np.asarray(a_11)
    if np.iscomplexobj(a00) or np.iscomplexobj(a11):
        raise ValueError("invHermMat2D: the diagonal of a Hermitian matrix is real")
    shape = np.broadcast(a00, a01, a11).shape
    cplx = np.iscomplexobj(a01)
    n = int(np.prod(shape)) if len(shape) else 1
    d0 = _f64(np.broadcast_to(a00, shape)).reshape(-1)
    d1 = _f64(np.broadcast_to(a11, shape)).reshape(-1)
    off = np.ascontiguousarray(np.broadcast_to(a01, shape),
                               dtype=np.complex128 if cplx else np.float64).reshape(-1)
    i00, i11, i01 = np.empty(n), np.empty(n), np.empty_like(off)
    nzero = np.zeros(1, dtype=np.int32)
    if n > 0:
        check(lib.sig_invherm(_dev(device), n, int(cplx), dptr(d0), dptr(off), dptr(d1),
                              dptr(i00), dptr(i01), dptr(i11), iptr(nzero)), "sig_invherm")
    if nzero[0]:
        warnings.warn("The matrix is probably non invertible! %s" % str(np.zeros(nzero[0])))
    if not len(shape):
        return i00.reshape(shape)[()], i01.reshape(shape)[()], i11.reshape(shape)[()]
    return i00.reshape(shape), i01.reshape(shape), i11.reshape(shape)


def f0_table(f0min=80, f0max=3000, stepnote=16):
    """The F0 grid of f0detectionFunction (signalTools.py:226-234)."""
    F0number = np.ceil((12. * stepnote) * np.log2(f0max / f0min))
    return f0min * (2. ** (np.arange(F0number) / (12. * stepnote)))


def _harmonic_test(freqs, nh, f0, threshold):
    # signalTools.py:273-275, the reference's expression
    with np.errstate(divide='ignore', invalid='ignore'):
        return (np.abs(12 * np.log2(freqs / (nh * f0)))) < threshold


def harmonic_bins(freqs, F0Table, numberHarmonics, threshold):
    """The bins f0detectionFunction selects (signalTools.py:272-275) as a CSR
    list: harmonic nh of F0Table[i] owns bin_idx[bin_ptr[i * numberHarmonics +
    nh - 1]:bin_ptr[i * numberHarmonics + nh]].

    Every bin kept has passed the reference's own expression on the host, so
    the selection is the reference's exactly.  For an increasing frequency
    axis the expression is only evaluated near the analytic interval
    nh f0 2^(-+threshold/12) (two bins of margin on either side, far more
    than its rounding can move a bound); any other axis takes the full test.
    """
    freqs = np.asarray(freqs, dtype=np.float64)
    F0Table = np.asarray(F0Table, dtype=np.float64)
    NH = int(numberHarmonics)
    nhs = np.arange(1, NH + 1)
    centres = (nhs[None, :] * F0Table[:, None]).reshape(-1)  # nh * f0, as the reference forms it
    monotone = (freqs.size > 1 and np.all(np.isfinite(freqs)) and np.all(np.diff(freqs) > 0)
                and np.all(np.isfinite(centres)) and np.all(centres > 0)
                and np.isfinite(threshold))
    if not monotone:
        ptr = [0]
        idx = []
        for f0 in F0Table:
            for nh in range(1, NH + 1):
                sel = np.flatnonzero(_harmonic_test(freqs, nh, f0, threshold))
                idx.append(sel)
                ptr.append(ptr[-1] + sel.size)
        idx = np.concatenate(idx) if idx else np.zeros(0)
        return np.asarray(ptr, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    half = 2. ** (max(threshold, 0.) / 12.)
    lo = np.maximum(np.searchsorted(freqs, centres / half, 'left') - 2, 0)
    hi = np.minimum(np.searchsorted(freqs, centres * half, 'right') + 2, freqs.size)
    cnt = np.maximum(hi - lo, 0)
    seg = np.repeat(np.arange(centres.size), cnt)
    start = np.cumsum(cnt) - cnt
    cand = np.arange(cnt.sum()) - np.repeat(start, cnt) + np.repeat(lo, cnt)
    keep = _harmonic_test(freqs[cand], 1, centres[seg], threshold)
    kept = np.bincount(seg[keep], minlength=centres.size)
    ptr = np.concatenate([[0], np.cumsum(kept)])
    if ptr[-1] > 2 ** 31 - 1:
        raise ValueError("harmonic_bins: %d selected bins exceed an int" % ptr[-1])
    return ptr.astype(np.int32), np.ascontiguousarray(cand[keep], dtype=np.int32)


def f0detectionFunction(TFmatrix, freqs=None, axis=None,
                        samplingrate=44100, fouriersize=2048,
                        f0min=80, f0max=3000, stepnote=16,
                        numberHarmonics=20, threshold=0.5,
                        detectFunc=np.sum, weightFreqs=None,
                        debug=False, device=None):
    """Harmonic sum / product F0 salience (signalTools.py:198-318), on the GPU.

    Returns (hs, F0Table): hs[i, t] is detectFunc over the harmonics nh of
    F0Table[i] that own at least one bin within `threshold` semitones of
    nh * f0, of max_bins(weightFreqs * TFmatrix[:, t]) / TFmatrix[:, t].sum();
    0 where no harmonic owns a bin.  The F0 table and the bin selection are
    computed on the host with the reference's expressions (harmonic_bins), the
    maxima and sums on the device.

    What is kept of the reference's text, and what is not:

    * `detectFunc` is np.sum or np.prod; anything else raises
      NotImplementedError naming it.
    * `debug=True` only prints shapes and intermediate arrays in the
      reference (:276-301, nothing is plotted or returned), so it raises
      NotImplementedError here too.  The "No freq bins for f0" / "No input
      for f0" lines the reference prints for harmonics past the last bin are
      not printed.
    * The reference is Python 2 text: with its integer defaults f0max / f0min
      floor-divides there (1001 F0s).  Here, as in the Python 3 translation
      the fixtures come from, it is a true division (1004 F0s for the
      defaults); float arguments give the same table under both.
    * One-dimensional input (ndim == 1, one frame): the reference's outer
      product (:281) only yields a result when no harmonic owns more than one
      bin, and raises ValueError otherwise; so does this function.
    * `axis` is accepted and, as in the reference, not used.
    """
    if detectFunc is np.sum:
        prod = 0
    elif detectFunc is np.prod:
        prod = 1
    else:
        raise NotImplementedError("f0detectionFunction: detectFunc %r (np.sum and np.prod run "
                                  "on the GPU)" % (detectFunc,))
    if debug:
        raise NotImplementedError("f0detectionFunction: debug=True only prints intermediate "
                                  "arrays in the reference")
    TF = np.asarray(TFmatrix)
    if TF.ndim not in (1, 2) or np.iscomplexobj(TF):
        raise ValueError("f0detectionFunction: a real vector or matrix, not %s %s"
                         % (TF.dtype, TF.shape))
    one_d = TF.ndim == 1
    tf = _f64(TF.reshape(-1, 1) if one_d else TF)
    nfreqs, nframes = tf.shape
    if freqs is None:
        # assuming STFT
        freqs = np.arange(nfreqs) * samplingrate / np.double(fouriersize)
    freqs = np.asarray(freqs, dtype=np.float64)
    if weightFreqs is None:
        weightFreqs = np.ones(nfreqs)
    w = _f64(weightFreqs)
    if freqs.shape != (nfreqs,) or w.shape != (nfreqs,):
        raise ValueError("f0detectionFunction: freqs %s and weightFreqs %s for %d bins"
                         % (freqs.shape, w.shape, nfreqs))
    F0Table = f0_table(f0min, f0max, stepnote)
    NF0, NH = F0Table.size, int(numberHarmonics)
    hs = np.zeros([NF0, nframes])
    if NF0 == 0 or NH < 1 or nframes == 0 or nfreqs == 0:
        return hs, F0Table
    ptr, idx = harmonic_bins(freqs, F0Table, NH, threshold)
    if one_d and np.any(np.diff(ptr) > 1):
        raise ValueError("f0detectionFunction: one-dimensional input with more than one bin "
                         "for a harmonic (the reference's outer product has no result there)")
    idx_arg = idx if idx.size else np.zeros(1, dtype=np.int32)
    check(lib.sig_hsum(_dev(device), nfreqs, nframes, NF0, NH, dptr(tf), dptr(w), iptr(ptr),
                       iptr(idx_arg), prod, dptr(hs)), "sig_hsum")
    return hs, F0Table


def harmonicSum(TFmatrix, **kwargs):
    """The harmonic sum (signalTools.py:320-323)."""
    return f0detectionFunction(TFmatrix, detectFunc=np.sum, **kwargs)


def harmonicProd(TFmatrix, **kwargs):
    """The harmonic product (signalTools.py:325-328)."""
    return f0detectionFunction(TFmatrix, detectFunc=np.prod, **kwargs)


def sortSpectrum(spectrum, numberHarmonicsHS=50, numberHarmonicsHP=1, **kwargs):
    """Sort the columns of `spectrum` by their F0, estimated as the argmax of
    harmonic sum x harmonic product (signalTools.py:330-352).  The two
    saliences run on the GPU, the argmax / argsort over them on the host.
    Returns (sortedSpectrum, sorted f0s, hs, hp, F0 table).
    """
    hs, f0tablehs = harmonicSum(spectrum, numberHarmonics=numberHarmonicsHS, **kwargs)
    hp, f0tablehp = harmonicProd(spectrum, numberHarmonics=numberHarmonicsHP, **kwargs)
    f0s = f0tablehs[np.argmax(hs * hp, axis=0)]
    indsort = np.argsort(f0s)
    sortedSpectrum = spectrum[:, indsort]
    return sortedSpectrum, f0s[indsort], hs, hp, f0tablehs


def inv_herm_mat_2d(sigma_x_diag, sigma_x_off, verbose=False, device=None):
    """Batched explicit inverse of 2x2 Hermitian matrices (signalTools.py:132-196).

    Same contract as the reference: returns (inv_diag, inv_off, det) with the
    determinant floored to sign(det+eps)*max(|det|, eps).  Runs on the GPU.
    """
    d = np.ascontiguousarray(np.asarray(sigma_x_diag, dtype=np.float64))
    o = np.asarray(sigma_x_off)
    shape = o.shape
    n = int(np.prod(shape)) if len(shape) else 1
    d = np.ascontiguousarray(d.reshape(2, n))
    o = np.ascontiguousarray(o.astype(np.complex128).reshape(n))
    inv_d = np.empty((2, n))
    inv_o = np.empty(n, dtype=np.complex128)
    det = np.empty(n)
    dev = _lib.default_device() if device is None else device
    check(lib.fasst_inv_herm_mat_2d(dev, n, dptr(d), dptr(o), dptr(inv_d), dptr(inv_o),
                                    dptr(det)), "fasst_inv_herm_mat_2d")
    return inv_d.reshape((2,) + shape), inv_o.reshape(shape), det.reshape(shape)
