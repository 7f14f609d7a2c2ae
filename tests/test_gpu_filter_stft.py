"""filter_stft / filter_conv_stft on the GPU (k_filter_frames) against the
reference's outputs (tests/golden/filter_stft.npz) and, for the shapes without
a fixture, the live restatement (tests/filter_stft_ref.py).

Metric: max-norm error over the whole output relative to max |reference|.
Bound: TOL, the one tests/test_gpu_parity.py applies to istft against
stft.npz (test_stft_istft_golden_gpu).
"""
import numpy as np
import pytest

import filter_stft_ref as FR
from pyfasst_amd.tftransforms.stft import filter_conv_stft, filter_stft

pytestmark = pytest.mark.gpu

TOL = 1e-13


@pytest.fixture(scope="module")
def g():
    return np.load(FR.GOLDEN)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def run_gpu(name, **kw):
    c = FR.CASES[name]
    data, W, aw, sw = FR.draw(name)
    fn = filter_stft if c['fn'] == 'stft' else filter_conv_stft
    return fn(data, W, analysisWindow=aw, synthWindow=sw, hopsize=float(c['hop']),
              nfft=float(c['nfft']), **kw)


@pytest.mark.parametrize("name", sorted(FR.CASES))
def test_vs_reference(g, name):
    y, r = run_gpu(name), g['y_' + name]
    assert isinstance(y, np.ndarray) and y.dtype == np.float64 and y.shape == r.shape
    err = rel(y, r)
    print(name, "gpu vs fixture: %.3g" % err)
    assert err < TOL


# shapes without a fixture: (fn, L, wlen, nfft, hop, M, time-varying, complex W)
LIVE = [
    ('stft', 333, 64, 64, 16, 9, True, True),      # M_in > 8: the out-of-place form
    ('stft', 333, 64, 128, 24, 10, False, False),
    ('stft', 700, 256, 512, 64, 8, True, True),    # the widest in-register form, 3 blocks of bins
    ('stft', 257, 32, 32, 16, 2, True, False),     # hop = wlen / 2, the largest a sine bell allows
    ('conv', 333, 64, 64, 16, 5, True, True),
    ('conv', 64, 64, 64, 16, 12, False, True),
]


@pytest.mark.parametrize("case", LIVE, ids=lambda c: "%s_M%d_nfft%d_%s" % (c[0], c[5], c[3],
                                                                         "tv" if c[6] else "ti"))
def test_vs_live_restatement(case):
    fn, L, wlen, nfft, hop, M, tv, cplx = case
    rs = np.random.RandomState(L + M)
    F, N = nfft // 2 + 1, -(-L // hop)
    shape = ((M, M, F) if fn == 'stft' else (M, F)) + ((N,) if tv else ())
    W = rs.randn(*shape) + (1j * rs.randn(*shape) if cplx else 0)
    data = rs.randn(L, M) if fn == 'stft' else rs.randn(L)
    kw = dict(analysisWindow=np.hanning(wlen) + 0.1, synthWindow=FR.sinebell(wlen),
              hopsize=float(hop), nfft=float(nfft))
    got = (filter_stft if fn == 'stft' else filter_conv_stft)(data, W, **kw)
    ref = (FR.filter_stft if fn == 'stft' else FR.filter_conv_stft)(data, W, **kw)
    assert got.shape == ref.shape
    err = rel(got, ref)
    print(case, "gpu vs restatement: %.3g" % err)
    assert err < TOL


def test_identity_filter_returns_the_input():
    """W = I with analysisWindow = synthWindow = sine bell: the window-product
    normalisation makes the chain the identity on [0, L)."""
    rs = np.random.RandomState(11)
    for L, wlen, nfft, hop, M in ((1000, 64, 128, 16, 3), (1000, 64, 64, 24, 2), (50, 64, 64, 16, 1)):
        x = rs.randn(L, M)
        W = np.zeros((M, M, nfft // 2 + 1))
        W[np.arange(M), np.arange(M)] = 1.0
        sw = FR.sinebell(wlen)
        y = filter_stft(x, W, analysisWindow=sw, synthWindow=sw, hopsize=float(hop), nfft=float(nfft))
        assert y.shape[0] >= L
        err = rel(y[:L], x)
        print((L, wlen, nfft, hop, M), "identity: %.3g" % err)
        assert err < TOL
    x = rs.randn(500)
    sw = FR.sinebell(64)
    y = filter_conv_stft(x, np.ones((2, 33)), analysisWindow=sw, synthWindow=sw, hopsize=16.0,
                         nfft=64.0)
    assert rel(y[:500, 0], x) < TOL and rel(y[:500, 1], x) < TOL


def test_two_runs_are_bit_equal():
    for name in ("m5_surplus", "conv_m2_tv"):
        np.testing.assert_array_equal(run_gpu(name), run_gpu(name))


def _lib_layout(name):
    return {"numpy": 0, "frames": 1}[name]       # FILTER_W_NUMPY / FILTER_W_FRAMES


class _Hip(object):
    """hipMalloc / hipMemcpy of the HIP runtime the library already loaded
    (as tests/test_gpu_sigtools.py does), for device pointers."""

    def __init__(self):
        import ctypes
        path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
        self.ct, self.rt, self.bufs = ctypes, ctypes.CDLL(path), []
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]

    def up(self, a):
        ct = self.ct
        a = np.ascontiguousarray(a)
        p = ct.c_void_p()
        assert self.rt.hipMalloc(ct.byref(p), a.nbytes) == 0
        self.bufs.append(p)
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return ct.cast(p, ct.POINTER(ct.c_double))

    def down(self, p, shape):
        ct = self.ct
        a = np.empty(shape)
        assert self.rt.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0
        return a

    def free(self):
        for p in self.bufs:
            self.rt.hipFree(p)


@pytest.mark.parametrize("name", ["base_m2", "m5_surplus", "short_m3", "m4_tv_real", "conv_m3_col",
                                  "conv_m1", "lds_4096"])
def test_device_pointer_entry_and_frame_major_layout(name):
    """fasst_filter_stft_dev on arrays already in device memory gives the host
    entry's bits, with W in NumPy order and, for a time-varying W, again with
    W handed over frame-major ([.., N, F]: no transpose runs)."""
    import ctypes
    from pyfasst_amd import _lib
    c = FR.CASES[name]
    data, W, aw, sw = FR.draw(name)
    host = run_gpu(name)
    aw = sw if aw is None or len(aw) != len(sw) else aw
    W = np.asarray(W, dtype=np.complex128)
    m_in = c['M'] if c['fn'] == 'stft' else 1
    tv = W.ndim == (4 if c['fn'] == 'stft' else 3)
    hip = _Hip()
    _lib.lib.fasst_filter_set_timing(1)
    try:
        dx, daw, dsw = hip.up(data), hip.up(aw), hip.up(sw)
        dy = hip.up(np.zeros(host.shape))
        layouts = [(W, _lib_layout("numpy"))]
        if tv:
            layouts.append((np.moveaxis(W, -1, -2), _lib_layout("frames")))
        for Wl, flag in layouts:
            n = ctypes.c_int(0)
            st = _lib.lib.fasst_filter_stft_dev(
                0, dx, c['L'], m_in, c['M'], hip.up(Wl), int(tv), W.shape[-1] if tv else 0, daw,
                dsw, c['wlen'], c['nfft'], c['hop'], dy, ctypes.byref(n), flag, None)
            assert st == _lib.FASST_OK, _lib.last_error()
            assert n.value == host.shape[0]
            np.testing.assert_array_equal(hip.down(dy, host.shape), host)
            tot, tr = ctypes.c_double(-1), ctypes.c_double(-1)
            assert _lib.lib.fasst_filter_last_ms(ctypes.byref(tot), ctypes.byref(tr)) == 0
            if not (tv and flag == 0):
                assert tr.value == 0.0          # no transpose ran
        st = _lib.lib.fasst_filter_stft_dev(0, dx, c['L'], m_in, c['M'], hip.up(W), int(tv),
                                            W.shape[-1] if tv else 0, daw, dsw, c['wlen'],
                                            c['nfft'], c['hop'], dy, None, 7, None)
        assert st == _lib.FASST_ERR_SHAPE and "layout" in _lib.last_error()
    finally:
        _lib.lib.fasst_filter_set_timing(0)
        hip.free()


TORCH_CASES = ["base_m2", "m5_surplus", "short_m3", "m4_tv_real", "conv_m3_col", "conv_m1",
               "lds_4096"]


@pytest.fixture(scope="module")
def torch_child():
    """tests/filter_stft_torch_child.py, once: the tensor route needs a process
    in which torch initialised the GPU before the library did, which this one
    (the library has run already) is not."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "filter_stft_torch_child.py")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("name", TORCH_CASES)
def test_torch_tensors_in_tensor_out_bit_equal(torch_child, name):
    """Tensors in and a tensor out, on the device, equal to the NumPy route
    bit for bit; and with the frame-major W layout flag, equal again."""
    r = torch_child["cases"][name]
    c = FR.CASES[name]
    assert r["tensor_out"] and r["bit_equal"] and r["mixed_bit_equal"]
    if c['wdim'] == (4 if c['fn'] == 'stft' else 3):
        assert r["frame_major_bit_equal"]
    else:
        assert r["frame_major_refused"]
    assert r["scaled"] < TOL


def test_torch_tensors_raise_the_reference_exceptions(torch_child):
    assert torch_child["errors"] == {k: "ok" for k in ("channels", "bins", "ndim", "frames", "single",
                                                       "conv_ndim", "cpu_tensor")}


def test_past_the_lds_ceiling_is_refused_before_any_launch():
    # 2 buffers of 8192 complex doubles = 256 KB > 160 KB
    with pytest.raises(NotImplementedError, match=r"M=3.*nfft=8192"):
        filter_stft(np.zeros((9000, 3)), np.zeros((3, 3, 4097)), synthWindow=FR.sinebell(8192),
                    hopsize=2048.0, nfft=8192.0)
    with pytest.raises(NotImplementedError, match=r"nfft=8192"):
        filter_conv_stft(np.zeros(9000), np.zeros((3, 4097)), synthWindow=FR.sinebell(8192),
                         hopsize=2048.0, nfft=8192.0)


def test_the_reference_exceptions():
    rs = np.random.RandomState(0)
    sw = FR.sinebell(64)
    kw = dict(synthWindow=sw, hopsize=16.0, nfft=64.0)
    x = rs.randn(200, 2)
    with pytest.raises(AttributeError, match="W does not have the right number of channels"):
        filter_stft(x, rs.randn(3, 3, 33), **kw)
    with pytest.raises(AttributeError, match="W not the right size"):
        filter_stft(x, rs.randn(2, 2, 65), **kw)
    with pytest.raises(NotImplementedError):
        filter_stft(x, rs.randn(2, 2, 33, 13, 1), **kw)
    with pytest.raises(IndexError):
        filter_stft(x, rs.randn(2, 2, 33, 12), **kw)
    with pytest.raises(NotImplementedError, match="non-integer hopsize"):
        filter_stft(x, rs.randn(2, 2, 33), synthWindow=sw, hopsize=16.5, nfft=64.0)
    with pytest.raises(ValueError):
        filter_stft(rs.randn(100, 2), rs.randn(2, 2, 33), synthWindow=sw, hopsize=60.0, nfft=64.0)
    with pytest.raises(ValueError):
        filter_conv_stft(rs.randn(100), rs.randn(2, 33), synthWindow=sw, hopsize=60.0, nfft=64.0)
    with pytest.raises(NotImplementedError, match="96"):
        filter_stft(x, rs.randn(2, 2, 49), synthWindow=sw, hopsize=16.0, nfft=96.0)
    with pytest.raises(AttributeError, match="provided data should be single channel"):
        filter_conv_stft(x, rs.randn(2, 33), **kw)
    with pytest.raises(AttributeError, match="W not the right size"):
        filter_conv_stft(x[:, 0], rs.randn(2, 65), **kw)
    with pytest.raises(ValueError, match="right shape"):
        filter_conv_stft(x[:, 0], rs.randn(2, 33, 13, 1), **kw)
    with pytest.raises(IndexError):
        filter_conv_stft(x[:, :1], rs.randn(2, 33, 12), **kw)
    # the calls above left the device usable
    assert rel(filter_stft(x, np.tile(np.eye(2)[:, :, None], (1, 1, 33)), analysisWindow=sw, **kw)[:200],
               x) < TOL


def test_reference_import_name_and_defaults():
    import inspect
    import pyfasst.tftransforms.stft as s
    assert s.filter_stft is filter_stft and s.filter_conv_stft is filter_conv_stft
    p = inspect.signature(filter_stft).parameters
    assert list(p)[:7] == ['data', 'W', 'analysisWindow', 'synthWindow', 'hopsize', 'nfft', 'fs']
    assert (p['analysisWindow'].default is None and p['hopsize'].default == 256.0 and
            p['nfft'].default == 2048.0 and p['fs'].default == 44100.0 and
            p['synthWindow'].default.shape == (2048,) and p['device'].default is None)
    q = inspect.signature(filter_conv_stft).parameters
    assert list(q)[:9] == list(p)[:7] + ['verbose', 'device'] and q['verbose'].default == 0
    # the defaults run: 2048-point sine bell, hop 256
    rs = np.random.RandomState(3)
    x = rs.randn(3000, 2)
    W = rs.randn(2, 2, 1025)
    assert rel(filter_stft(x, W), FR.filter_stft(x, W)) < TOL
