"""The NumPy restatement tests/filter_stft_ref.py against the reference's own
outputs (tests/golden/filter_stft.npz, written by make_golden_filter.py), and
the host-side half of the fasst_filter_stft ABI.  CPU only.

Restatement against fixture, max |difference| / max |fixture| per case:
measured worst case 0.0 over the 15 cases (every case is bit-equal: the
restatement makes the reference's NumPy calls in the reference's order).  The
assertion is ten times that worst case, i.e. equality.  Nothing on the GPU
depends on this figure.
"""
import ctypes
import json

import numpy as np
import pytest

import filter_stft_ref as FR
from pyfasst_amd import _lib
from pyfasst_amd.tftransforms.stft import filter_conv_stft, filter_stft  # noqa: F401

WORST_MEASURED = 0.0


@pytest.fixture(scope="module")
def g():
    return np.load(FR.GOLDEN)


def test_fixture_holds_every_case_and_only_parameters_and_outputs(g):
    assert sorted(g.files) == sorted(['y_' + n for n in FR.CASES] + ['case_' + n for n in FR.CASES])
    for n in FR.CASES:
        assert json.loads(str(g['case_' + n])) == dict(FR.CASES[n], seed=FR.seed_of(n))


@pytest.mark.parametrize("name", sorted(FR.CASES))
def test_restatement_vs_reference(g, name):
    y, r = FR.run_ref(name), g['y_' + name]
    c = FR.CASES[name]
    nframes = -(-c['L'] // c['hop'])
    assert y.shape == r.shape == ((nframes - 1) * c['hop'] + c['wlen'] - c['wlen'] // 2, c['M'])
    err = np.max(np.abs(y - r)) / np.max(np.abs(r))
    print(name, "restatement vs fixture: %.3g" % err)
    assert err <= 10 * WORST_MEASURED


def _call(L, m_in, m_out, tv, nwf, wlen, nfft, hop):
    """fasst_filter_stft with y_out == NULL: validation and *len_out only."""
    one = np.zeros(1)
    n = ctypes.c_int(-1)
    st = _lib.lib.fasst_filter_stft(0, _lib.dptr(one), L, m_in, m_out, _lib.dptr(one), tv, nwf,
                                    _lib.dptr(one), _lib.dptr(one), wlen, nfft, hop, None,
                                    ctypes.byref(n))
    return st, n.value, _lib.last_error()


def test_abi_length_query_touches_no_device():
    assert _call(1000, 2, 2, 0, 0, 64, 64, 16)[:2] == (_lib.FASST_OK, 1024)
    assert _call(50, 3, 3, 1, 4, 64, 128, 16)[:2] == (_lib.FASST_OK, 80)
    assert _call(6000, 2, 2, 1, 6, 4096, 4096, 1024)[:2] == (_lib.FASST_OK, 7168)
    # M_in > 8: input and output buffers side by side
    assert _call(1000, 10, 10, 0, 0, 64, 64, 16)[0] == _lib.FASST_OK
    assert _call(5000, 2, 2, 0, 0, 8192, 8192, 2048)[0] == _lib.FASST_OK
    assert _call(5000, 8, 8, 0, 0, 2048, 2048, 512)[0] == _lib.FASST_OK


def test_abi_refuses_on_the_host():
    st, _, msg = _call(5000, 3, 3, 0, 0, 8192, 8192, 2048)        # 2 x 8192 x 16 B = 256 KB
    assert st == _lib.FASST_ERR_UNSUPPORTED and "M=3" in msg and "nfft=8192" in msg
    st, _, msg = _call(5000, 9, 9, 0, 0, 1024, 1024, 256)         # out of place: 10 x 1024 x 16 B
    assert st == _lib.FASST_OK
    st, _, msg = _call(5000, 9, 9, 0, 0, 2048, 2048, 512)
    assert st == _lib.FASST_ERR_UNSUPPORTED and "M=9" in msg and "nfft=2048" in msg
    st, _, msg = _call(1000, 2, 2, 0, 0, 64, 96, 16)
    assert st == _lib.FASST_ERR_UNSUPPORTED and "96" in msg
    assert _call(1000, 2, 2, 0, 0, 64, 32, 16)[0] == _lib.FASST_ERR_SHAPE      # nfft < wlen
    assert _call(1000, 2, 2, 0, 0, 64, 16384, 16)[0] == _lib.FASST_ERR_SHAPE   # nfft > 8192
    assert _call(1000, 2, 2, 1, 62, 64, 64, 16)[0] == _lib.FASST_ERR_SHAPE     # 63 frames needed
    assert _call(1000, 2, 2, 1, 63, 64, 64, 16)[0] == _lib.FASST_OK
    assert _call(100, 2, 2, 0, 0, 64, 64, 60)[0] == _lib.FASST_ERR_SHAPE       # 32 + 100 > 124
    # grid extents: M_out on y, M_in * M_out on z (LDS alone would admit them at nfft 32)
    assert _call(1000, 320, 320, 0, 0, 32, 32, 8)[0] == _lib.FASST_ERR_SHAPE
    assert _call(1000, 1, 65536, 0, 0, 4, 4, 2)[0] == _lib.FASST_ERR_SHAPE
    assert _call(1000, 255, 257, 0, 0, 32, 32, 8)[0] == _lib.FASST_OK
    assert _call(0, 2, 2, 0, 0, 64, 64, 16)[0] == _lib.FASST_ERR_SHAPE
    assert _call(1000, 0, 2, 0, 0, 64, 64, 16)[0] == _lib.FASST_ERR_SHAPE


def test_python_errors_come_before_any_device_call():
    """The reference's exceptions, raised on the host (no GPU here)."""
    rs = np.random.RandomState(0)
    sw = FR.sinebell(64)
    kw = dict(synthWindow=sw, hopsize=16.0, nfft=64.0)
    x = rs.randn(200, 2)
    with pytest.raises(AttributeError, match="right number of channels"):
        filter_stft(x, rs.randn(3, 3, 33), **kw)
    with pytest.raises(AttributeError, match="W not the right size"):
        filter_stft(x, rs.randn(2, 2, 65), **kw)
    with pytest.raises(NotImplementedError):
        filter_stft(x, rs.randn(2, 2, 33, 13, 1), **kw)
    with pytest.raises(IndexError):
        filter_stft(x, rs.randn(2, 2, 33, 12), **kw)                # 13 frames needed
    with pytest.raises(NotImplementedError, match="hopsize"):
        filter_stft(x, rs.randn(2, 2, 33), synthWindow=sw, hopsize=16.5, nfft=64.0)
    with pytest.raises(ValueError):
        filter_stft(rs.randn(100, 2), rs.randn(2, 2, 33), synthWindow=sw, hopsize=60.0, nfft=64.0)
    with pytest.raises(NotImplementedError, match="96"):
        filter_stft(x, rs.randn(2, 2, 49), synthWindow=sw, hopsize=16.0, nfft=96.0)
    with pytest.raises(AttributeError, match="single channel"):
        filter_conv_stft(x, rs.randn(2, 33), **kw)
    with pytest.raises(AttributeError, match="W not the right size"):
        filter_conv_stft(x[:, 0], rs.randn(2, 65), **kw)
    with pytest.raises(ValueError, match="right shape"):
        filter_conv_stft(x[:, 0], rs.randn(2, 33, 13, 1), **kw)
    with pytest.raises(IndexError):
        filter_conv_stft(x[:, :1], rs.randn(2, 33, 12), **kw)
    with pytest.raises(NotImplementedError, match="M=3"):
        filter_stft(rs.randn(5000, 3), np.zeros((3, 3, 4097)), synthWindow=FR.sinebell(8192),
                    hopsize=2048.0, nfft=8192.0)


def test_registry_has_the_base_class():
    from pyfasst_amd.tftransforms import tft
    assert tft.tftransforms['stftold'] is tft.TFTransform
    t = tft.TFTransform(fmin=30, linFTLen=512, anything=1)
    assert t.transformname == 'dummy' and t.transfo is None
    assert t.computeTransform(np.zeros(4)) is None and t.invertTransform() is None
