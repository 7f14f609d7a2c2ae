"""The transfer-heavy stateless calls give, bit for bit, what they gave before
their host copies went through DBuf's typed upload / put / get
(tests/golden/host_transfers.npz, written by make_golden_host_transfers.py
on the earlier library).  Kernels and inputs are unchanged, so the tolerance
is 0: any difference is a wrong count, a wrong buffer or a lost zero fill on
the host side."""
import os

import numpy as np
import pytest

import host_transfer_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pyfasst_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def got(lib):
    return cases.run_cases(lib)


@pytest.fixture(scope="module")
def want(golden_dir):
    with np.load(os.path.join(golden_dir, "host_transfers.npz")) as z:
        return {k: z[k] for k in z.files}


def _same(got, want, prefix):
    names = sorted(k for k in want if k.startswith(prefix))
    assert names and names == sorted(k for k in got if k.startswith(prefix))
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert not np.isnan(got[k]).any(), k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("call", ["istft_8_8_2_5", "istft_16_8_3_4", "istft_simm_8_8_2_5",
                                  "istft_simm_16_8_3_4"])
def test_istft_bit_exact(got, want, call):
    """fasst_istft / fasst_istft_simm, analysis window given and NULL."""
    _same(got, want, call + "_")


def test_istft_simm_refuses_less_than_two_windows(lib):
    """T = 1 gives len_out = wlen < 2 wlen: FASST_ERR_SHAPE with the edge-copy
    message from fasst_istft_simm, while fasst_istft accepts the same frame."""
    X = np.ones((5, 1), complex)
    w = np.ones(8)
    st, _ = cases.call_istft(lib, True, X, w, None, 8, 2)
    assert st == lib.FASST_ERR_SHAPE
    assert "8 samples < two windows (8); the reference's edge copy fails" in lib.last_error()
    st, y = cases.call_istft(lib, False, X, w, None, 8, 2)
    assert st == lib.FASST_OK and not np.isnan(y).any()


@pytest.mark.parametrize("L", cases.STFT_LENGTHS)
def test_stft_bit_exact(got, want, L):
    """L = 0 and 1: the signal buffer is larger than the copy and the kernel
    reads its zero fill; L = 9: a ragged last frame."""
    _same(got, want, "stft_L%d" % L)


@pytest.mark.parametrize("name", ["conv", "inst"])
def test_mix_solve_bit_exact(got, want, name):
    """All ranks 'conv' runs both kernels, all 'inst' only the first."""
    _same(got, want, "mix_solve_" + name)


def test_mix_solve_singular_leaves_mix_unwritten(lib):
    rss, rxs, mix = cases.mix_solve_inputs(3, 2, 9)
    rss[1] = 0.0
    st, out = cases.call_mix_solve(lib, rss, rxs, mix, [2, 2])
    assert st == lib.FASST_ERR_SINGULAR
    assert "Singular Matrix" in lib.last_error()
    assert np.array_equal(out, mix)


@pytest.mark.parametrize("shape", ["2_3_5", "2_1_257"])
def test_inv_sigma_mix_bit_exact(got, want, shape):
    _same(got, want, "inv_sigma_mix_%s_" % shape)


@pytest.mark.parametrize("n", [15, 257])
def test_wiener_gain_bit_exact(got, want, n):
    _same(got, want, "wiener_gain_%d" % n)
