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


# ---- set / get round trips (tolerance 0) ------------------------------------
# Each setter stores its input unchanged in source j's rows of a padded image;
# both sources are set with different data before either is read back, so a
# wrong offset or pitch shows as a neighbour's rows overwritten.

def test_spectral_round_trip():
    """fasst_set_spectral / fasst_get_spectral: FB [Fp][KP], FW [KP][KP] and
    TW [KP][Tp] rows of two sources, F, T and K below their padded sizes."""
    e = cases.rt_engine()
    F, T, K = cases.RT_F, cases.RT_T, cases.RT_K
    sent = [(cases.rt_rand(10 * j, F, K), cases.rt_rand(10 * j + 1, K, K),
             cases.rt_rand(10 * j + 2, K, T)) for j in range(2)]
    for j in range(2):
        e.set_spectral(j, *sent[j], fb_free=True, tw_free=True)
    for j in range(2):
        for a, b in zip(sent[j], e.get_spectral(j, K)):
            assert np.array_equal(a, b), j
    e.close()


def test_spatial_round_trip():
    """fasst_set_spatial / fasst_get_spatial: a convolutive source of rank 2
    (rows of A at pitch Fp) and an instantaneous one of rank 2 (Pinst at rank
    offset 2)."""
    e = cases.rt_engine(conv=(True, False))
    rng = np.random.default_rng(3)
    conv = rng.standard_normal((2, 2, cases.RT_F)) + 1j * rng.standard_normal((2, 2, cases.RT_F))
    inst = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    e.set_spatial(0, conv, True)
    e.set_spatial(1, inst, True)
    assert np.array_equal(e.get_spatial(0, conv.shape), conv)
    assert np.array_equal(e.get_spatial(1, inst.shape), inst)
    e.close()


def test_tb_round_trip():
    """fasst_set_tb / fasst_get_tb with L = 4 < kMaxTB on both sources: the
    factor TW at its offset in the slot buffer, TB rows at pitch Tp."""
    e = cases.rt_engine()
    F, T, K, L = cases.RT_F, cases.RT_T, cases.RT_K, 4
    for j in range(2):
        e.set_spectral(j, cases.rt_rand(j, F, K), np.eye(K), cases.rt_rand(j + 5, K, T), True, True)
    sent = [(cases.rt_rand(20 + j, K, L), cases.rt_rand(30 + j, L, T)) for j in range(2)]
    for j in range(2):
        e.set_tb(j, 0, *sent[j])
    for j in range(2):
        TW, TB = e.get_tb(j, 0, K, L)
        assert np.array_equal(TW, sent[j][0]) and np.array_equal(TB, sent[j][1]), j
    e.close()


def test_tw_constr_round_trip():
    """fasst_set_tw_constr / fasst_get_tw_constr: TW_all rows at pitch Tp,
    the SHMM transitions [K][K] at pitch KP (source 0) and the GSMM priors
    [K] (source 1), and the decoded states read back as the zero they were
    set to."""
    e = cases.rt_engine()
    F, T, K = cases.RT_F, cases.RT_T, cases.RT_K
    for j in range(2):
        e.set_spectral(j, cases.rt_rand(j, F, K), np.eye(K), cases.rt_rand(j + 5, K, T), True, True)
    kinds = ("SHMM", "GSMM")
    sent = [(cases.rt_rand(40, K, T), cases.rt_rand(41, K, K)),
            (cases.rt_rand(42, K, T), cases.rt_rand(43, K))]
    for j in range(2):
        e.set_tw_constr(j, kinds[j], *sent[j])
    for j in range(2):
        a, d, s = e.get_tw_constr(j, kinds[j])
        assert np.array_equal(a, sent[j][0]) and np.array_equal(d, sent[j][1]), j
        assert not s.any(), j
    e.close()


def test_sfnmf_round_trip(lib):
    """sfnmf_set_params / sfnmf_get_params: odd N and K, below their even
    padded pitches pN and pK."""
    sent, back = cases.sfnmf_round_trip(lib, cases.RT_F, cases.RT_T, (cases.RT_K, 1, 5), 50)
    for a, b in zip(sent, back):
        assert np.array_equal(a, b)


def test_sf_round_trip():
    """fasst_set_factors / fasst_get_factors and fasst_sf_set_spatial /
    fasst_sf_get_spatial: source 1's factor shares source 0's FB (an alias
    pointer), so setting it replaces what source 0 reads; mix rows of source 1
    start behind source 0's."""
    from pyfasst_amd.engine import Engine
    F, T, K = cases.RT_F, cases.RT_T, cases.RT_K
    e = Engine(F, T)
    e.sf_configure([2, 2], [True, False], [[(K, 2, 1, 1, 1)], [(K, 4, 1, 1, 1)]],
                   [[(-1, -1, -1)], [(0, -1, -1)]])
    f0 = (cases.rt_rand(60, F, K), cases.rt_rand(61, K, 2), cases.rt_rand(62, 2, T))
    f1 = (cases.rt_rand(63, F, K), cases.rt_rand(64, K, 4), cases.rt_rand(65, 4, T))
    e.set_factors(0, 0, *f0)
    e.set_factors(1, 0, *f1)
    g0, g1 = e.get_factors(0, 0), e.get_factors(1, 0)
    assert np.array_equal(g0[0], f1[0]) and np.array_equal(g1[0], f1[0])   # the shared FB
    for q in (1, 2):
        assert np.array_equal(g0[q], f0[q]) and np.array_equal(g1[q], f1[q]), q
    rng = np.random.default_rng(66)
    conv = rng.standard_normal((2, 2, F)) + 1j * rng.standard_normal((2, 2, F))
    inst = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    e.sf_set_spatial(0, conv, True)
    e.sf_set_spatial(1, inst, True)
    assert np.array_equal(e.sf_get_spatial(0, conv.shape), conv)
    assert np.array_equal(e.sf_get_spatial(1, inst.shape), inst)
    e.close()


def test_demix_plane_and_mask_round_trip(lib):
    """demix_set_plane / demix_get_plane for planes 1 and 3, demix_set_mask /
    demix_get_mask for cluster masks 0 and 2: each at its offset which * n."""
    import ctypes
    F, N, nb = cases.RT_F, cases.RT_T, 3
    n = F * (N - nb + 1)
    h = ctypes.c_void_p()
    assert lib.lib.demix_create(0, F, N, nb, 3, ctypes.byref(h)) == lib.FASST_OK, lib.last_error()
    try:
        planes = {w: cases.rt_rand(70 + w, n) for w in (1, 3)}
        masks = {s: (np.random.default_rng(80 + s).random(n) < 0.5).astype(np.uint8) for s in (0, 2)}
        for w, a in planes.items():
            assert lib.lib.demix_set_plane(h, w, lib.dptr(a)) == lib.FASST_OK, lib.last_error()
        for s, a in masks.items():
            st = lib.lib.demix_set_mask(h, s, a.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
            assert st == lib.FASST_OK, lib.last_error()
        for w, a in planes.items():
            out = np.full(n, np.nan)
            assert lib.lib.demix_get_plane(h, w, lib.dptr(out)) == lib.FASST_OK, lib.last_error()
            assert np.array_equal(out, a), w
        for s, a in masks.items():
            out = np.full(n, 255, np.uint8)
            st = lib.lib.demix_get_mask(h, s, out.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
            assert st == lib.FASST_OK, lib.last_error()
            assert np.array_equal(out, a), s
    finally:
        lib.lib.demix_destroy(h)


# ---- bit-exact against the library before the copies moved onto DSpan --------
@pytest.fixture(scope="module")
def got_compute(lib):
    return cases.run_compute_cases(lib)


@pytest.fixture(scope="module")
def want_compute(golden_dir):
    with np.load(os.path.join(golden_dir, "host_transfers_compute.npz")) as z:
        return {k: z[k] for k in z.files}


def test_viterbi_bit_exact(got_compute, want_compute):
    """S = 3, N = 5 with host leading dimensions 8 and 4."""
    _same(got_compute, want_compute, "viterbi_3_5")


@pytest.mark.parametrize("n", [7, 101])
def test_nsgt_fft_bit_exact(got_compute, want_compute, n):
    _same(got_compute, want_compute, "nsgt_fft_%d_" % n)


@pytest.mark.parametrize("prefix", ["cqt_cell_", "cqt_cells_raster", "cqt_cells_inverse",
                                    "cqt_raster_forward", "cqt_raster_inverse"])
def test_cqt_bit_exact(got_compute, want_compute, prefix):
    """cqt24 on 101 samples through the cells (forward, raster, inverse) and
    cqt12 through the raster path; outputs above 2 KB as SHA-256 digests."""
    _same(got_compute, want_compute, prefix)


def test_filter_stft_bit_exact(got_compute, want_compute):
    _same(got_compute, want_compute, "filter_stft")


@pytest.mark.parametrize("prefix", ["nmf_K3_", "nmf_K16_", "snmf_", "simm_stereo_", "simm_mono_"])
def test_nmf_contexts_bit_exact(got_compute, want_compute, prefix):
    """One iteration of the nmf (plain and fused), snmf and simm (stereo and
    mono) contexts, then their getters."""
    _same(got_compute, want_compute, prefix)


@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_nsgt_plan_bit_exact(got_compute, want_compute, kind):
    """fasst_nsgt_forward / fasst_nsgt_backward on host arrays of 101 samples."""
    _same(got_compute, want_compute, "nsgt_%s_" % kind)


def test_gemm_harness_skew_bit_exact(got_compute, want_compute):
    _same(got_compute, want_compute, "gemm_skew_")
