"""Every separation call gives, bit for bit, what it gave before the calls
shared one image producer per model and one iSTFT sink
(tests/golden/separation_tail.npz, written by make_golden_separation_tail.py on
the earlier library), and refuses what it refused with the same status.
Kernels, launches and inputs are unchanged, so the tolerance is 0: any
difference is a wrong buffer, stride, count or a lost zero fill on the host
side.  Shapes and cases: tests/separation_tail_cases.py."""
import os

import numpy as np
import pytest

import separation_tail_cases as cases

pytestmark = pytest.mark.gpu

GEOMETRIES = ["8_8_2_5", "16_8_3_4"]
STFT_CALLS = ["separate", "spatial", "sf", "nmf"]


@pytest.fixture(scope="module")
def lib():
    from pyfasst_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def got(lib):
    return cases.run_cases(lib)


@pytest.fixture(scope="module")
def want(golden_dir):
    with np.load(os.path.join(golden_dir, "separation_tail.npz")) as z:
        return {k: z[k] for k in z.files}


def _same(got, want, prefix, count):
    names = sorted(k for k in want if k.startswith(prefix))
    assert len(names) == count and names == sorted(k for k in got if k.startswith(prefix))
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert not np.isnan(got[k]).any(), k
        assert np.array_equal(got[k], want[k]), k


def test_no_case_left_out(got, want):
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("g", GEOMETRIES)
def test_main_model_bit_exact(got, want, g):
    """wiener_images and separate_waveforms (analysis window given and NULL),
    one source per component and one source of both (NS = 1 != J)."""
    _same(got, want, "main_images_" + g, 1)
    _same(got, want, "main_waveforms_" + g, 2)
    _same(got, want, "main_images_one_source_" + g, 1)
    _same(got, want, "main_waveforms_one_source_" + g, 2)


@pytest.mark.parametrize("g", GEOMETRIES)
def test_spatial_filter_bit_exact(got, want, g):
    _same(got, want, "spatial_gains_" + g, 1)
    _same(got, want, "spatial_images_" + g, 1)
    _same(got, want, "spatial_waveforms_" + g, 2)


@pytest.mark.parametrize("g", GEOMETRIES)
def test_two_factor_bit_exact(got, want, g):
    """src_of = (0, 0, -1) and (1, 0, 1)."""
    _same(got, want, "sf_images_" + g, 2)
    _same(got, want, "sf_waveforms_" + g, 4)


@pytest.mark.parametrize("g", GEOMETRIES)
def test_nmf_bit_exact(got, want, g):
    _same(got, want, "nmf_images_" + g, 1)
    _same(got, want, "nmf_waveforms_" + g, 2)


@pytest.mark.parametrize("call", ["cqt_separate", "cqt_spatial", "cqt_sf_separate"])
def test_cqt_sink_bit_exact(got, want, call):
    _same(got, want, call, 1)


@pytest.mark.parametrize("call", STFT_CALLS)
def test_refusals_as_before(lib, got, want, call):
    """The recorded statuses are FASST_ERR_SHAPE throughout (checked here so a
    fixture from a broken library cannot pass); the cases assert that a
    refused call leaves its NaN-filled output alone."""
    kinds = ["nfft_12", "wlen_above_nfft", "hop_0", "other_bin_count"]
    if call != "nmf":
        kinds.append("no_stft")
    for kind in kinds:
        k = "refuse_%s_%s" % (call, kind)
        assert want[k].tolist() == [lib.FASST_ERR_SHAPE], k
        assert np.array_equal(got[k], want[k]), k
    n = sum(k.startswith("refuse_%s_" % call) for k in want)
    assert n == len(kinds)


@pytest.mark.parametrize("call", STFT_CALLS)
def test_valid_call_after_refusals(got, want, call):
    """The context that refused answers the next valid call as the fixture,
    which is also what a fresh context gave."""
    _same(got, want, "after_refusals_" + call, 1)
    fresh = {"separate": "main_waveforms_8_8_2_5_aw", "spatial": "spatial_waveforms_8_8_2_5_aw",
             "sf": "sf_waveforms_8_8_2_5_src1_aw", "nmf": "nmf_waveforms_8_8_2_5_aw"}[call]
    assert np.array_equal(got["after_refusals_" + call], got[fresh])
    if call != "nmf":
        _same(got, want, "after_no_stft_" + call, 1)
        assert np.array_equal(got["after_no_stft_" + call], got[fresh])
