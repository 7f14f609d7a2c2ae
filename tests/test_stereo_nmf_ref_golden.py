"""tests/stereo_nmf_ref.py reproduces the reference's stereo_NMF
(SIMM.py:945-1104) bit for bit on every case of tests/golden/stereo_nmf.npz
(written by tests/golden/make_golden_stereo_nmf.py from the reference itself),
and leaves NumPy's global stream where the reference leaves it.  CPU only.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_nmf_ref as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_nmf.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_fixture_holds_the_case_inputs(golden):
    for name in S.CASES:
        SXR, SXL, kw, seed = S.case_inputs(name)
        assert np.array_equal(golden[name + "_SXR"], SXR)
        assert np.array_equal(golden[name + "_SXL"], SXL)
        assert int(golden[name + "_seed"]) == seed
        for k in ("WM0", "HM0"):
            assert (k in kw) == (name + "_" + k in golden)
            if k in kw:
                assert np.array_equal(golden[name + "_" + k], kw[k])


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_restatement_is_the_reference_bit_for_bit(golden, name):
    SXR, SXL, kw, seed = S.case_inputs(name)
    np.random.seed(seed)
    res = S.stereo_NMF(SXR, SXL, **kw)
    after = np.random.rand()
    for n, v in zip(S.NAMES, res):
        assert v.shape == golden["%s_%s" % (name, n)].shape
        assert np.array_equal(v, golden["%s_%s" % (name, n)]), (name, n)
    assert after == float(golden[name + "_rand"])
    reco = res[4]
    assert reco.shape == (3 * kw["numberOfIterations"] + 1,) and np.all(np.isfinite(reco))


def test_betas_are_diagonal_and_sum_to_one(golden):
    for name in S.CASES:
        bR, bL = golden[name + "_betaR"], golden[name + "_betaL"]
        R = S.CASES[name][3]
        assert bR.shape == bL.shape == (R, R)
        assert np.array_equal(bR, np.diag(np.diag(bR)))
        assert np.allclose(np.diag(bR) + np.diag(bL), 1.0, rtol=0, atol=1e-15)
