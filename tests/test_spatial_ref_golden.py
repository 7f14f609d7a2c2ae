"""tests/spatial_filter_ref.py (the NumPy restatement the GPU tests compare
against at arbitrary shapes) reproduces what the reference itself computed in
separate_spatial_filter_comp and gcc_phat_tdoa_2d, recorded in
tests/golden/spatial_<case>*.npz.  CPU only."""
import json

import numpy as np
import pytest

import spatial_filter_ref as SR
from helpers import rel

TOL = 1e-13


def channel_transforms(g):
    """The channel transforms of the fixture's WAV by the oracle's front ends."""
    import fasst_ref as R
    kw = json.loads(str(g['ctor']))['kw']
    x, _ = R.read_scaled(g['wav'])
    wlen, hop = kw['wlen'], kw['hopsize']
    if kw.get('transf', 'stft') == 'stft':
        w = np.hanning(wlen)
        return [R.stft(x[:, c], w, hop, wlen) for c in range(2)], wlen
    import cqt_ref
    t = cqt_ref.RefCQT(kw['transf'], fmin=kw['tffmin'], fmax=18000, bins=kw['tfbpo'],
                       fs=int(g['fs']), linFTLen=wlen, atomHopFactor=hop / float(wlen))
    return [t.forward(x[:, c]) for c in range(2)], wlen


@pytest.fixture(scope="module", params=SR.CASES)
def case(request):
    g = SR.load_fixture(request.param)
    X, nfft = channel_transforms(g)
    return g, X, nfft


def test_fixture_is_well_conditioned(case):
    g = case[0]
    assert float(g['cond_max']) <= 1e3
    assert SR.cond_max(g['params']) == pytest.approx(float(g['cond_max']), rel=1e-9)


def test_gains(case):
    g = case[0]
    err = rel(SR.gains(g['params']), g['WG'])
    print("gains rel", err)
    assert err <= TOL


def test_images(case):
    g, X, _ = case
    err = rel(SR.images(g['WG'], X), g['images'])
    print("images rel", err)
    assert err <= TOL


def test_gcc_phat(case):
    g, X, nfft = case
    out = SR.gcc_phat(X[0] * np.conj(X[1]), nfft)
    assert out.shape == g['gcc'].shape
    # the MinQT has exactly-zero points, whose 0/0 makes their frames NaN in
    # the reference too; the STFT cases are finite
    bad = ~np.isfinite(g['gcc'])
    assert np.array_equal(~np.isfinite(out), bad)
    assert bad.any() if 'mqt' in str(g['ctor']) else not bad.any()
    err = rel(np.where(bad, 0.0, out), np.where(bad, 0.0, g['gcc']))
    print("gcc rel", err)
    assert err <= TOL
