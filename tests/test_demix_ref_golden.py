"""The NumPy restatement tests/demix_ref.py against the reference's own numbers
(tests/golden/demix_<case>.npz, written by make_golden_demix.py).  CPU only.

Masks, sizes, indices and the NaN pattern are equal; real values within 1e-12
relative.  The fixtures' decision margins (demix_ref's docstring) are asserted
to be at least 1e-9 and every argmax unique up to that gap, which is what makes
the exact mask comparison of tests/test_gpu_demix.py legitimate.
"""
import os

import numpy as np
import pytest

import demix_ref as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-12
_cache = {}


def case(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        d, out = D.run_case(D.read_scaled(g['wav']), int(g['fs']), **D.CASES[name])
        _cache[name] = (g, d, out)
    return _cache[name]


def close(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    if not np.array_equal(np.isinf(a), np.isinf(b)):
        return False
    ok = np.isfinite(b)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= RTOL * np.abs(b[ok])))


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_signal_is_the_fixtures(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert np.array_equal(D.case_signal(name), g['wav'])


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_features(name):
    g, d, out = case(name)
    for k in ('confidence', 'thetaVarAll'):
        for v in (0.0, D.eps, np.inf):
            assert np.array_equal(out[k] == v, g[k] == v), (k, v)
    for k in ('confidence', 'thetaAll', 'thetaVarAll'):
        assert close(out[k], g[k]), k
    # phi is an angle: compared on the circle, relative to pi
    dphi = np.angle(np.exp(1j * (out['phiAll'] - g['phiAll'])))
    assert np.array_equal(np.isnan(out['phiAll']), np.isnan(g['phiAll']))
    assert np.nanmax(np.abs(dphi)) <= RTOL * np.pi


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_rounds_and_masks(name):
    g, d, out = case(name)
    for k in ('index', 'zoom', 'size', 'remaining'):
        assert np.array_equal(out['round_' + k], g['round_' + k]), k
    assert np.array_equal(out['clusters'], g['clusters'])
    assert np.array_equal(np.isnan(out['round_delta']), np.isnan(g['round_delta']))
    assert np.array_equal(out['round_delta'], g['round_delta'], equal_nan=True)
    for k in ('theta', 'confidence'):
        assert close(out['round_' + k], g['round_' + k]), k
    assert np.max(np.abs(np.angle(np.exp(1j * (out['round_phi'] - g['round_phi']))))) <= RTOL * np.pi
    if name == 'demix_b':
        assert np.isnan(g['round_delta']).any() and (g['round_zoom'] > 1).any()


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_refinement_and_steering(name):
    g, d, out = case(name)
    for k in ('ref_index', 'ref_sizes'):
        assert np.array_equal(out[k], g[k]), k
    assert np.array_equal(out['ref_delta'], g['ref_delta'])
    for k in ('ref_theta', 'ref_confidence'):
        assert close(out[k], g[k]), k
    assert out['steering'].shape == g['steering'].shape
    assert np.max(np.abs(out['steering'] - g['steering'])) <= RTOL


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_decision_margins(name):
    """No comparison that decides a mask is closer than 1e-9 (relative), and
    an argmax is either unique up to that gap or an exact tie of the constants
    0 / eps, which both sides resolve to the lowest flat index."""
    g, d, out = case(name)
    print(name, d.margins, d.argmax_ties)
    for k, v in d.margins.items():
        assert v >= D.MARGIN_MIN, (k, v)
    for rnd, value, count in d.argmax_ties:
        assert value in (0.0, D.eps), (rnd, value, count)


def test_helpers():
    seq = np.array([0., 1., 3., 2.5, 1., 0., 0., 2.9])
    assert np.array_equal(np.flatnonzero(D.get_indices_peak(seq, 2, 0.8)), [2, 3])
    assert np.array_equal(np.flatnonzero(D.get_indices_peak(seq, 7, 0.5)), [7])
    assert D.invdb(D.decibel(3.0)) == pytest.approx(3.0, rel=1e-15)
    assert D.confidenceFromVar(0.01, 5) == pytest.approx(
        20 * np.log10((0.08 + 1 + np.sqrt(1.16)) / 0.08), rel=1e-15)
