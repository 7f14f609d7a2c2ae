"""The NumPy restatement tests/slicq_ref.py against the reference's fixtures
tests/golden/slicq_*.npz.  CPU only: no device call is made.

The planner is held to the reference's bits; coefficients and reconstruction to
slicq_ref.TIGHT (1e-9, the project's FP64 bound) relative to the largest
magnitude: both sides are numpy.fft on the same inputs.
"""
import numpy as np
import pytest

import slicq_ref as SR
from helpers import load, rel


def check_planner(p, g):
    """Windows, positions, lengths and duals equal the fixture's bits."""
    assert np.array_equal(p.M, g["M"])
    assert np.array_equal(p.rfbas, g["rfbas"])
    assert int(p.nn) == int(g["nn"])
    assert np.array_equal([w[0] for w in p.wins], g["start"])
    nh = len(p.g) // 2 + 1
    assert np.array_equal(np.concatenate(p.g[:nh]), g["g_half"])
    for k in range(nh, len(p.g)):       # the mirrored bands repeat their sources
        assert np.array_equal(p.g[k], p.g[len(p.g) - k])
    assert np.array_equal(np.concatenate(p.gd), g["gd"])


def stored_slices(name, g):
    """{slice index: concatenated coefficients} of a case's fixture."""
    n = int(g["nslices"])
    if not SR.CASES[name].get("big"):
        return dict(enumerate(g["coef"]))
    first = load("slicq_%s_coef" % name)["coef"]
    return {0: first[0], 1: first[1], n - 1: g["c_last"]}


def stored_rec(name, g):
    return load("slicq_%s_rec" % name)["rec"] if SR.CASES[name].get("big") else g["rec"]


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_planner_equals_the_reference_exactly(name):
    check_planner(SR.plan_of(name), load("slicq_" + name))


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_slices_and_reconstruction_match_the_reference(name):
    p, g = SR.plan_of(name), load("slicq_" + name)
    x, cs, rec = SR.reference_of(name)
    assert len(cs) == int(g["nslices"]) == p.nslices(len(x))
    assert np.array_equal([len(b) for b in cs[0]], g["lens"])
    for s, want in stored_slices(name, g).items():
        r = rel(np.concatenate(cs[s]), want)
        assert r < SR.TIGHT, (name, s, r)
    assert len(rec) == 2 * p.hhop * len(cs) >= len(x)
    want = stored_rec(name, g)
    assert want.shape == x.shape
    assert rel(rec[:len(x)], want) < SR.TIGHT
    assert rel(rec[:len(x)], x) < SR.TIGHT
    assert np.iscomplexobj(rec) == (not SR.CASES[name]["real"])


def test_the_cases_reach_the_arms_they_are_named_for():
    small, big6, big2 = SR.plan_of("small"), SR.plan_of("big6"), SR.plan_of("big2")
    assert small.M.min() == 16 and small.M.max() == 168 and len(small.g) // 2 + 1 == 20
    assert SR.plan_of("matrix").M.min() == SR.plan_of("matrix").M.max()
    assert big6.M.max() == 3452 and big2.M.max() == 5720       # Bluestein past P = 4096
    assert int(np.sum(big6.M[big6.used])) == 21044
    assert big6.nn == 20000 and big6.nslices(100000) == 11 and SR.plan_of("tiny").nslices(2500) == 11
    assert all(np.all(SR.plan_of(n).M % 4 == 0) for n in SR.CASES)
