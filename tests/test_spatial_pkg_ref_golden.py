"""The NumPy restatement tests/spatial_pkg_ref.py against the reference's own
numbers (tests/golden/spatial_pkg.npz, written by make_golden_spatial_pkg.py
with `np`, `soundCelerity = 340.` and `inv_mat = inv_herm_mat_2d` bound in the
reference's steering_vectors module).  CPU only; everything bit for bit.
"""
import os

import numpy as np
import pytest

import spatial_pkg_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_pkg.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", sorted(S.ULA_CASES))
def test_steer_ula_bit_equal(g, name):
    for i, th in enumerate(S.ULA_THETAS):
        a = S.steer_ula(S.FREQS33, S.ULA_CASES[name], th, S.ULA_DIST)
        assert same(a, g['ula_%s_%d' % (name, i)]), i


def test_steer_acous_bit_equal(g):
    assert same(S.steer_acous(S.FREQS33, S.ACOUS_DIST), g['acous'])


@pytest.mark.parametrize("name", sorted(S.DD_CASES))
def test_dir_diag_stereo_bit_equal(g, name):
    Cx, kw = S.dd_input(name)
    if int(g['dd_%s_raised' % name]):
        with pytest.raises(ValueError, match="singular covariance"):
            S.dir_diag_stereo(Cx, **kw)
        return
    d, th = S.dir_diag_stereo(Cx, **kw)
    assert same(d, g['dd_%s_diagram' % name]) and same(th, g['dd_%s_theta' % name])
    assert same(S.cx_tmean(Cx), g['dd_%s_mean' % name])


def test_which_covariance_the_reference_refuses(g):
    """An all-zero bin does not raise: inv_herm_mat_2d's clamp makes its
    determinant eps, and the diagram is 0 there.  Only det + eps == 0 gives a
    determinant of exactly 0 (the 'singular' case)."""
    assert int(g['dd_zero_bin_raised']) == 0 and int(g['dd_singular_raised']) == 1
    assert np.all(g['dd_zero_bin_diagram'][:, 5] == 0)
    Cx, _ = S.dd_input('singular')
    m = S.cx_tmean(Cx)
    assert m[0, 5] == -S.EPS and m[3, 5] == 1 and m[1, 5] == 0 and m[2, 5] == 0


@pytest.mark.parametrize("name", sorted(S.MVDR_CASES))
def test_mvdr_bit_equal(g, name):
    w = S.mvdr_target(*S.mvdr_input(name))
    assert np.all(np.isfinite(w))
    assert same(w, g['mvdr_%s' % name])


@pytest.mark.parametrize("name", sorted(S.mvdr_bad_inputs()))
def test_mvdr_error_branches(g, name):
    t, i, exc = S.mvdr_bad_inputs()[name]
    with pytest.raises(exc) as e:
        S.mvdr_target(t, i)
    assert str(g['mvdr_bad_%s' % name]) == exc.__name__ + ": " + str(e.value)


def test_steer_vec_thetas_bit_equal(g):
    fr, th, A = S.steer_vec_thetas(**S.SVT_KW)
    assert same(fr, g['svt_freqs']) and same(th, g['svt_thetas']) and same(A, g['svt_A'])
    Raa = S.steer_vec_thetas(computeRaa=True, **S.SVT_KW)[3]
    assert same(Raa, g['svt_Raa'])


@pytest.mark.parametrize("n", S.ULAD_SENSORS)
def test_ula_diagram_bit_equal(g, n):
    kw = dict(S.ULAD_KW, n_sensors=n)
    th, fr, d = S.ula_diagram(theta_filter=np.pi / 4., **kw)
    assert same(th, g['ulad_%d_thetas' % n]) and same(fr, g['ulad_%d_freqs' % n])
    assert same(d, g['ulad_%d_none' % n])
    assert same(S.ula_diagram(w_filter=S.ulad_filter(n), **kw)[2], g['ulad_%d_given' % n])
    with pytest.raises(ValueError) as e:
        S.ula_diagram(w_filter=S.ulad_filter(n)[:, :-1], **kw)
    assert str(e.value) == str(g['ulad_%d_bad' % n])


def test_bounds_are_the_measured_figures():
    """The tolerances of the GPU tests: 16 x the float64 / longdouble
    difference of this restatement over the tests' own shapes, floor 1e-13."""
    m = S.measure()
    print(m)
    for k, v in m.items():
        assert v <= S.MEASURED[k] * 1.001 and v >= S.MEASURED[k] * 0.5, (k, v, S.MEASURED[k])
        assert S.BOUND[k] == max(16 * S.MEASURED[k], 1e-13)
