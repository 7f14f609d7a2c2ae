"""stereo_NMF (reference SIMM.py:945-1104) on the MI355X, against the
reference's runs (tests/golden/stereo_nmf.npz) and the CPU restatement
(tests/stereo_nmf_ref.py, which test_stereo_nmf_ref_golden.py pins to those
runs bit for bit).  Compute goes through libfasst_hip.so (snmf_*,
include/fasst_simm.h).

Bounds (max-normalised, helpers.rel), DESIGN.md 7.3's rule: 1e-10 against
golden, scaled by the case's sensitivity over the nmf.npz yardstick's
(1.40e-15) and rounded up to one digit where the case is the more sensitive;
1e-9 live; the error vector 1e-10 relative, element by element.  Largest
relative move of the restatement's outputs under a 1e-15 relative perturbation
of SXR / SXL, 5 draws, CPU (tools/relcheck_stereo_nmf.py), betaR / betaL / HM /
WM:
    rand       1.23e-16 1.34e-16 6.30e-16 1.06e-15   -> x1
    omega07    1.39e-16 1.31e-16 3.94e-16 6.93e-16   -> x1
    r1         1.53e-16 0        5.28e-16 4.16e-16   -> x1
    wrongshape 3.68e-16 2.66e-16 7.60e-16 1.31e-15   -> x1
    given      2.80e-16 2.75e-16 6.11e-16 1.97e-15   -> x2 (1.40 x the yardstick)
"""
import functools

import numpy as np
import pytest

from helpers import load, rel
import stereo_nmf_ref as S

pytestmark = pytest.mark.gpu

GOLD_TOL = {'rand': 1e-10, 'omega07': 1e-10, 'r1': 1e-10, 'wrongshape': 1e-10, 'given': 2e-10}
LIVE_TOL = 1e-9
ERR_TOL = 1e-10


def _simm():
    import pyfasst_amd.SeparateLeadStereo.SIMM.SIMM as SIMM
    return SIMM


def _check(res, ref, tol, what):
    for n, a, b in zip(S.NAMES, res, ref):
        assert a.shape == b.shape, (what, n, a.shape, b.shape)
        r = rel(a, b)
        print(what, n, "%.2e" % r)
        assert r < tol, (what, n, r)


@pytest.fixture(scope="module")
def g():
    return load("stereo_nmf")


@pytest.mark.parametrize("case", sorted(S.CASES))
def test_stereo_nmf_golden(g, case, capsys):
    kw = dict(S.case_inputs(case)[2])
    for k in ('WM0', 'HM0'):
        if case + '_' + k in g:
            kw[k] = g[case + '_' + k]
    np.random.seed(int(g[case + '_seed']))
    res = _simm().stereo_NMF(g[case + '_SXR'], g[case + '_SXL'], **kw)
    assert np.random.rand() == float(g[case + '_rand'])
    said = capsys.readouterr().out
    assert ("Wrong dimensions for given WM0" in said) == (case == 'wrongshape')
    _check(res, [g['%s_%s' % (case, n)] for n in S.NAMES], GOLD_TOL[case], case)


# smallest with R = 1; nothing a multiple of 16; the pipeline's R; several bin
# tiles and frame chunks; the ceiling (two output slabs); exact tiles
LIVE = [(33, 17, 1, 3), (65, 90, 5, 3), (129, 70, 40, 2), (257, 301, 10, 2), (70, 45, 128, 2),
        (64, 64, 16, 3)]


@functools.lru_cache(maxsize=None)
def _live_ref(F, N, R, niter, omega=1.0):
    """data, the seed, and the restatement's run (computed once, read only)"""
    SXR, SXL = S.make_data(F + N + R, F, N, R=min(R, 6))
    seed = 7 * F + N
    np.random.seed(seed)
    ref = S.stereo_NMF(SXR, SXL, R, numberOfIterations=niter, updateRulePower=omega)
    after = np.random.rand()
    for a in (SXR, SXL) + tuple(ref):
        a.setflags(write=False)
    return SXR, SXL, seed, ref, after


@pytest.mark.parametrize("F,N,R,niter", LIVE)
def test_stereo_nmf_vs_restatement(F, N, R, niter):
    SXR, SXL, seed, ref, after = _live_ref(F, N, R, niter)
    assert all(np.all(np.isfinite(a)) for a in ref)
    np.random.seed(seed)
    res = _simm().stereo_NMF(SXR, SXL, R, numberOfIterations=niter)
    # same draw (a different one could not pass the comparison), and the global
    # stream left where the restatement leaves it
    assert np.random.rand() == after
    assert res[0].shape == res[1].shape == (R, R)
    assert np.array_equal(res[0], np.diag(np.diag(res[0])))
    _check(res, ref[:4], LIVE_TOL, "live %s" % ((F, N, R),))


def test_stereo_nmf_omega(capsys):
    F, N, R, niter = 65, 90, 5, 3
    SXR, SXL, seed, ref, after = _live_ref(F, N, R, niter, 0.7)
    np.random.seed(seed)
    res = _simm().stereo_NMF(SXR, SXL, R, numberOfIterations=niter, updateRulePower=0.7)
    assert np.random.rand() == after
    _check(res, ref[:4], LIVE_TOL, "omega 0.7")
    assert rel(ref[3], _live_ref(F, N, R, niter)[3][3]) > 1e-3      # the power is applied


def _start(F, N, R, seed):
    rs = np.random.RandomState(seed)
    return np.abs(rs.randn(F, R)) + 0.05, np.abs(rs.randn(R, N)) + 0.05, rs.rand(R)


def _run_dev(SXR, SXL, WM, HM, bR, niter, omega, err=True):
    from pyfasst_amd import _lib
    return _simm()._stereo_nmf_run(SXR, SXL, WM, HM, bR, niter, omega, err, _lib.default_device())


def test_stereo_nmf_small_model_takes_the_second_clamp():
    """Half the bins carry 1e-13 of the energy and start from WM rows of 1e-12:
    hat < 1e-10 there, so max(hat ** 2, eps) is the eps branch from the first
    step on (SIMM.py:1023), while max(hat, eps) is not."""
    F, N, R, niter = 65, 90, 5, 3
    SXR, SXL = S.make_data(5, F, N)
    WM, HM, bR = _start(F, N, R, 6)
    SXR[:F // 2] *= 1e-13
    SXL[:F // 2] *= 1e-13
    WM[:F // 2] *= 1e-12
    hat = S._model(WM, HM, np.diag(bR))
    assert np.all(hat[:F // 2] < 1e-10) and np.all(hat[:F // 2] > 1e-18)
    assert np.all(hat[F // 2:] > 1e-6)
    ref = S.iterate(SXR, SXL, WM.copy(), HM.copy(), np.diag(bR), niter, 1.0)
    assert all(np.all(np.isfinite(a)) for a in ref)
    bRd, bLd, HMd, WMd, err = _run_dev(SXR, SXL, WM, HM, bR, niter, 1.0)
    _check((np.diag(bRd), np.diag(bLd), HMd, WMd), ref[:4], LIVE_TOL, "clamp")
    # WM's small rows against their own magnitude, not the plane's maximum
    assert rel(WMd[:F // 2], ref[3][:F // 2]) < LIVE_TOL
    assert np.max(np.abs(err - ref[4]) / np.abs(ref[4])) < ERR_TOL


@pytest.mark.parametrize("F,N,R,niter", [(65, 90, 5, 3), (129, 70, 40, 2), (70, 45, 128, 2)])
def test_stereo_nmf_error_vector(F, N, R, niter):
    SXR, SXL = S.make_data(F + R, F, N, R=min(R, 6))
    WM, HM, bR = _start(F, N, R, F)
    ref = S.iterate(SXR, SXL, WM.copy(), HM.copy(), np.diag(bR), niter, 1.0)
    with_err = _run_dev(SXR, SXL, WM, HM, bR, niter, 1.0)
    err = with_err[4]
    assert err.shape == (3 * niter + 1,)
    r = np.max(np.abs(err - ref[4]) / np.abs(ref[4]))
    print("error vector %.2e" % r, err)
    assert r < ERR_TOL
    # asking for the error vector does not change the parameters
    without = _run_dev(SXR, SXL, WM, HM, bR, niter, 1.0, err=False)
    assert without[4] is None
    assert all(np.array_equal(a, b) for a, b in zip(with_err[:4], without[:4]))


@pytest.mark.parametrize("F,N,R", [(257, 301, 10), (70, 45, 128)])
def test_stereo_nmf_two_runs_bit_equal(F, N, R):
    SXR, SXL = S.make_data(3, F, N)
    WM, HM, bR = _start(F, N, R, 4)
    a = _run_dev(SXR, SXL, WM, HM, bR, 2, 1.0)
    b = _run_dev(SXR, SXL, WM, HM, bR, 2, 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_stereo_nmf_verbose_prints_the_reference_lines(capsys):
    SXR, SXL = S.make_data(8, 33, 17)
    np.random.seed(1)
    _simm().stereo_NMF(SXR, SXL, 3, numberOfIterations=2, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("Reconstruction error at beginning:  ")
    assert out[1] == "iteration  0  over  2"
    assert [l[:43] for l in out[2:5]] == ["Reconstruction error difference after HM   ",
                                          "Reconstruction error difference after WM   ",
                                          "Reconstruction error difference after BETA "]
    assert len(out) == 1 + 2 * 4
    assert all(np.isfinite(float(l.split(":")[1])) for l in out if ":" in l)


def test_stereo_nmf_refusals_leave_the_stream_alone(capsys):
    SIMM = _simm()
    SXR, SXL = S.make_data(9, 33, 17)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    with pytest.raises(NotImplementedError, match="displayEvolution"):
        SIMM.stereo_NMF(SXR, SXL, 3, displayEvolution=True)
    with pytest.raises(NotImplementedError, match="128"):
        SIMM.stereo_NMF(SXR, SXL, 129)
    with pytest.raises(ValueError, match="Dimension of STFT matrices must be the same."):
        SIMM.stereo_NMF(SXR, SXL[:, :-1], 3)
    assert "The input STFT matrices do not have the same dimension." in capsys.readouterr().out
    assert np.array_equal(np.random.get_state()[1], state)
    # the engine's own limit, for a caller of the C ABI
    import ctypes
    from pyfasst_amd import _lib
    ptr = ctypes.c_void_p()
    assert _lib.lib.snmf_create(_lib.default_device(), 33, 17, 129,
                                ctypes.byref(ptr)) == _lib.FASST_ERR_UNSUPPORTED
    assert "128" in _lib.last_error()


def test_stereo_nmf_is_served_under_the_reference_name():
    import pyfasst.SeparateLeadStereo.SIMM.SIMM as ref_name
    import pyfasst.tools.distances as dist
    import pyfasst_amd.tools.distances as dist2
    assert ref_name.stereo_NMF is _simm().stereo_NMF
    assert dist.ISDistortion is dist2.ISDistortion
    X = np.array([[1.0, 2.0], [3.0, 0.5]])
    assert dist.ISDistortion(X, X) == 0.0
    assert dist.ISDistortion(X, 2 * X) == S.ISDistortion(X, 2 * X)
