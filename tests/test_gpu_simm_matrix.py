"""Every reachable instantiation of fasst_simm.hip against the oracle, held
to rounding error elementwise (run on MI355X).

The cases, and the restated dispatch that says which kernels each one
launches, are in simm_matrix_cases.py; test_simm_matrix_cases.py (CPU) fails
when the table stops covering the reachable set.  Each case runs the public
SIMM.Stereo_SIMM / SIMM.SIMM for one and for two iterations (the second takes
the state the first left: SF0 with its scale applied, SMR / SML, WPHI), with
computeError=True where the function has it.

Metric: helpers.rel_elem(got, longdouble oracle, floor=1e-12) per returned
parameter, every element against its own magnitude.  Yardstick: the same
quantity e_ref for the float64 oracle, i.e. what NumPy's own float64
summation order costs on these inputs.  Bound: err <= MARGIN * max(e_ref,
2**-52).  The GPU sums the F- and N-long contractions in another order, with
FMA and Newton-Raphson reciprocals in the fused products, so a factor over
e_ref is expected; MARGIN is the next power of two above the worst measured
err / max(e_ref, 2**-52) over all cases (the SIMM matrix table),
and is capped at 64: a case needing more is a finding, not a reason to widen.

Every case prints 'simm-matrix <case> it=<n> [<arms>] <param>=<err>/<e_ref>'
before asserting.
"""
import ctypes

import numpy as np
import pytest

import simm_matrix_cases as M
from helpers import rel_elem

pytestmark = pytest.mark.gpu

MARGIN = 8      # worst measured 4.51 (st-N255-K4-R7, two iterations, WM); the cap is 64
ULP = 2.0 ** -52
FLOOR = 1e-12


def _S():
    from pyfasst_amd.SeparateLeadStereo.SIMM import SIMM as S
    return S


def _nf0_counts():
    from pyfasst_amd import _lib
    d, k = ctypes.c_long(0), ctypes.c_long(0)
    _lib.check(_lib.lib.simm_nf0_product_counts(ctypes.byref(d), ctypes.byref(k)),
               "simm_nf0_product_counts")
    return d.value, k.value


def _run(case, n_iter):
    SXR, SXL, WF0, WG = M.data(case.shape, case.data_seed, case.zero)
    K, R = case.shape[4:]
    S = _S()
    np.random.seed(case.init_seed)
    if case.stereo:
        return S.Stereo_SIMM(SXR, SXL, WF0, WG, numberOfFilters=K,
                             numberOfAccompanimentSpectralShapes=R, numberOfIterations=n_iter,
                             updateHGAMMA=case.hgamma, computeError=True, verbose=False)
    return S.SIMM(SXR, WF0, WG, numberOfFilters=K, numberOfAccompanimentSpectralShapes=R,
                  numberOfIterations=n_iter, verbose=False)


def _errors(case, n_iter, got, finite_only=False):
    """name -> (err, e_ref) against the longdouble oracle."""
    ref = M.oracle_run(case.id, n_iter, 'longdouble')
    f64 = M.oracle_run(case.id, n_iter, 'float64')
    out = {}
    for name, g, hi, lo in zip(M.names(case), got, ref, f64):
        g = np.asarray(g)
        assert g.shape == hi.shape, name
        if finite_only and hi.ndim:
            ok = np.isfinite(hi)
            g, hi, lo = g[ok], hi[ok], lo[ok]
        out[name] = (rel_elem(g, hi, floor=FLOOR), rel_elem(lo, hi, floor=FLOOR))
    return out


def _report_and_assert(case, n_iter, errs):
    print("simm-matrix %s it=%d [%s] %s" % (
        case.id, n_iter, " ".join(sorted(M.case_arms(case))),
        " ".join("%s=%.3g/%.3g" % (n, errs[n][0], errs[n][1]) for n in M.names(case))))
    for name in M.names(case):
        err, e_ref = errs[name]
        assert err <= MARGIN * max(e_ref, ULP), (case.id, n_iter, name, err, e_ref,
                                                 err / max(e_ref, ULP))


RUNS = [(c, n) for c in M.CASES for n in c.iters]


@pytest.mark.parametrize("case,n_iter", RUNS, ids=["%s-it%d" % (c.id, n) for c, n in RUNS])
def test_simm_arm_vs_longdouble_oracle(monkeypatch, case, n_iter):
    # FASST_SIMM_GEMM is read when the SIMM context is created
    if case.gemm:
        monkeypatch.setenv("FASST_SIMM_GEMM", str(case.gemm))
    else:
        monkeypatch.delenv("FASST_SIMM_GEMM", raising=False)
    d0, k0 = _nf0_counts()
    got = _run(case, n_iter)
    d1, k1 = _nf0_counts()
    # two NF0-sized products per iteration (WF0^T [num | den], SF0 = WF0 HF0)
    # and SF0 once when the model is built, all on the kernel the case names
    n_products = 2 * n_iter + 1
    assert (d1 - d0, k1 - k0) == ((0, n_products) if case.gemm == 2 else (n_products, 0))
    _report_and_assert(case, n_iter, _errors(case, n_iter, got))


def test_simm_zero_frame_and_zero_bin():
    """Frame 3 and bin 7 of both channels are zero: HF0, HPHI and HM lose
    that frame, WM that bin, exactly as in the oracle (whose parameters all
    stay finite), and recoError is infinite in the slots that are filled."""
    case = M.ZERO_CASE
    (n_iter,) = case.iters
    got = _run(case, n_iter)
    ref = M.oracle_run(case.id, n_iter, 'longdouble')
    for name, g, hi in zip(M.names(case), got, ref):
        g = np.asarray(g)
        if name == 'recoError':
            assert np.array_equal(np.isinf(g), np.isinf(hi)), (name, g[:8], hi[:8])
            assert np.array_equal(np.isnan(g), np.isnan(hi)), (name, g[:8], hi[:8])
            assert np.all(g[np.isinf(g)] > 0)
        else:
            assert np.all(np.isfinite(hi)) and np.all(np.isfinite(g)), name
        assert np.array_equal(g == 0, hi == 0), name
    frame, fbin = case.zero
    names = M.names(case)
    for name in ('HPHI', 'HF0', 'HM'):
        assert not np.any(got[names.index(name)][:, frame]), name
    assert not np.any(got[names.index('WM')][fbin])
    _report_and_assert(case, n_iter, _errors(case, n_iter, got, finite_only=True))
