"""The NumPy restatement tests/nsgt_ref.py against the reference's fixtures
tests/golden/nsgt_*.npz, and the host-side refusals of the fasst_nsgt_* entry
points.  CPU only: no device call is made.
"""
import ctypes

import numpy as np
import pytest

import nsgt_ref as NR
from helpers import load, rel

# both sides are numpy.fft on the same inputs; loose on purpose
TOL = 1e-12


@pytest.fixture(scope="module", params=sorted(NR.CASES))
def case(request):
    name = request.param
    return name, NR.plan_of(name), load("nsgt_" + name)


def test_planning_equals_the_reference_exactly(case):
    _, p, g = case
    assert np.array_equal(p.M, g["M"])
    assert np.array_equal(p.rfbas, g["rfbas"])
    assert p.nn == int(g["nn"])
    assert np.array_equal([w[0] for w in p.wins], g["start"])
    for gi, w in zip(p.g, p.wins):   # a window's bins are consecutive mod nn
        assert np.array_equal(w, (w[0] + np.arange(len(gi))) % p.nn)
    assert np.array_equal(np.concatenate(p.g), g["g"])
    assert np.array_equal(np.concatenate(p.gd), g["gd"])


def test_package_planning_equals_the_reference_exactly(case):
    """The product's planner (pyfasst_amd.tftransforms.nsgt, host NumPy) gives
    the same bits; no device is touched before the first transform."""
    import warnings
    from pyfasst_amd.tftransforms.nsgt import NSGT, MelScale, OctScale
    name, _, g = case
    c = NR.CASES[name]
    scale = (OctScale(c["fmin"], c["fmax"], c["bins"]) if c["kind"] == "oct"
             else MelScale(c["fmin"], c["fmax"], c["bnds"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = NSGT(scale, c["fs"], c["Ls"], real=c["real"], matrixform=c.get("matrixform", False),
                 reducedform=c.get("reducedform", 0), multichannel="nch" in c)
    assert np.array_equal(t.M, g["M"]) and t.nn == int(g["nn"])
    assert np.array_equal([w[0] for w in t.wins], g["start"])
    assert np.array_equal(np.concatenate(t.g), g["g"])
    assert np.array_equal(np.concatenate(t.gd), g["gd"])
    assert t._plan is None


def test_transforms_match_the_reference(case):
    name, p, g = case
    x = NR.signal(name)
    assert np.array_equal(x, g["x"])
    chans = x if x.ndim == 2 else x[None]
    rec = g["rec"] if x.ndim == 2 else g["rec"][None]
    for ch, want_c, want_r in zip(chans, g["coef"], rec):
        c = p.forward(ch)
        assert np.array_equal([len(b) for b in c], g["lens"])
        assert rel(np.concatenate(c), want_c) < TOL
        assert rel(p.backward(c), want_r) < TOL


@pytest.mark.parametrize("seed", [0, 1])
def test_reconstruction_is_exact_to_seven_places(seed):
    """The reference's own check (its unit test on random signals)."""
    rs = np.random.RandomState(seed)
    sig = rs.random_sample(20000)
    fmin = rs.random_sample() * 200 + 1
    fmax = rs.random_sample() * (22048 - fmin) + fmin
    bins = rs.randint(24) + 1
    f, q = NR.oct_scale(fmin, fmax, bins)
    p = NR.Plan(f, q, 44100, len(sig))
    s_r = p.backward(p.forward(sig))
    norm = lambda x: np.sqrt(np.sum(np.abs(np.square(x))))
    assert round(norm(sig - s_r) / norm(sig), 7) == 0


def test_nn_equals_ls_in_the_non_sliced_arm():
    for name in NR.CASES:
        assert NR.plan_of(name).nn == NR.CASES[name]["Ls"]


def test_wideband_has_a_band_past_the_lds_fft():
    assert NR.plan_of("wideband").M.max() > 4096


# ------------------------------------------------------- the C ABI's refusals
def _create(Ls, nn, M, Lg, start, nbands=None, real=0):
    from pyfasst_amd import _lib
    M = np.asarray(M, dtype=np.int32)
    Lg = np.asarray(Lg, dtype=np.int32)
    start = np.asarray(start, dtype=np.int32)
    g = np.ones(max(1, int(np.sum(np.maximum(Lg, 0)))))
    h = ctypes.c_void_p()
    st = _lib.lib.fasst_nsgt_plan_create(-7, Ls, nn, len(M) if nbands is None else nbands,
                                         _lib.iptr(M), _lib.iptr(Lg), _lib.iptr(start),
                                         _lib.dptr(g), _lib.dptr(g), real, 0, ctypes.byref(h))
    return st, _lib.last_error(), h


def test_plan_create_refuses_bad_plans_on_the_host():
    """Device index -7 does not exist: every refusal below comes back before
    any device call, with a message."""
    from pyfasst_amd import _lib
    st, msg, h = _create(100, 100, [8, 8], [8, 8], [0, 50], nbands=0)
    assert st == _lib.FASST_ERR_SHAPE and "nbands 0" in msg and not h.value
    st, msg, h = _create(100, 100, [8, 0], [8, 8], [0, 50])
    assert st == _lib.FASST_ERR_SHAPE and "M 0" in msg and not h.value
    st, msg, h = _create(100, 100, [8, 200], [8, 101], [0, 50])
    assert st == _lib.FASST_ERR_SHAPE and "window of 101 points" in msg and not h.value
    big = (1 << 23) + 1
    st, msg, h = _create(big, big, [8, 8], [8, 8], [0, 50])
    assert st == _lib.FASST_ERR_UNSUPPORTED and "ceiling" in msg and not h.value
    st, msg, h = _create(100, 100, [8, big], [8, 8], [0, 50])
    assert st == _lib.FASST_ERR_UNSUPPORTED and "ceiling" in msg and not h.value
    with pytest.raises(NotImplementedError):
        _lib.check(st, "fasst_nsgt_plan_create")


def test_coef_len_and_fft_refuse_on_the_host():
    """Only the refusals can be shown without a device: a plan needs one to
    exist.  That fasst_nsgt_coef_len answers a live plan (from the plan's host
    fields; its code makes no device call) is checked on the GPU, by
    test_gpu_nsgt.py::test_coef_len_is_the_sum_of_the_kept_bands."""
    from pyfasst_amd import _lib
    n = ctypes.c_long(-1)
    assert _lib.lib.fasst_nsgt_coef_len(None, ctypes.byref(n)) == _lib.FASST_ERR_SHAPE
    x = np.zeros(4, complex)
    assert _lib.lib.fasst_nsgt_fft(-7, 0, -1, _lib.dptr(x), _lib.dptr(x)) == _lib.FASST_ERR_SHAPE
    assert _lib.lib.fasst_nsgt_fft(-7, 4, 0, _lib.dptr(x), _lib.dptr(x)) == _lib.FASST_ERR_SHAPE
    assert (_lib.lib.fasst_nsgt_fft(-7, (1 << 23) + 1, -1, _lib.dptr(x), _lib.dptr(x))
            == _lib.FASST_ERR_UNSUPPORTED)
    assert _lib.lib.fasst_nsgt_forward(None, 1, _lib.dptr(x), 0, _lib.dptr(x)) == _lib.FASST_ERR_SHAPE
    assert _lib.lib.fasst_nsgt_backward(None, 1, _lib.dptr(x), 0, _lib.dptr(x)) == _lib.FASST_ERR_SHAPE
