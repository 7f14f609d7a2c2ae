"""pyfasst_amd.tftransforms.slicq on the GPU against the reference's fixtures
tests/golden/slicq_*.npz and the NumPy restatement tests/slicq_ref.py.

Bound: slicq_ref.TIGHT = 1e-9 relative to the largest magnitude of the
compared array (FP64 throughout; the reference's own round trip is at 4e-16 to
7e-16 on these cases).  Everything that compares two runs of the device
(block splits, slices per call, channels, the tensor route, repeats) is held
to bit equality.
"""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import slicq_ref as SR
from helpers import load, rel
from test_slicq_ref_golden import check_planner, stored_rec, stored_slices

pytestmark = pytest.mark.gpu

TIGHT = SR.TIGHT
_cache = {}


def make(name, **over):
    from pyfasst_amd.tftransforms.slicq import CQ_NSGT_sliced
    c = SR.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CQ_NSGT_sliced(c["fmin"], c["fmax"], c["bins"], c["sl_len"], c["tr_area"], c["fs"],
                              **dict(SR.options(c), **over))


def setup(name):
    """(transform, its coefficients per slice, its reconstruction of them),
    computed once per case and shared: do not modify."""
    if name not in _cache:
        t = make(name)
        cs = list(t.forward((SR.signal(name),)))
        _cache[name] = (t, cs, np.concatenate(list(t.backward(cs))))
    return _cache[name]


def flat(cs):
    return np.array([np.concatenate(c) for c in cs])


def split(row, lens):
    return np.split(row, np.cumsum(lens)[:-1])


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_planner_equals_the_reference_exactly(name):
    t = make(name)
    check_planner(t, load("slicq_" + name))
    assert t._plan is None          # planning touches no device
    c = SR.CASES[name]
    assert (t.sl_len, t.tr_area, t.nn) == (c["sl_len"], c["tr_area"], c["sl_len"])
    assert len(t.frqs) == len(t.q) and len(t.wins) == len(t.g) == len(t.gd) == len(t.M)


@pytest.mark.parametrize("name", SR.SMALL_CASES)
def test_forward_matches_the_fixture_slice_by_slice_and_band_by_band(name):
    t, cs, _ = setup(name)
    g = load("slicq_" + name)
    assert len(cs) == int(g["nslices"]) == t.nslices(SR.CASES[name]["L"])
    worst = 0.0
    for s, (got, want) in enumerate(zip(cs, g["coef"])):
        assert [len(b) for b in got] == list(g["lens"])
        top = np.max(np.abs(want))
        for k, (gb, wb) in enumerate(zip(got, split(want, g["lens"]))):
            assert gb.dtype == np.complex128
            r = float(np.max(np.abs(gb - wb)) / top)
            worst = max(worst, r)
            assert r < TIGHT, (name, s, k, r)
    print("slicq parity forward %s %.3e" % (name, worst))


@pytest.mark.parametrize("name", SR.BIG_CASES)
def test_forward_of_the_big_cases_matches_the_restatement_and_the_fixture(name):
    t, cs, _ = setup(name)
    _, want, _ = SR.reference_of(name)
    assert len(cs) == len(want)
    worst = 0.0
    for s, (got, wc) in enumerate(zip(cs, want)):
        top = max(np.max(np.abs(b)) for b in wc)
        for k, (gb, wb) in enumerate(zip(got, wc)):
            assert gb.shape == wb.shape
            r = float(np.max(np.abs(gb - wb)) / top)
            worst = max(worst, r)
            assert r < TIGHT, (name, s, k, r)
    for s, wrow in stored_slices(name, load("slicq_" + name)).items():
        assert rel(np.concatenate(cs[s]), wrow) < TIGHT
    print("slicq parity forward %s %.3e" % (name, worst))


@pytest.mark.parametrize("name", SR.SMALL_CASES)
def test_backward_of_the_fixture_coefficients(name):
    t, _, _ = setup(name)
    g = load("slicq_" + name)
    L = SR.CASES[name]["L"]
    blocks = list(t.backward([split(row, g["lens"]) for row in g["coef"]]))
    assert len(blocks) == int(g["nslices"])
    assert all(b.shape == (2 * t.hhop,) for b in blocks)
    y = np.concatenate(blocks)
    assert np.iscomplexobj(y) == (not SR.CASES[name]["real"])
    r = rel(y[:L], g["rec"])
    print("slicq parity backward %s %.3e" % (name, r))
    assert r < TIGHT


@pytest.mark.parametrize("name", SR.BIG_CASES)
def test_backward_of_the_restatements_coefficients(name):
    t, _, _ = setup(name)
    x, want, wrec = SR.reference_of(name)
    y = np.concatenate(list(t.backward(want)))
    assert y.shape == wrec.shape
    r = rel(y, wrec)
    r2 = rel(y[:len(x)], stored_rec(name, load("slicq_" + name)))
    print("slicq parity backward %s %.3e %.3e" % (name, r, r2))
    assert r < TIGHT and r2 < TIGHT


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_round_trip_returns_the_signal(name):
    t, cs, y = setup(name)
    x = SR.signal(name)
    assert len(y) == 2 * t.hhop * len(cs) >= len(x)
    r = rel(y[:len(x)], x)
    print("slicq parity roundtrip %s %.3e" % (name, r))
    assert r < TIGHT
    assert rel(y[len(x):], np.zeros(len(y) - len(x))) < TIGHT * np.max(np.abs(x))


@pytest.mark.parametrize("name", ["small", "complex"])
def test_input_block_splits_do_not_change_a_bit(name):
    t, cs, _ = setup(name)
    x = SR.signal(name)
    got = list(t.forward((x[:700], x[700:701], x[701:])))
    assert np.array_equal(flat(got), flat(cs))
    lazy = list(t.forward(x[a:a + 97] for a in range(0, len(x), 97)))
    assert np.array_equal(flat(lazy), flat(cs))


@pytest.mark.parametrize("name", ["small", "complex", "recwnd", "tiny"])
@pytest.mark.parametrize("per", [1, 3])
def test_slices_per_call_does_not_change_a_bit(name, per):
    """7 and 11 slices in calls of 1 and of 3: calls that start on odd slices
    (a nonzero first_slice_index parity) and a last call that is not full,
    against one call of all slices."""
    t, cs, y = setup(name)
    assert len(cs) % 2 == 1 and t.slices_per_call >= len(cs)
    u = make(name, slices_per_call=per)
    got = list(u.forward((SR.signal(name),)))
    assert np.array_equal(flat(got), flat(cs))
    assert np.array_equal(np.concatenate(list(u.backward(cs))), y)


@pytest.mark.parametrize("name", ["small", "complex", "big6"])
def test_two_backward_runs_are_bit_equal(name):
    t, cs, y = setup(name)
    assert np.array_equal(np.concatenate(list(t.backward(cs))), y)


@pytest.mark.parametrize("name", ["small", "complex"])
def test_multichannel_is_the_single_channel_transform_of_each_channel(name):
    t, cs, y = setup(name)
    x = SR.signal(name)
    x2 = np.cos(np.arange(len(x)) * 0.37) * x[::-1]
    single = make(name, slices_per_call=3)
    cs2 = list(single.forward((x2,)))
    y2 = np.concatenate(list(single.backward(cs2)))
    m = make(name, multichannel=True, slices_per_call=2)
    both = np.array([x, x2])
    got = list(m.forward((both[:, :1000], both[:, 1000:])))
    assert len(got) == len(cs) and all(isinstance(it, tuple) and len(it) == 2 for it in got)
    assert np.array_equal(flat([it[0] for it in got]), flat(cs))
    assert np.array_equal(flat([it[1] for it in got]), flat(cs2))
    blocks = list(m.backward(got))
    assert all(b.shape == (2, 2 * m.hhop) for b in blocks)
    ym = np.concatenate(blocks, axis=1)
    assert np.array_equal(ym[0], y) and np.array_equal(ym[1], y2)


def test_launch_count_does_not_grow_with_the_slices():
    """One call of 3 slices and one of 11 launch the same number of kernels:
    those of the plain transform plus one (k_slice, k_unslice)."""
    from pyfasst_amd.tftransforms.nsgt import _device
    t = make("small")
    rs = np.random.RandomState(5)
    fwd, bwd = [], []
    for L, n in ((1024, 3), (5120, 11)):
        x = rs.randn(L)
        cs = list(t.forward((x,)))        # builds the plan (its table launches) first
        assert len(cs) == n
        n0 = _device.launch_count()
        list(t.forward((x,)))
        n1 = _device.launch_count()
        list(t.backward(cs))
        fwd.append(n1 - n0)
        bwd.append(_device.launch_count() - n1)
    assert fwd[0] == fwd[1] and bwd[0] == bwd[1], (fwd, bwd)
    # the whole-signal transform on the same windows: one launch fewer each way
    plain = _device.DevicePlan(t.g, t.gd, t.wins, t.nn, t.M, t.sl_len, t.real, t.reducedform)
    c = plain.forward(rs.randn(1, t.sl_len))
    n0 = _device.launch_count()
    plain.forward(rs.randn(1, t.sl_len))
    n1 = _device.launch_count()
    plain.backward(c)
    n2 = _device.launch_count()
    assert fwd[0] == n1 - n0 + 1 and bwd[0] == n2 - n1 + 1, (fwd, bwd, n1 - n0, n2 - n1)


@pytest.mark.parametrize("name", ["small", "complex"])
def test_functional_forms_on_cut_slices_match_the_restatement(name):
    """nsgtf_sl / nsigtf_sl: the per-slice transforms without rotation."""
    from pyfasst_amd.tftransforms.slicq import nsgtf_sl, nsigtf_sl
    p = SR.plan_of(name)
    slices = p.slices(SR.signal(name))
    want = [p.forward(sl) for sl in slices]
    got = list(nsgtf_sl(iter(slices), p.g, p.wins, p.nn, p.M, real=p.real))
    assert len(got) == len(want)
    rf = max(rel(np.concatenate(gc), np.concatenate(wc)) for gc, wc in zip(got, want))
    back = list(nsigtf_sl(iter(want), p.gd, p.wins, p.nn, p.sl_len, real=p.real))
    rb = max(rel(gy, p.backward(wc)) for gy, wc in zip(back, want))
    print("slicq parity functional %s %.3e %.3e" % (name, rf, rb))
    assert rf < TIGHT and rb < TIGHT
    assert all(gy.shape == (p.sl_len,) and np.iscomplexobj(gy) == (not p.real) for gy in back)


def test_refusals():
    from pyfasst_amd import _lib
    from pyfasst_amd.tftransforms import nsgt, slicq
    with pytest.raises(ValueError, match="multiple of 4"):
        slicq.CQ_NSGT_sliced(200, 3500, 4, 1022, 128, 8000)
    with pytest.raises(ValueError, match="tr_area"):
        slicq.CQ_NSGT_sliced(200, 3500, 4, 1024, 127, 8000)
    with pytest.raises(ValueError, match="tr_area"):
        slicq.CQ_NSGT_sliced(200, 3500, 4, 1024, 512, 8000)
    with pytest.raises(ValueError, match="multiples of 4"):
        slicq.CQ_NSGT_sliced(200, 3500, 4, 1024, 128, 8000, min_win=18)
    with pytest.raises(ValueError, match="reducedform"):
        slicq.CQ_NSGT_sliced(200, 3500, 4, 1024, 128, 8000, reducedform=3)
    with pytest.raises(NotImplementedError, match="ceiling"):
        slicq.CQ_NSGT_sliced(200, 3500, 4, (1 << 23) + 4, 128, 8000)
    with pytest.raises(NotImplementedError, match="pyfasst_amd.tftransforms.slicq"):
        nsgt.NSGT_sliced(nsgt.OctScale(50, 4000, 12), 4096, 1024, 8000)
    with pytest.raises(NotImplementedError, match="pyfasst_amd.tftransforms.slicq"):
        nsgt.CQ_NSGT_sliced(50, 4000, 12, 4096, 1024, 8000)
    f, q = nsgt.OctScale(50, 4000, 12)()
    with pytest.raises(NotImplementedError, match="pyfasst_amd.tftransforms.slicq"):
        nsgt.nsgfwin(f, q, 8000, 4096, sliced=True)
    t, cs, _ = setup("small")
    with pytest.raises(ValueError, match="bands"):
        list(t.backward([cs[0][:-1]]))
    with pytest.raises(ValueError, match="empty"):
        list(t.forward((np.zeros(0),)))
    # the ABI refuses more than 65535 slices x channels a call, on the host
    x = np.zeros(8)
    st = _lib.lib.fasst_nsgt_sliced_forward(t.plan._h, 2, 40000, 0, _lib.dptr(x), 8, 0, _lib.dptr(x))
    assert st == _lib.FASST_ERR_SHAPE and "65535" in _lib.last_error()
    st = _lib.lib.fasst_nsgt_sliced_backward(t.plan._h, 2, 40000, 0, _lib.dptr(x), _lib.dptr(x), 0,
                                             _lib.dptr(x), 8)
    assert st == _lib.FASST_ERR_SHAPE and "65535" in _lib.last_error()


@pytest.fixture(scope="module")
def torch_child():
    """tests/slicq_torch_child.py, once: the tensor route needs a process in
    which torch initialised the GPU before the library did."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "slicq_torch_child.py")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("name", ["small", "complex", "recwnd", "stereo"])
def test_torch_tensors_in_tensors_out_bit_equal(torch_child, name):
    """A CUDA tensor in, tensors out on that device (the coefficient buffer
    [nslices, (nchan,) coef_len] and the offsets of its bands), equal to the
    NumPy route bit for bit."""
    r = torch_child[name]
    assert r["tensor_out"] and r["shapes_ok"]
    assert r["forward_bit_equal"] and r["backward_bit_equal"]
    assert r["scaled"] < TIGHT
