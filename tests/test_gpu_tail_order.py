"""The mixing update's place in the fused-tail iteration (DESIGN.md section
3.3a; FASST_MIX_SIDE, read when a context is created): by default k_mix runs
on the side stream beside the FB contraction, with FASST_MIX_SIDE=0 on the
main stream before it.  Only the order across the two streams changes, no
summation order: both must give the same bits, through halted batches and
singular mixing solves included."""
import numpy as np
import pytest

import fasst_ref as R
from helpers import rel
from test_gpu_fast_tail import _dead_tw, _models

pytestmark = pytest.mark.gpu

PARENT = "0"
# (FASST_MIX_SIDE, FASST_FAST_TAIL): the default, and the tail that leaves the
# next iteration's prep to the side stream beside the E-step
ORDERS = [("1", "2"), ("1", "1")]

SHAPES = [
    # (F, T, J, K, rank, iters), conv
    ((65, 77, 4, 32, 2, 6), True),     # several bin tiles and TW-update blocks, ragged last frame tile
    ((33, 130, 2, 16, 1, 6), False),   # 'inst' mixing (k_mix, then k_mix_inst)
]


def _params(m, J):
    out = []
    for j in range(J):
        fac = m.spec_comps[j]['factor'][0]
        out += [np.array(fac[key]) for key in ('FB', 'FW', 'TW')]
        out.append(np.array(m.spat_comps[j]['params']))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y)
                                    for x, y in zip(a, b))


def _run(monkeypatch, order, ftail, args, conv, prep=None, seed=None):
    monkeypatch.setenv("FASST_MIX_SIDE", order)
    monkeypatch.setenv("FASST_FAST_TAIL", ftail)
    m, o, X = _models(*args, conv=conv)
    if prep:
        prep(m)
        prep(o)
    if seed is not None:
        np.random.seed(seed)
    ll = m.estim_param_a_post_model()
    return m, o, ll


_parent = {}


def _parent_run(monkeypatch, ftail, args, conv):
    """k_mix on the main stream, computed once per (tail form, shape)"""
    key = (ftail, args, conv)
    if key not in _parent:
        m, _, ll = _run(monkeypatch, PARENT, ftail, args, conv)
        _parent[key] = (np.array(ll), _params(m, args[2]))
    return _parent[key]


@pytest.mark.parametrize("order,ftail", ORDERS, ids=lambda v: str(v))
@pytest.mark.parametrize("args,conv", SHAPES, ids=["conv65x77", "inst33x130"])
def test_orders_give_the_same_bits(monkeypatch, args, conv, order, ftail):
    ll0, p0 = _parent_run(monkeypatch, ftail, args, conv)
    m, _, ll = _run(monkeypatch, order, ftail, args, conv)
    assert np.all(np.isfinite(ll))
    assert np.array_equal(np.asarray(ll), ll0)
    assert _same(_params(m, args[2]), p0)


@pytest.mark.parametrize("order,ftail", ORDERS, ids=lambda v: str(v))
def test_restart_halts_the_batch_then_second_run(monkeypatch, order, ftail):
    """sum(TW) < eps after the first iteration (the restart case of
    test_gpu_fast_tail.py): k_renorm_tail raises the flag, the batch's later
    kernels -- the side stream's k_mix among them -- return at entry,
    fasst_run rebuilds W.  Then the model runs again: the w_ready /
    prep_ready hand-over starts from the parameters."""
    args = (33, 40, 2, 4, 1, 5)
    m0, o, ll0 = _run(monkeypatch, PARENT, ftail, args, True, prep=_dead_tw, seed=11)
    m1, _, ll1 = _run(monkeypatch, order, ftail, args, True, prep=_dead_tw, seed=11)
    np.random.seed(11)
    llo = o.estim_param_a_post_model()
    assert np.array_equal(ll1, ll0)
    assert _same(_params(m1, 2), _params(m0, 2))
    assert rel(ll1, llo) < 1e-10
    ll0b = m0.estim_param_a_post_model()
    ll1b = m1.estim_param_a_post_model()
    llob = o.estim_param_a_post_model()
    assert np.array_equal(ll1b, ll0b)
    assert _same(_params(m1, 2), _params(m0, 2))
    assert rel(ll1b, llob) < 1e-10


def _device_spectral(m, J, K):
    return [np.array(x) for j in range(J) for x in m._engine.get_spectral(j, K)]


@pytest.mark.parametrize("conv", [True, False], ids=["conv", "inst"])
def test_singular_mixing_solve_same_error_same_iteration(monkeypatch, conv):
    """A silent source (the inputs of test_gpu_parity.py's singular case)
    makes the first iteration's mixing solve singular: LinAlgError under both
    orders, and in both the halt reaches the iteration's first parameter
    update -- the device's FB / FW / TW are still the uploaded ones, bit for
    bit, so no later kernel of that or a later iteration ran."""
    args = (33, 40, 2, 4, 2, 3)
    left = {}
    for order in (PARENT, "1"):
        monkeypatch.setenv("FASST_MIX_SIDE", order)
        m, o, _ = _models(*args, conv=conv)
        m.spec_comps[1]['factor'][0]['FB'][:] = 0.0
        before = [np.array(m.spec_comps[j]['factor'][0][key]) for j in range(2)
                  for key in ('FB', 'FW', 'TW')]
        with pytest.raises(np.linalg.LinAlgError, match="Singular"):
            m.estim_param_a_post_model()
        left[order] = _device_spectral(m, 2, 4)
        assert _same(left[order], before), order
    assert _same(left["1"], left[PARENT])
