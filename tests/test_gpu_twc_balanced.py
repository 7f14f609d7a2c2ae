"""k_tw_contract_lds under its balanced schedule (pyfasst_amd/csrc/
fasst_twsched.h: persistent blocks, one partial slot per segment) against the
oracle and against the grid form (FASST_TWC_SCHED=grid: the static bin split),
through the normal engine path (run on MI355X).

Shapes are small and awkward: F = 65 / 130 are nft = 5 / 9 bin steps with a
ragged last tile; T = 77 / 200 are ntt = 5 / 13 frame tiles (not a multiple of
the 8 of a frame group, ragged last frame), so G = 1 / 2 groups per source.
With U = J G nft steps, FASST_TWC_NB forces
  NB = 1   one block walks every unit: a prologue / epilogue turn per unit
  NB = 3   ranges that span several units and cut units in the middle
  NB = U   one bin step per block, nft slots per unit
and the default is one round of resident blocks (clamped to U here).

Bounds: those of tests/test_gpu_parity.py::test_em_stft_domain_vs_oracle for
the same quantities (loglik 1e-10, TW / FB 1e-8, relative to the largest
value).  The grid form's own deviation from the oracle on the same case is the
measure: the balanced form's may not exceed 4 x it, the parity bound being the
floor.  Every case prints its deviations ('twc-balanced ...') before asserting.
"""
import os

import numpy as np
import pytest

import fasst_ref as R  # noqa: F401  (the oracle, through test_gpu_parity._c3_like)
from helpers import rel
from test_gpu_parity import _c3_like

pytestmark = pytest.mark.gpu

TOL = {'ll': 1e-10, 'TW': 1e-8, 'FB': 1e-8}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twc_grid_parent.npz")

# name: (F, T, J, K, rank, source with a fixed TW or None)
CASES = {
    'j4k20': (65, 77, 4, 20, 2, None),      # KP = 32, G = 1, U = 20
    'j3k48': (130, 200, 3, 48, 1, 1),       # KP = 64, G = 2, U = 54; source 1's TW fixed
    'j1k16': (65, 200, 1, 16, 2, None),     # KP = 16, G = 2, U = 10
}


def _steps(name):
    F, T, J = CASES[name][:3]
    nft, ntt = (F + 15) // 16, (T + 15) // 16
    return J * ((ntt + 7) // 8) * nft


def _fix_tw(jfix):
    def prep(mod):
        mod.spec_comps[jfix]['factor'][0]['TW_frdm_prior'] = 'fixed'
    return prep


def _dead_tw(mod):   # tiny but non-zero: the mixing solve stays regular
    mod.spec_comps[1]['factor'][0]['TW'][:] = 1e-30


_ORACLE = {}
_RUNS = {}


def _freeze(res):
    for v in res.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return res


def _results(mod, J, ll):
    return _freeze({'ll': np.array(ll),
                    'TW': [np.array(mod.spec_comps[j]['factor'][0]['TW']) for j in range(J)],
                    'FB': [np.array(mod.spec_comps[j]['factor'][0]['FB']) for j in range(J)]})


def _run(key, shape, iters, sched, nb, monkeypatch, capfd, prep=None, seed=None, cache=True):
    """The product's results under one schedule (and the oracle's, once per
    case): sched 'grid' | 'balanced' | None (no knob), nb the forced block
    count or None."""
    F, T, J, K, rank = shape
    rkey = (key, iters, sched, nb)
    if cache and rkey in _RUNS:
        return _RUNS[rkey], _ORACLE[(key, iters)]
    monkeypatch.delenv("FASST_NSPLIT_T", raising=False)
    monkeypatch.setenv("FASST_VERBOSE", "1")
    for name, v in (("FASST_TWC_SCHED", sched), ("FASST_TWC_NB", nb)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    m, o, X = _c3_like(F, T, J, K, rank, iters)
    for mod in (m, o):
        if prep:
            prep(mod)
    if (key, iters) not in _ORACLE:
        if seed is not None:
            np.random.seed(seed)
        _ORACLE[(key, iters)] = _results(o, J, o.estim_param_a_post_model())
    if seed is not None:
        np.random.seed(seed)
    capfd.readouterr()
    res = _results(m, J, m.estim_param_a_post_model())
    err = capfd.readouterr().err
    # the schedule asked for is the one that ran (not clamped or ignored)
    if sched == 'grid':
        assert "persistent blocks" not in err and "splits" in err, err
    else:
        assert "persistent blocks" in err, err
        if nb is not None:
            assert "tw %d persistent blocks" % nb in err, err
    if cache:
        _RUNS[rkey] = res
    return res, _ORACLE[(key, iters)]


def _deviations(got, ref, J):
    d = {'ll': rel(got['ll'], ref['ll'])}
    for name in ('TW', 'FB'):
        for j in range(J):
            assert got[name][j].shape == ref[name][j].shape, (name, j)
        d[name] = max(rel(got[name][j], ref[name][j]) for j in range(J))
    return d


def _check(tag, bal, grid, ref, J):
    db, dg = _deviations(bal, ref, J), _deviations(grid, ref, J)
    print("twc-balanced %s balanced-vs-oracle %s | grid-vs-oracle %s" % (
        tag, " ".join("%s=%.3g" % kv for kv in sorted(db.items())),
        " ".join("%s=%.3g" % kv for kv in sorted(dg.items()))))
    for name, tol in TOL.items():
        assert db[name] < tol, (name, db[name])
        assert db[name] <= max(4.0 * dg[name], tol), (name, db[name], dg[name])


def _nbs(name):
    return [1, 3, _steps(name), None]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_balanced_vs_oracle_and_grid(name, iters, monkeypatch, capfd):
    """One and three GEM iterations at NB = 1, 3, U and the default."""
    shape, jfix = CASES[name][:5], CASES[name][5]
    prep = _fix_tw(jfix) if jfix is not None else None
    J = shape[2]
    grid, ref = _run(name, shape, iters, 'grid', None, monkeypatch, capfd, prep=prep)
    for nb in _nbs(name):
        bal, _ = _run(name, shape, iters, 'balanced', nb, monkeypatch, capfd, prep=prep)
        _check("%s iters=%d NB=%s" % (name, iters, nb), bal, grid, ref, J)


def test_default_is_balanced(monkeypatch, capfd):
    """With no knob the balanced schedule runs, and gives the bits of
    FASST_TWC_SCHED=balanced."""
    shape = CASES['j4k20'][:5]
    a, _ = _run('j4k20', shape, 3, None, None, monkeypatch, capfd, cache=False)
    b, _ = _run('j4k20', shape, 3, 'balanced', None, monkeypatch, capfd)
    assert np.array_equal(a['ll'], b['ll'])
    for j in range(shape[2]):
        assert np.array_equal(a['TW'][j], b['TW'][j])


@pytest.mark.parametrize("nb", [3, None])
def test_balanced_is_deterministic(nb, monkeypatch, capfd):
    """The partials are summed in slot order: two runs with the same NB give
    bit-identical results."""
    shape = CASES['j3k48'][:5]
    prep = _fix_tw(CASES['j3k48'][5])
    a, _ = _run('j3k48', shape, 3, 'balanced', nb, monkeypatch, capfd, prep=prep, cache=False)
    b, _ = _run('j3k48', shape, 3, 'balanced', nb, monkeypatch, capfd, prep=prep, cache=False)
    assert np.array_equal(a['ll'], b['ll'])
    for j in range(shape[2]):
        assert np.array_equal(a['TW'][j], b['TW'][j])
        assert np.array_equal(a['FB'][j], b['FB'][j])


def test_grid_is_the_recorded_kernel(monkeypatch, capfd):
    """FASST_TWC_SCHED=grid is the kernel and launch from before the balanced
    schedule, bit for bit: tests/golden/twc_grid_parent.npz holds the outputs
    of that commit (no knob existed) on the j4k20 case, three iterations."""
    shape = CASES['j4k20'][:5]
    got, _ = _run('j4k20', shape, 3, 'grid', None, monkeypatch, capfd)
    with np.load(GOLDEN) as g:
        assert np.array_equal(got['ll'], g['ll'])
        for j in range(shape[2]):
            assert np.array_equal(got['TW'][j], g['TW%d' % j])
            assert np.array_equal(got['FB'][j], g['FB%d' % j])


@pytest.mark.parametrize("nb", [3, None])
def test_restart_halts_the_batch(nb, monkeypatch, capfd):
    """A dead TW row block (sum(TW) < eps after the first iteration) raises the
    restart flag: the batch's later iterations, TW contraction and update
    included, return at entry, the host redraws TW and resumes.  The resumed
    iterations read only partials their own contraction wrote: the results
    meet the oracle's as in the unhalted cases."""
    shape = (33, 40, 2, 4, 1)
    key = 'restart'
    grid, ref = _run(key, shape, 5, 'grid', None, monkeypatch, capfd, prep=_dead_tw, seed=11)
    bal, _ = _run(key, shape, 5, 'balanced', nb, monkeypatch, capfd, prep=_dead_tw, seed=11)
    _check("restart NB=%s" % nb, bal, grid, ref, 2)
