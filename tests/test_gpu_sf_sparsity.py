"""Sparsity reweighting of the source activations on the GPU (k_sf_bary,
k_sf_sparsify; fasst_sf_set_sparsity / fasst_sf_reweigh / fasst_sf_run_sparse)
against the restatement tests/sf_sparsity_ref.py and the reference's own run
tests/golden/sf_sparse.npz.

Bounds: a reweighed TW against the float64 restatement REWEIGH_TOL (16 x the
restatement's own float64 / longdouble gap on these shapes, 2.4e-13); the
fixture's logliks 1e-10 and its parameters TIGHT = 1e-9 (the restatement's
sensitivity with the schedule on, tools/relcheck_sf.py: 9.0e-15, scales 1e-9
by 9.0e-15 / 2.2e-13 < 1, and the bound never goes below 1e-9); the resident
form against the loop 1e-12."""
import copy

import numpy as np
import pytest

import sf_sparsity_ref as SP
from helpers import load, rel
from sf_ref import PARTS, compare, fixture_oracle, fixture_product, pair
from test_gpu_parity import TIGHT

pytestmark = pytest.mark.gpu

LL_TOL = 1e-10
REWEIGH_TOL = SP.REWEIGH_TOL
RESIDENT_TOL = 1e-12
F0 = 8   # bins of the engine-level models: the reweighting never reads them


def _bare(Ks, T, Ls, sigma, TWs, share=False, profile=False):
    """One-factor components with TW [K, T] on an engine of their own; the
    reweighed TWs (and the launch counts when profiling)."""
    from pyfasst_amd.engine import Engine
    eng = Engine(F0, T)
    J = len(Ks)
    alias = [[(-1, -1, -1)] for _ in Ks]
    if share:
        alias[1][0] = (-1, -1, 0)
    eng.sf_configure([1] * J, False, [[(2, K, False, False, True)] for K in Ks], alias)
    for j, K in enumerate(Ks):
        eng.set_factors(j, 0, np.ones((F0, 2)), np.ones((2, K)), TWs[j])
    eng.sf_set_sparsity(Ls)
    if profile:
        eng.set_profiling(True)
    eng.sf_reweigh(sigma)
    out = [eng.get_factors(j, 0, tw_only=True) for j in range(J)]
    times = eng.kernel_times() if profile else None
    eng.close()
    return (out, times) if profile else out


@pytest.mark.parametrize("K,T,L", SP.BARE_SHAPES)
def test_bare_reweigh_vs_restatement(K, T, L):
    for sigma in SP.bare_sigmas(K):
        TW = SP.bare_tw(K, T)
        got = _bare([K], T, [L], sigma, [TW])[0]
        if K <= 2:
            np.testing.assert_array_equal(got, TW)
            continue
        ref = TW.copy()
        SP.reweigh_tw(ref, L, sigma)
        err = rel(got, ref)
        print("K %d T %d L %d sigma %g: rel err %.3g" % (K, T, L, sigma, err))
        assert err < REWEIGH_TOL, (sigma, err)
        assert not np.array_equal(got, TW)


def test_all_zero_column():
    """Denominator eps x sum of the weights: the track is 0 there, the mask
    finite, the column stays 0 and its neighbours' medians see the 0."""
    K, T, L = 14, 300, 3
    for sigma in SP.bare_sigmas(K):
        TW = SP.bare_tw(K, T, zero_col=150)
        got = _bare([K], T, [L], sigma, [TW])[0]
        ref = TW.copy()
        SP.reweigh_tw(ref, L, sigma)
        assert np.all(np.isfinite(got)) and np.all(got[:, 150] == 0.0)
        assert rel(got, ref) < REWEIGH_TOL, rel(got, ref)


def test_shared_tw_is_multiplied_twice():
    """One TW array in two components (one device buffer): reweighed by the
    first, then by the second on the first's result, as the reference's
    in-place loop does."""
    K, T = 14, 300
    TW = SP.bare_tw(K, T)
    got = _bare([K, K], T, [3, 5], 9.0, [TW, TW], share=True)
    ref = TW.copy()
    SP.reweigh_tw(ref, 3, 9.0)
    once = ref.copy()
    SP.reweigh_tw(ref, 5, 9.0)
    assert rel(got[0], ref) < REWEIGH_TOL, rel(got[0], ref)
    np.testing.assert_array_equal(got[0], got[1])
    assert rel(got[0], once) > 1e-3


def test_components_without_a_length_are_left_alone():
    K, T = 14, 67
    TWs = [SP.bare_tw(K, T), SP.bare_tw(K, T + 0) * 2.0, SP.bare_tw(2, T)]
    got, times = _bare([K, K, 2], T, [0, 4, 3], 9.0, TWs, profile=True)
    np.testing.assert_array_equal(got[0], TWs[0])
    np.testing.assert_array_equal(got[2], TWs[2])       # K <= 2
    ref = TWs[1].copy()
    SP.reweigh_tw(ref, 4, 9.0)
    assert rel(got[1], ref) < REWEIGH_TOL
    assert times["k_sf_bary"][1] == 1 and times["k_sf_sparsify"][1] == 1
    assert times["k_sf_bary"][0] > 0 and times["k_sf_sparsify"][0] > 0   # device time


def test_refused_sigma():
    with pytest.raises(ValueError, match="sigma"):
        _bare([14], 20, [3], 0.0, [SP.bare_tw(14, 20)])


# ---------------------------------------------------------------- the fixture
def _reweigh(m, sigma):
    import pyfasst_amd.audioModel as am
    am.multiChanSourceF0Filter.reweigh_sparsity_constraint(m, sigma)


def _loop(m, sig):
    """The reference's loop body (audioModel.py:2954-2977) with the class's
    own methods."""
    ll = np.ones(m.iter_num)
    for i in range(m.iter_num):
        m.noise['PSD'] = m._annealed_psd(i)
        ll[i] = m.GEM_iteration()
        _reweigh(m, sig[i])
    return ll


def _fixture_model(g, tmp_path):
    m = fixture_product(g, SP.SPARSE_CASE, tmp_path)
    SP.set_sparsity(m, [int(L) for L in g['sparsity']])
    return m


def _params(m):
    out = [np.array(m.spat_comps[j]['params']) for j in sorted(m.spat_comps)]
    for k in sorted(m.spec_comps):
        for i in sorted(m.spec_comps[k]['factor']):
            out += [np.array(m.spec_comps[k]['factor'][i][p]) for p in PARTS]
    return out


def _compare_fixture(m, g, ll, tol):
    assert rel(ll, g['logliks']) < LL_TOL, rel(ll, g['logliks'])
    for j in range(3):
        assert rel(m.spat_comps[j]['params'], g['final_params_%d' % j]) < tol, j
        for i, fac in m.spec_comps[j]['factor'].items():
            for part in PARTS:
                ref = g['final_%s_%d_%d' % (part, j, i)]
                assert rel(fac[part], ref) < tol, (j, i, part, rel(fac[part], ref))


def test_bare_method_on_the_fixture(tmp_path):
    """reweigh_sparsity_constraint of the class on the fixture's initial
    parameters against the reference's two bare applications: TW changed in
    place, the component without a length and every factor 1 untouched."""
    g = load('sf_sparse')
    for sigma in (169., 9.):
        m = _fixture_model(g, tmp_path)
        before = copy.deepcopy(m.spec_comps)
        arrays = [m.spec_comps[k]['factor'][0]['TW'] for k in range(3)]
        _reweigh(m, sigma)
        for k in range(3):
            TW = m.spec_comps[k]['factor'][0]['TW']
            assert TW is arrays[k]
            assert rel(TW, g['rw%d_TW_%d' % (sigma, k)]) < REWEIGH_TOL, (sigma, k)
        np.testing.assert_array_equal(arrays[1], before[1]['factor'][0]['TW'])
        for k in range(2):
            for p in PARTS:
                np.testing.assert_array_equal(m.spec_comps[k]['factor'][1][p],
                                              before[k]['factor'][1][p])


def test_fixture_loop_vs_reference(tmp_path):
    g = load('sf_sparse')
    m = _fixture_model(g, tmp_path)
    sig = SP.sigma_schedule(m)
    ll = _loop(m, sig)
    print("loglik rel err %.3g" % rel(ll, g['logliks']))
    assert rel(m.noise['PSD'], g['final_psd']) < 1e-14
    _compare_fixture(m, g, ll, TIGHT)


def test_resident_form_equals_the_loop(tmp_path):
    g = load('sf_sparse')
    m = _fixture_model(g, tmp_path)
    sig = SP.sigma_schedule(m)
    ll = _loop(m, sig)
    r = _fixture_model(g, tmp_path)
    rows = np.array([r._annealed_psd(i) for i in range(r.iter_num)])
    order, Ks, conv = r._upload()
    r._engine.sf_set_sparsity([int(L) for L in g['sparsity']])
    r._engine.set_profiling(True)
    llr, done, mask = r._engine.sf_run_sparse(rows, r.nmfUpdateCoeff, sig)
    times = r._engine.kernel_times()
    r._engine.set_profiling(False)
    assert done == 4 and mask == 0
    r._download(order, Ks, conv)
    assert times["k_sf_bary"][1] == times["k_sf_sparsify"][1] == 2 * 4
    assert rel(llr, ll) < RESIDENT_TOL, rel(llr, ll)
    for a, b in zip(_params(r), _params(m)):
        assert rel(a, b) < RESIDENT_TOL, rel(a, b)
    _compare_fixture(r, g, llr, TIGHT)


# ---------------------------------------------------------------- restart order
FREE, FIX = 'free', 'fixed'
SRC = (13, 13, (FIX, FIX, FREE), True)


def test_restart_leaves_the_flagged_iteration_unreweighed():
    """Component 0 is sparse; the first sigma is so narrow that the mask's
    maximum underflows in every frame (no division, an all-zero mask), so the
    reweigh after iteration 1 leaves its TW all zero and iteration 2 flags it
    dead.  sf_run_sparse stops there WITHOUT iteration 2's reweigh: the host
    redraws (the reference's redraw is inside GEM_iteration), reweighs at
    sigma[1] and resumes.  The component's mixing parameters and its filter's
    FW are fixed, as in test_gpu_multifactor's forced restart."""
    def setup(mod):
        mod.spat_comps[0]['frdm_prior'] = FIX
        SP.set_sparsity(mod, [3, False, False])
    spec = {0: [SRC, (13, 3, (FIX, FIX, FREE))], 1: [SRC, (13, 3, (FIX, FREE, FREE))]}
    m, o, X = pair(65, 67, 3, 4, 1, 4, False, spec, setup=setup)
    sig = np.array([1e-12, 60., 25., 9.])
    # the restatement: the state each iteration leaves before its reweigh
    snap = {}
    o.iter_num = 4

    def step(i, mod):
        snap[i] = (copy.deepcopy(mod.spat_comps), copy.deepcopy(mod.spec_comps),
                   list(mod.restarted))
        SP.reweigh_sparsity_constraint(mod, sig[i])
    np.random.seed(11)
    llo = o.estim_param_a_post_model(callback=step)
    assert not snap[0][2] and (0, 0) in snap[1][2]
    assert not np.any(snap[1][1][1]['factor'][0]['TW'] == 0)

    rows = np.array([m._annealed_psd(i) for i in range(4)])
    lengths = [3, 0, 0]
    order, Ks, conv = m._upload()
    eng = m._engine
    eng.sf_set_sparsity(lengths)
    eng.set_profiling(True)
    ll = np.ones(4)
    l0, done, mask = eng.sf_run_sparse(rows, m.nmfUpdateCoeff, sig)
    times = eng.kernel_times()
    eng.set_profiling(False)
    assert done == 2 and mask & 1
    ll[:2] = l0
    # one reweigh ran (after iteration 1), none after the flagged iteration
    assert times["k_sf_bary"][1] == 1 and times["k_sf_sparsify"][1] == 1
    m._download(order, Ks, conv)
    assert np.all(m.spec_comps[0]['factor'][0]['TW'] == 0)
    # the other components as iteration 2 left them, before any reweigh
    for k in (1, 2):
        for i, fac in m.spec_comps[k]['factor'].items():
            for p in PARTS:
                assert rel(fac[p], snap[1][1][k]['factor'][i][p]) < TIGHT, (k, i, p)
    np.random.seed(11)
    m._restart_tw(mask, order)
    order, Ks, conv = m._upload()
    eng.sf_set_sparsity(lengths)
    eng.sf_reweigh(sig[1])
    l1, done, mask = eng.sf_run_sparse(rows[2:], m.nmfUpdateCoeff, sig[2:])
    assert done == 2 and mask == 0
    ll[2:] = l1
    m._download(order, Ks, conv)
    compare(m, o, ll, llo, LL_TOL, TIGHT)


# ---------------------------------------------------------------- isolation
def test_model_without_sparsity_launches_neither_kernel(tmp_path):
    g = load('sf_sparse')
    m = fixture_product(g, SP.SPARSE_CASE, tmp_path)
    SP.set_sparsity(m, [False, False, False])
    m._upload()
    m._engine.set_profiling(True)
    m.estim_param_a_post_model()
    _reweigh(m, 9.0)
    times = m._engine.kernel_times()
    m._engine.set_profiling(False)
    assert "k_sf_renorm" in times
    assert "k_sf_bary" not in times and "k_sf_sparsify" not in times


def test_fused_estimation_still_refuses_sparsity(tmp_path):
    import pyfasst_amd.audioModel as am
    g = load('sf_sparse')
    m = _fixture_model(g, tmp_path)
    before = _params(m)
    with pytest.raises(NotImplementedError, match="sparsity") as e:
        am.multiChanSourceF0Filter.estim_param_a_post_model(m)
    assert "reweigh_sparsity_constraint" in str(e.value) and "sf_run_sparse" in str(e.value)
    for a, b in zip(before, _params(m)):
        np.testing.assert_array_equal(a, b)
