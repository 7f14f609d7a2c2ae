"""Wide fixed F0 dictionaries on the two-factor path (test infrastructure
only): the reference-run fixture tests/golden/sf_wide.npz
(tests/golden/make_golden_sf_wide.py) loaded into the restatement and into the
product, hand-set wide models on both sides, and the parity bounds.

Bounds (measured by tools/relcheck_sf_wide.py on the CPU): the
largest relative move of the restatement's final parameters under a 1e-15
relative perturbation of Cx, 5 draws, scaled from em_conv (2.2e-13 <-> 1e-9),
never below TIGHT = 1e-9:

    sf_wide (Kb = 146, 3 iterations)         4.2e-15  -> TIGHT
      (the source activations perturbed instead: 2.7e-15)
    live Kb = 257, omega 1   (3 iterations)  7.5e-15  -> TIGHT
    live Kb = 257, omega 0.7 (3 iterations)  1.1e-14  -> TIGHT
    live Kb = 150, sparsity schedule (2)     1.2e-14  -> TIGHT

The logliks keep 1e-10."""
import json
import os

import numpy as np

from sf_ref import PARTS, _ref_class, pair

TIGHT = 1e-9
LL_TOL = 1e-10
WIDE_TOL = {'sf_wide': TIGHT, 'live': TIGHT}
SPARSE_LENGTHS = [3, 2, False]   # the sparsity case (Kb = 150): median lengths per component
FIX, FREE = 'fixed', 'free'
F, T = 129, 90


def _load_state(mod, g):
    """The fixture's initial state into a model of either side; an array the
    reference holds in several factors (the F0 dictionary, its weights, the
    filter basis) is ONE array here too: the renormalisation rescales it in
    place once per holder."""
    J = 0
    while 'init_params_%d' % J in g:
        J += 1
    for j in range(J):
        mod.spat_comps[j] = {'time_dep': 'indep', 'mix_type': 'inst', 'frdm_prior': 'free',
                             'params': np.array(g['init_params_%d' % j])}
        mod.spec_comps[j] = {'spat_comp_ind': j, 'factor': {}, 'sparsity': False}
        i = 0
        while 'priors_%d_%d' % (j, i) in g:
            pri = [str(p) for p in g['priors_%d_%d' % (j, i)]]
            fac = {'TB': [], 'FB_frdm_prior': pri[0], 'FW_frdm_prior': pri[1],
                   'TW_frdm_prior': pri[2], 'TB_frdm_prior': [], 'TW_constr': 'NMF'}
            for part in PARTS:
                k0, i0 = (int(v) for v in str(g['alias_%s_%d_%d' % (part, j, i)]).split('_'))
                if (k0, i0) != (j, i):
                    fac[part] = mod.spec_comps[k0]['factor'][i0][part]
                else:
                    fac[part] = np.array(g['init_%s_%d_%d' % (part, j, i)])
            mod.spec_comps[j]['factor'][i] = fac
            i += 1
    return J


def fixture_oracle(g):
    """The restatement on the fixture's WAV.  Returns (model, channel STFTs)."""
    import fasst_ref as R
    kw = json.loads(str(g['ctor']))
    x, _ = R.read_scaled(g['wav'])
    w = np.hanning(kw['wlen'])
    X = [R.stft(x[:, c], w, kw['hopsize'], kw['wlen']) for c in range(2)]
    o = _ref_class()(iter_num=kw['iter_num'])
    o.set_transform(X)
    _load_state(o, g)
    return o, X


def fixture_product(g, tmp_path, **extra):
    """multiChanSourceF0Filter built on the fixture's WAV by its constructor
    (`extra`: wideDictionary), then given the fixture's initial state, so that
    the comparison does not rest on the F0 dictionary built on the device."""
    import scipy.io.wavfile as wf
    import pyfasst_amd.audioModel as am
    kw = json.loads(str(g['ctor']))
    wav = os.path.join(str(tmp_path), "sf_wide.wav")
    wf.write(wav, int(g['fs']), g['wav'])
    np.random.seed(0)
    m = am.multiChanSourceF0Filter(wav, **dict(kw, **extra))
    built = m.spec_comps[0]['factor'][0]['FB']
    _load_state(m, g)
    return m, built


def final_state(mod):
    out = [np.array(sc['params']) for sc in mod.spat_comps.values()]
    for c in mod.spec_comps.values():
        for f in c['factor'].values():
            out += [np.array(f[p]) for p in PARTS]
    return out


def compare_fixture(mod, g, ll, ll_tol, tol, cmp=None):
    """Final state against the fixture (cmp = None: equality)."""
    from helpers import rel

    def close(a, b, what):
        assert np.shape(a) == np.shape(b), what
        if cmp is None:
            np.testing.assert_array_equal(a, b, err_msg=str(what))
        else:
            assert rel(a, b) < tol, (what, rel(a, b))
    if cmp is None:
        np.testing.assert_array_equal(ll, g['logliks'])
    else:
        assert rel(ll, g['logliks']) < ll_tol, rel(ll, g['logliks'])
    for j in range(len(mod.spat_comps)):
        close(mod.spat_comps[j]['params'], g['final_params_%d' % j], j)
        for i, fac in mod.spec_comps[j]['factor'].items():
            for part in PARTS:
                key = 'final_%s_%s' % (part, str(g['alias_%s_%d_%d' % (part, j, i)]))
                close(fac[part], g[key], (j, i, part))


def wide_spec(Kb, comps=(0, 1)):
    """Source factor Kb wide (fixed FB, FW = I fixed, TW free) times a filter
    factor FB 129 x 6 fixed, FW 6 x 3 free, TW free."""
    return {k: [(Kb, Kb, (FIX, FIX, FREE), True), (6, 3, (FIX, FREE, FREE))] for k in comps}


def wide_pair(Kb, iters=3, omega=1., spec=None, setup=None, share=False, T=T):
    """(product, restatement, X) with hand-set dictionaries, the product's
    switch on.  share: component 1's source factor holds component 0's FB and
    FW arrays (the class's default structure)."""
    def prepare(mod):
        if share:
            f0, f1 = mod.spec_comps[0]['factor'][0], mod.spec_comps[1]['factor'][0]
            f1['FB'], f1['FW'] = f0['FB'], f0['FW']
        if setup is not None:
            setup(mod)
    m, o, X = pair(F, T, 3, 4, 1, iters, False, spec or wide_spec(Kb), omega=omega, setup=prepare)
    m.wideDictionary = True
    return m, o, X
