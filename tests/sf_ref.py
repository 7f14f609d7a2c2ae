"""Two-factor (source / filter) test models (test infrastructure only).

`two_factor(m, spec)` replaces spectral components of a model -- the product's
or the restatement's (oracle/fasst_ref.py), which share the reference's dict
layout -- by hand-built components of one or two factors with seeded positive
random matrices, identically on both sides.  `pair()` builds the product and
the restatement on the same STFT-domain mixture."""
import numpy as np

PARTS = ('FB', 'FW', 'TW')
EPS = 1e-10


def _ref_class():
    import fasst_ref as R

    class RefFASSTsf(R.RefFASST):
        """oracle/fasst_ref.py with renormalize_parameters corrected on the
        point where it departs from the reference for several factors
        (audioModel.py:2003-2036): the reference REUSES `global_energy`.  It
        enters a component as the spatial energy, multiplies factor 0's FB,
        and is then overwritten by mean(TW) of each factor in turn, so the FB
        of factor i > 0 is multiplied by the mean that factor i - 1's TW was
        just divided by (the energy handed down the chain), not by the spatial
        energy again.  The restatement multiplies every factor by the spatial
        energy; with one factor the two agree.  tests/golden/sf_*.npz (runs of
        the reference) pin this version (tests/test_sf_ref_golden.py)."""

        def renormalize_parameters(self, rng=np.random):
            energy = np.zeros(len(self.spat_comps))
            for j, sc in self.spat_comps.items():
                energy[j] = np.mean(np.abs(sc['params']) ** 2)
                sc['params'] /= np.sqrt(energy[j])
            self.restarted = []
            for k, comp in self.spec_comps.items():
                ge = energy[comp['spat_comp_ind']]
                nfac = len(comp['factor'])
                for fi, fac in comp['factor'].items():
                    ge = renorm_factor(fac, ge, fi < nfac - 1, rng,
                                       lambda: self.restarted.append((k, fi)))
    return RefFASSTsf


def renorm_factor(fac, ge, divide, rng=np.random, on_restart=None):
    """One factor's renormalisation (audioModel.py:2006-2036, no time blobs);
    returns mean(TW), the `global_energy` the next factor receives."""
    fac['FB'] *= ge
    w = fac['FB'].max(axis=0)
    w[w == 0] = 1.
    fac['FB'] /= w
    fac['FW'] *= np.vstack(w)
    w = fac['FW'].mean(axis=0)
    w[w == 0] = 1.
    fac['FW'] /= w
    fac['TW'] *= np.vstack(w)
    if np.sum(fac['TW']) < EPS:
        fac['TW'] = rng.randn(*fac['TW'].shape) ** 2
        fac['TW'] *= 1e3 * EPS
        if on_restart is not None:
            on_restart()
    ge = fac['TW'].mean()
    if divide:
        fac['TW'] /= ge
    return ge


def class_ref(m, seed, src, srcw, filt):
    """multiChanSourceF0Filter._initialize_structures (audioModel.py:2650-2772)
    restated on the oracle's model, from the product's dictionaries: the
    source basis and its weights are one array in every component."""
    o = _ref_class()(iter_num=m.iter_num)
    o.nbFreqsSigRepr, o.nbFramesSigRepr = m.nbFreqsSigRepr, m.nbFramesSigRepr
    T = o.nbFramesSigRepr
    np.random.seed(seed)
    nb = m.nbComps

    def fac(FB, FW, TW, fb, fw):
        return {'FB': FB, 'FW': FW, 'TW': TW, 'TB': [], 'FB_frdm_prior': fb, 'FW_frdm_prior': fw,
                'TW_frdm_prior': 'free', 'TB_frdm_prior': [], 'TW_constr': 'NMF'}
    for j in range(nb - 1):
        r = m.rank[j]
        np.random.randn(2, r)
        p = np.array([np.sin((j + 1) * np.pi / (2. * nb)) + np.random.randn(r) * np.sqrt(0.01),
                      np.cos((j + 1) * np.pi / (2. * nb)) + np.random.randn(r) * np.sqrt(0.01)])
        o.spat_comps[j] = {'time_dep': 'indep', 'mix_type': 'inst', 'frdm_prior': 'free',
                           'params': p}
        TW0 = 0.75 * np.abs(np.random.randn(src.shape[1], T)) + 0.25
        FW1 = 0.75 * np.abs(np.random.randn(m.nbFilterComps, m.nbFilterWeigs[j])) + 0.25
        TW1 = 0.75 * np.abs(np.random.randn(m.nbFilterWeigs[j], T)) + 0.25
        o.spec_comps[j] = {'spat_comp_ind': j, 'factor': {
            0: fac(src, srcw, TW0, 'fixed', 'fixed'), 1: fac(filt, FW1, TW1, 'fixed', 'free')}}
    j = nb - 1
    o.spat_comps[j] = {'time_dep': 'indep', 'mix_type': 'inst', 'frdm_prior': 'free',
                       'params': np.random.randn(2, m.rank[-1])}
    FB = 0.75 * np.abs(np.random.randn(o.nbFreqsSigRepr, m.nbNMFResComps)) + 0.25
    TW = 0.75 * np.abs(np.random.randn(m.nbNMFResComps, T)) + 0.25
    o.spec_comps[j] = {'spat_comp_ind': j, 'factor': {
        0: fac(FB, np.eye(m.nbNMFResComps), TW, 'free', 'fixed')}}
    o.renormalize_parameters()
    return o


def _factor(rs, F, T, Kb, Kw, pri, eye=False):
    FW = np.eye(Kb) if eye else 0.75 * np.abs(rs.randn(Kb, Kw)) + 0.25
    return {'FB': 0.75 * np.abs(rs.randn(F, Kb)) + 0.25, 'FW': FW,
            'TW': 0.75 * np.abs(rs.randn(FW.shape[1], T)) + 0.25, 'TB': [],
            'FB_frdm_prior': pri[0], 'FW_frdm_prior': pri[1], 'TW_frdm_prior': pri[2],
            'TB_frdm_prior': [], 'TW_constr': 'NMF'}


def two_factor(m, spec, seed=7):
    """spec: {key: [(Kb, Kw, (FB, FW, TW priors)[, eye]), ...]}: the factors
    of spectral component `key` (its spatial component is kept)."""
    F, T = m.nbFreqsSigRepr, m.nbFramesSigRepr
    for k in sorted(spec):
        rs = np.random.RandomState(seed + 31 * k)
        m.spec_comps[k]['factor'] = {
            i: _factor(rs, F, T, f[0], f[1], f[2], len(f) > 3 and f[3])
            for i, f in enumerate(spec[k])}


def pair(F, T, J, K, rank, iters, conv, spec, seed=0, omega=1., setup=None):
    """(product model, restatement) with identical parameters."""
    import fasst_ref as R
    import pyfasst_amd.audioModel as am
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    rk = np.atleast_1d(rank)
    X = synthetic.stereo_mixture(F, T, J=J, K_true=4, rank=int(rk[0]), seed=seed)
    np.random.seed(1)
    m = am.MultiChanNMFInst_FASST(SpectralAudio(X=X), nbComps=J, nbNMFComps=K, spatial_rank=rank,
                                  iter_num=iters, wlen=2 * (F - 1), hopsize=(F - 1) // 2,
                                  nmfUpdateCoeff=omega)
    o = _ref_class()(iter_num=iters, nmfUpdateCoeff=omega)
    o.set_transform([X[0], X[1]])
    np.random.seed(1)
    R.init_nmf_inst(o, J, K, rank)
    if conv:
        am.MultiChanNMFConv.makeItConvolutive(m)
        R.make_convolutive(o)
    for mod in (m, o):
        two_factor(mod, spec)
        if setup is not None:
            setup(mod)
    return m, o, X


def compare(m, o, ll, llo, ll_tol, tol):
    from helpers import rel
    assert rel(ll, llo) < ll_tol, rel(ll, llo)
    for j in range(len(m.spat_comps)):
        assert rel(m.spat_comps[j]['params'], o.spat_comps[j]['params']) < tol, j
    for k in sorted(m.spec_comps):
        assert sorted(m.spec_comps[k]['factor']) == sorted(o.spec_comps[k]['factor'])
        for i in m.spec_comps[k]['factor']:
            fm, fo = m.spec_comps[k]['factor'][i], o.spec_comps[k]['factor'][i]
            for part in PARTS:
                assert np.shape(fm[part]) == np.shape(fo[part]), (k, i, part)
                assert rel(fm[part], fo[part]) < tol, (k, i, part, rel(fm[part], fo[part]))


# ---- reference-run fixtures tests/golden/sf_<case>.npz (make_golden_sf.py) ----
_FIX, _FREE = 'fixed', 'free'
SF_CFG = dict(nbComps=3, nbNMFComps=4, n=4000, fs=8000)
SF_FIXTURES = {
    # 'inst', rank 1: source factor FB 65 x 13 fixed, FW = I fixed, TW free;
    # filter factor FB 65 x 6 fixed, FW 6 x 3 free, TW 3 x T free
    'sf_inst': dict(conv=False, spatial_rank=1,
                    kw=dict(iter_num=4, wlen=128, hopsize=64),
                    spec={k: [(13, 13, (_FIX, _FIX, _FREE), True), (6, 3, (_FIX, _FREE, _FREE))]
                          for k in (0, 1)}),
    # 'conv' after makeItConvolutive(), rank 2: FB of the source factor free,
    # TW of the filter factor fixed, omega 0.7
    'sf_conv': dict(conv=True, spatial_rank=2,
                    kw=dict(iter_num=4, wlen=128, hopsize=64, nmfUpdateCoeff=0.7),
                    spec={k: [(13, 13, (_FREE, _FIX, _FREE), True), (6, 3, (_FIX, _FREE, _FIX))]
                          for k in (0, 1)}),
}


def fixture_oracle(g, case):
    """The restatement on the fixture's WAV (oracle STFT), loaded with the
    fixture's initial state.  Returns (model, channel STFTs)."""
    import fasst_ref as R
    cfg = SF_FIXTURES[case]
    kw = cfg['kw']
    x, _ = R.read_scaled(g['wav'])
    w = np.hanning(kw['wlen'])
    X = [R.stft(x[:, c], w, kw['hopsize'], kw['wlen']) for c in range(2)]
    o = _ref_class()(iter_num=kw['iter_num'], nmfUpdateCoeff=kw.get('nmfUpdateCoeff', 1.))
    o.set_transform(X)
    J = SF_CFG['nbComps']
    for j in range(J):
        o.spat_comps[j] = {'time_dep': 'indep', 'mix_type': 'conv' if cfg['conv'] else 'inst',
                           'frdm_prior': 'free', 'params': np.array(g['init_params_%d' % j])}
        o.spec_comps[j] = {'spat_comp_ind': j, 'factor': {}}
        i = 0
        while 'init_FB_%d_%d' % (j, i) in g:
            pri = [str(p) for p in g['priors_%d_%d' % (j, i)]]
            o.spec_comps[j]['factor'][i] = {
                'FB': np.array(g['init_FB_%d_%d' % (j, i)]), 'FW': np.array(g['init_FW_%d_%d' % (j, i)]),
                'TW': np.array(g['init_TW_%d_%d' % (j, i)]), 'TB': [], 'FB_frdm_prior': pri[0],
                'FW_frdm_prior': pri[1], 'TW_frdm_prior': pri[2], 'TB_frdm_prior': [],
                'TW_constr': 'NMF'}
            i += 1
    return o, X


def fixture_product(g, case, tmp_path):
    """The product model built as make_golden_sf.py builds the reference's."""
    import json
    import os
    import scipy.io.wavfile as wf
    import pyfasst_amd.audioModel as am
    cfg = SF_FIXTURES[case]
    ctor = json.loads(str(g['ctor']))
    wav = os.path.join(str(tmp_path), case + ".wav")
    wf.write(wav, int(g['fs']), g['wav'])
    np.random.seed(0)
    cls = am.MultiChanNMFConv if cfg['conv'] else am.MultiChanNMFInst_FASST
    m = cls(wav, nbComps=ctor['nbComps'], nbNMFComps=ctor['nbNMFComps'],
            spatial_rank=ctor['spatial_rank'], **ctor['kw'])
    if cfg['conv']:
        m.makeItConvolutive()
    two_factor(m, cfg['spec'])
    return m


def compare_fixture(m, g, ll, S, ll_tol, tol):
    """Final state of a model (product or restatement) against the fixture."""
    from helpers import rel
    assert rel(ll, g['logliks']) < ll_tol, rel(ll, g['logliks'])
    for j in range(len(m.spat_comps)):
        assert rel(m.spat_comps[j]['params'], g['final_params_%d' % j]) < tol, j
        for i, fac in m.spec_comps[j]['factor'].items():
            for part in PARTS:
                ref = g['final_%s_%d_%d' % (part, j, i)]
                assert np.shape(fac[part]) == ref.shape
                assert rel(fac[part], ref) < tol, (j, i, part, rel(fac[part], ref))
    assert S.shape == g['absS'].shape
    assert rel(np.abs(S), g['absS']) < tol, rel(np.abs(S), g['absS'])
