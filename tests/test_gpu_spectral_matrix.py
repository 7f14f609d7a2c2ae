"""Every reachable template arm of the spectral update's contraction kernels
at every padded K, against the oracle (run on MI355X).

Which instantiations of k_multi_prep, k_fb_contract, k_fw_contract and
k_tw_contract a GEM iteration launches is decided on the host from the model's
structure (spectral_arms below restates it), and the arms are not one body
with another trip count: NKC sizes the accumulator tiles, BLK / LAM / TBQ /
DEN switch operand planes and terms in and out.  The 4 x 4 cases here take the
four multi-block structures through KP = 16 / 32 / 64 / 128;
test_every_reachable_arm_has_a_case (CPU) fails when the cases, with the
single-component ones named in ELSEWHERE, stop covering the set.

Every case prints its deviations ('spectral-matrix ...') before asserting.
"""
import numpy as np
import pytest

import test_gpu_parity as P
from helpers import rel
from test_gpu_parity import _c3_like, _spatial_groups, _split_spec, _time_blobs

F, T, J, ITERS = 33, 40, 2, 2

# one unaligned K per KP (12 -> 16, 24 -> 32, 40 -> 64, 100 -> 128) and its
# column blocks: source 0 in two components, source 1 in one (keys 0, 2 / 1)
SPLITS = {12: {0: [5, 7], 1: [12]}, 24: {0: [10, 14], 1: [24]},
          40: {0: [18, 22], 1: [40]}, 100: {0: [40, 60], 1: [100]}}
TIME_BLOBS = {0: (6, 'free', 'free'), 1: (4, 'free', 'free'), 2: (3, 'fixed', 'free')}

# structure -> what spectral_arms needs to know of it
STRUCTURES = {
    'multi_fw': dict(several=True, free_fw=True),
    'lambda_fw': dict(several=True, lam=True, free_fw=True),
    'time_blobs': dict(several=True, blobs=True, free_tb=True),
    'lambda_tb': dict(several=True, lam=True, blobs=True, free_tb=True),
    # one spectral component per source (spectral_update's own launches)
    'single': dict(),
    'single_fw': dict(free_fw=True),
}
CASES = [(K, what) for K in sorted(SPLITS)
         for what in ('multi_fw', 'lambda_fw', 'time_blobs', 'lambda_tb')]

# the single-component arms are pinned by older tests: (K, structure, test of
# test_gpu_parity.py that runs it)
ELSEWHERE = [
    (16, 'single', 'test_em_stft_domain_vs_oracle'),
    (32, 'single', 'test_em_stft_domain_vs_oracle'),
    (40, 'single', 'test_em_stft_domain_vs_oracle'),
    (100, 'single', 'test_em_stft_domain_vs_oracle'),
    (6, 'single_fw', 'test_em_end_to_end_vs_reference'),     # em_fw_free
    (32, 'single_fw', 'test_free_fw_vs_oracle'),
    (40, 'single_fw', 'test_free_fw_vs_oracle'),
    (100, 'single_fw', 'test_k_above_64_every_structure_vs_oracle'),   # free_fw
]


def spectral_arms(K, several=False, lam=False, blobs=False, free_tb=False, free_fw=False):
    """The instantiations of the four kernels one GEM iteration launches for
    sources of at most K NMF columns.  Restates pyfasst_amd/csrc/fasst_em.hip
    (configure_model, update_multi) and fasst_em_spectral.hip (the rest):
      configure_model   KP = K padded to 16 / 32 / 64 / 128, NKC = KP / 16;
      update_multi      BLK (the multi-block path, multi_spectral /
                        multi_step) when some source has several spectral
                        components, or lambdaCorr > 0, or a component has time
                        blobs; otherwise spectral_update launches for itself;
      spectral_update   k_fb_contract<NKC, kFPW> (no DEN), k_fw_contract<NKC>
                        when some FW is free; its TW contraction is
                        k_tw_contract_lds, not k_tw_contract;
      multi_step        k_multi_prep<NKC, LAM>, k_fb_contract<NKC, kFPW, DEN>,
                        k_fw_contract<NKC, BLK, LAM> when a FW of the step is
                        free, k_tw_contract<NKC, TPW, BLK, LAM>, and its TBQ
                        form when a TB of the step is free; LAM = lambdaCorr
                        > 0;
      tpw_for           TPW = 1 at NKC = 8, else kTPW.
    A change to those functions must be restated here, and the completeness
    test then says which arms lost their case."""
    KP = 16 if K <= 16 else (32 if K <= 32 else (64 if K <= 64 else 128))
    n = KP // 16
    tpw = "1" if n == 8 else "kTPW"
    lam, blk = int(bool(lam)), bool(several or lam or blobs)
    if not blk:
        arms = {"fb_contract<%d,kFPW,0>" % n}
        if free_fw:
            arms.add("fw_contract<%d,0,0>" % n)
        return arms
    arms = {"multi_prep<%d,%d>" % (n, lam), "fb_contract<%d,kFPW,1>" % n,
            "tw_contract<%d,%s,1,%d,0>" % (n, tpw, lam)}
    if free_fw:
        arms.add("fw_contract<%d,1,%d>" % (n, lam))
    if free_tb:
        arms.add("tw_contract<%d,%s,1,%d,1>" % (n, tpw, lam))
    return arms


def test_every_reachable_arm_has_a_case():
    """The cases name every reachable arm: per NKC two of k_multi_prep, two of
    k_fb_contract, three of k_fw_contract (LAM comes with BLK only) and four of
    k_tw_contract (always BLK)."""
    full = set()
    for n, tpw in ((1, "kTPW"), (2, "kTPW"), (4, "kTPW"), (8, "1")):
        full |= {"multi_prep<%d,%d>" % (n, l) for l in (0, 1)}
        full |= {"fb_contract<%d,kFPW,%d>" % (n, d) for d in (0, 1)}
        full |= {"fw_contract<%d,%d,%d>" % ((n,) + bl) for bl in ((0, 0), (1, 0), (1, 1))}
        full |= {"tw_contract<%d,%s,1,%d,%d>" % (n, tpw, l, q) for l in (0, 1) for q in (0, 1)}
    assert len(full) == 44
    assert len(CASES) == 16 and len(set(CASES)) == 16
    here = set()
    for K, what in CASES:
        here |= spectral_arms(K, **STRUCTURES[what])
    assert len(here) == 36 and here <= full
    other = set()
    for K, what, test in ELSEWHERE:
        assert callable(getattr(P, test)), test
        other |= spectral_arms(K, **STRUCTURES[what])
    assert other == full - here
    # the restated rule itself, at its edges
    assert spectral_arms(16, several=True) == {
        "multi_prep<1,0>", "fb_contract<1,kFPW,1>", "tw_contract<1,kTPW,1,0,0>"}
    assert spectral_arms(17, lam=True, free_fw=True) == {
        "multi_prep<2,1>", "fb_contract<2,kFPW,1>", "fw_contract<2,1,1>",
        "tw_contract<2,kTPW,1,1,0>"}
    assert spectral_arms(65, blobs=True, free_tb=True) == {
        "multi_prep<8,0>", "fb_contract<8,kFPW,1>", "tw_contract<8,1,1,0,0>",
        "tw_contract<8,1,1,0,1>"}
    assert spectral_arms(64, blobs=True) == {
        "multi_prep<4,0>", "fb_contract<4,kFPW,1>", "tw_contract<4,kTPW,1,0,0>"}
    assert spectral_arms(128) == {"fb_contract<8,kFPW,0>"}


def _build(K, what):
    """Product and oracle with the structure applied to both: FW free (dense,
    positive) on both components of source 0, or time blobs on every component
    (one TB fixed)."""
    m, o, X = _c3_like(F, T, J, K, 1, ITERS)
    tb = {}
    for mod in (m, o):
        _split_spec(mod, SPLITS[K])
        if STRUCTURES[what].get('lam'):
            mod.lambdaCorr = 0.3
        if STRUCTURES[what].get('free_fw'):
            for k in (0, 2):
                fac = mod.spec_comps[k]['factor'][0]
                n = fac['FW'].shape[0]
                fac['FW'] = fac['FW'] + 0.2 * np.abs(np.random.RandomState(80 + k).randn(n, n))
                fac['FW_frdm_prior'] = 'free'
        else:
            tb = TIME_BLOBS
            _time_blobs(mod, tb)
    return m, o, X, tb


@pytest.mark.gpu
@pytest.mark.parametrize("K,what", CASES, ids=["K%d-%s" % c for c in CASES])
def test_spectral_arm_vs_oracle(K, what):
    """The assertions and bounds of
    test_gpu_parity.test_k_above_64_every_structure_vs_oracle at each KP."""
    m, o, X, tb = _build(K, what)
    ll = m.estim_param_a_post_model()
    llo = o.estim_param_a_post_model()
    d = {'ll': rel(ll, llo)}
    for k in sorted(o.spec_comps):
        for key in ('FB', 'FW', 'TW', 'TB') if k in tb else ('FB', 'FW', 'TW'):
            d['%s%d' % (key, k)] = rel(m.spec_comps[k]['factor'][0][key],
                                      o.spec_comps[k]['factor'][0][key])
    for j in range(J):
        d['params%d' % j] = rel(m.spat_comps[j]['params'], o.spat_comps[j]['params'])
    groups = _spatial_groups(m)
    d['absS'] = rel(np.abs(m.separated_images(groups)), np.abs(o.separated_images(X, groups)))
    print("spectral-matrix K=%d %s [%s] %s" % (
        K, what, " ".join(sorted(spectral_arms(K, **STRUCTURES[what]))),
        " ".join("%s=%.3g" % kv for kv in sorted(d.items()))))
    assert d.pop('ll') < 1e-10
    for name, v in sorted(d.items()):
        assert v < 1e-8, (name, v)
