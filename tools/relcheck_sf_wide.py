"""tools/relcheck_sf.py's measurement for the wide-dictionary cases (DESIGN.md
7.2): how far the CPU restatement moves its final parameters when Cx is
perturbed by 1e-15 relative, 5 draws, on the fixture sf_wide and on the live
Kb = 257 models of tests/test_gpu_sf_wide.py.  CPU only:
python tools/relcheck_sf_wide.py"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ('', 'tests', 'oracle'):
    sys.path.insert(0, os.path.join(ROOT, d))
from helpers import load
from relcheck_sf import sensitivity
import sf_sparsity_ref as SP
import sf_wide_ref as W


def live(Kb, omega):
    """The restatement side of W.wide_pair, without the product."""
    import numpy as np
    import fasst_ref as R
    from pyfasst_amd import synthetic
    from sf_ref import _ref_class, two_factor
    X = synthetic.stereo_mixture(W.F, W.T, J=3, K_true=4, rank=1, seed=0)
    o = _ref_class()(iter_num=3, nmfUpdateCoeff=omega)
    o.set_transform([X[0], X[1]])
    np.random.seed(1)
    R.init_nmf_inst(o, 3, 4, 1)
    two_factor(o, W.wide_spec(Kb))
    return o


def tw_sensitivity(make, trials=5):
    """The same with the source activations perturbed instead of Cx: what a
    different summation order in the powers does, which a perturbation of Cx
    cannot show."""
    import numpy as np
    from helpers import rel
    from relcheck_sf import final
    base = final(make())
    worst = 0.0
    for s in range(trials):
        o = make()
        rs = np.random.RandomState(s)
        for j in (0, 1):
            tw = o.spec_comps[j]['factor'][0]['TW']
            tw *= 1 + 1e-15 * rs.randn(*tw.shape)
        worst = max(worst, max(rel(a, b) for a, b in zip(final(o), base)))
    return worst


if __name__ == "__main__":
    g = load('sf_wide')
    print('sf_wide %.2e' % sensitivity(lambda: W.fixture_oracle(g)[0]))
    print('sf_wide, TW perturbed %.2e' % tw_sensitivity(lambda: W.fixture_oracle(g)[0]))
    print('live Kb=257, TW perturbed %.2e' % tw_sensitivity(lambda: live(257, 1.)))
    for omega in (1., 0.7):
        print('live Kb=257 omega=%g %.2e' % (omega, sensitivity(lambda: live(257, omega))))

    def sparse():   # relcheck_sf.final runs the sparsity schedule for such a model
        o = live(150, 1.)
        SP.set_sparsity(o, W.SPARSE_LENGTHS)
        return o
    print('live Kb=150 sparse %.2e' % sensitivity(sparse))
