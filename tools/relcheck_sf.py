"""How far the CPU restatement moves its final parameters when Cx is perturbed
by 1e-15 relative (the conditioning measurement of DESIGN.md 3.5, as
tools/relcheck.py's figures), on em_conv, on the two-factor fixtures
sf_inst / sf_conv and on sf_sparse (sf_inst with the sparsity schedule on,
tests/sf_sparsity_ref.py).  CPU only:  python tools/relcheck_sf.py"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ('', 'tests', 'oracle'):
    sys.path.insert(0, os.path.join(ROOT, d))
import numpy as np
from helpers import load, rel, oracle_model_from_golden
import sf_sparsity_ref as SP
from sf_ref import PARTS, SF_FIXTURES, fixture_oracle


def final(o):
    if any(c.get('sparsity') for c in o.spec_comps.values()):
        SP.estim_param_a_post_model(o)
    else:
        o.estim_param_a_post_model()
    out = [np.array(sc['params']) for sc in o.spat_comps.values()]
    for c in o.spec_comps.values():
        for f in c['factor'].values():
            out += [np.array(f[p]) for p in PARTS]
    return out


def sensitivity(make, trials=5):
    base = final(make())
    worst = 0.0
    for s in range(trials):
        o = make()
        rs = np.random.RandomState(s)
        o.Cx = o.Cx * (1 + 1e-15 * rs.randn(*o.Cx.shape))
        worst = max(worst, max(rel(a, b) for a, b in zip(final(o), base)))
    return worst


if __name__ == "__main__":
    g = load('em_conv')
    print('em_conv %.2e' % sensitivity(lambda: oracle_model_from_golden(g, 'em_conv')[0]))
    for case in sorted(SF_FIXTURES):
        gg = load(case)
        print(case, '%.2e' % sensitivity(lambda: fixture_oracle(gg, case)[0]))
    gs = load('sf_sparse')

    def sparse():
        o = fixture_oracle(gs, SP.SPARSE_CASE)[0]
        SP.set_sparsity(o, [int(L) for L in gs['sparsity']])
        return o
    print('sf_sparse %.2e' % sensitivity(sparse))
