"""How far the CPU restatement of stereo_NMF (tests/stereo_nmf_ref.py) moves
its four outputs when SXR / SXL are perturbed by 1e-15 relative, 5 draws per
golden case (the conditioning measurement behind the golden bounds of
tests/test_gpu_stereo_nmf.py; yardstick: nmf.npz's 1.40e-15,
DESIGN.md 7.3).  CPU only:  python tools/relcheck_stereo_nmf.py"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ('', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, d))
import numpy as np
from helpers import rel
import stereo_nmf_ref as S

YARDSTICK = 1.40e-15


def run(name, SXR, SXL, kw, seed):
    np.random.seed(seed)
    return S.stereo_NMF(SXR, SXL, **kw)[:4]


def sensitivity(name, trials=5):
    SXR, SXL, kw, seed = S.case_inputs(name)
    base = run(name, SXR, SXL, kw, seed)
    worst = dict.fromkeys(S.NAMES, 0.0)
    for s in range(trials):
        rs = np.random.RandomState(s)
        pR = SXR * (1 + 1e-15 * rs.randn(*SXR.shape))
        pL = SXL * (1 + 1e-15 * rs.randn(*SXL.shape))
        for n, a, b in zip(S.NAMES, run(name, pR, pL, kw, seed), base):
            worst[n] = max(worst[n], rel(a, b))
    return worst


if __name__ == "__main__":
    for name in sorted(S.CASES):
        w = sensitivity(name)
        m = max(w.values())
        print(name, ' '.join('%s %.2e' % (n, w[n]) for n in S.NAMES),
              '| max %.2e = %.2f x yardstick' % (m, m / YARDSTICK))
