"""CPU measurement behind the tolerances of tests/test_gpu_cqt_cells.py
(CQT cells section): the largest relative move, max|d out| / max|out|,
of the NumPy restatements' outputs under a 1e-15 relative perturbation of the
input signal, over 5 draws -- for the perfRast=1 cases of tests/golden/cqt.npz
(whose 1e-10 bound tests/test_gpu_cqt.py applies) and for the perfRast=0 cases
of tests/cqt_cells_ref.py.

    python tools/cqt_cells_sensitivity.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cqt_cells_ref as C  # noqa: E402
import cqt_ref  # noqa: E402
from helpers import CQT_CASES, load, rel  # noqa: E402


def moves(fn, x, draws=5):
    base = fn(x)
    worst = [0.0] * len(base)
    for s in range(draws):
        rs = np.random.RandomState(100 + s)
        out = fn(x * (1.0 + 1e-15 * rs.randn(x.size)))
        worst = [max(w, rel(o, b)) for w, o, b in zip(worst, out, base)]
    return worst


def main():
    warnings.simplefilter('ignore')
    x = load("cqt")['x']
    for name, kind, kw in CQT_CASES:
        o = cqt_ref.RefCQT(kind, **kw)

        def fn(v):
            sp = o.forward(v)
            return [sp, o.inverse(sp)]
        print("perfRast=1 %-6s forward %.2e inverse %.2e" % ((name,) + tuple(moves(fn, x))))
    for name in sorted(C.CASES):
        kind, kw, _ = C.CASES[name]
        o = C.RefCells(kind, **kw)

        def fn(v):
            cells = o.forward(v)
            sp = o.cells_to_sp(cells)
            packed = np.concatenate([cells[k].ravel() for k in sorted(cells, key=str)])
            return [packed, sp, o.inverse(cells)]
        print("perfRast=0 %-6s cells %.2e raster %.2e inverse %.2e" %
              ((name,) + tuple(moves(fn, C.signal(name)))))


if __name__ == "__main__":
    main()
