"""Write tests/golden/separation_tail.npz: what the separation calls of
tests/separation_tail_cases.py give on an MI355X, and the statuses of their
refusals.

Run on the commit before the calls shared one image producer per model and one
iSTFT sink, so the file records what the hand-copied tails computed:

    python tests/golden/make_golden_separation_tail.py [out.npz]

Every case runs twice.  These kernels use no atomics, so every output is
expected to be bit-equal between the runs; one that is not is named and the
script fails rather than leave it out.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pyfasst_amd import _lib  # noqa: E402
import separation_tail_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "separation_tail.npz")
    a, b = cases.run_cases(_lib), cases.run_cases(_lib)
    assert sorted(a) == sorted(b)
    bad = sorted(k for k in a if not np.array_equal(a[k], b[k]))
    for k in sorted(a):
        if k.startswith("refuse_"):
            print("%s: status %d" % (k, a[k][0]))
    if bad:
        sys.exit("not bit-equal between two runs: %s" % bad)
    np.savez_compressed(out, **a)
    print("wrote %s: %d arrays, all bit-repeatable, %d bytes" % (out, len(a), os.path.getsize(out)))
