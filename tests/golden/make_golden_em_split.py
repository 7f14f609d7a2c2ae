"""Write tests/golden/em_split.npz: what the ten GEM runs of
tests/em_split_cases.py give on an MI355X.

Run once on the commit before the EM engine was split into one translation
unit per phase, so the file records what the single unit computed:

    python tests/golden/make_golden_em_split.py [out.npz]

Every case runs twice; a case whose two runs are not bit-equal cannot carry a
tolerance of 0 and is left out (named on stdout).  The results depend on the
device's CU count through configure_model's schedules: generate and check on
the same machine type.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import em_split_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "em_split.npz")
    keep = {}
    for name in cases.CASES:
        a, b = cases.run(name), cases.run(name)
        same = sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
        finite = all(np.isfinite(v).all() for v in a.values())
        print("case %s: %s, loglik %s, (done, mask) %s" % (
            name, "bit-repeatable" if same else "NOT bit-repeatable: left out",
            a["%s_loglik" % name], a["%s_done_mask" % name]), "" if finite else "NOT FINITE")
        if same:
            keep.update(a)
    np.savez_compressed(out, **keep)
    print("wrote %s: %d arrays, %d bytes" % (out, len(keep), os.path.getsize(out)))
