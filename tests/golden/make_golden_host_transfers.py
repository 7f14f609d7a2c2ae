"""Write tests/golden/host_transfers.npz: the outputs of the transfer-heavy
stateless calls (tests/host_transfer_cases.py) on an MI355X.

Run once on the commit before the host transfers moved onto DBuf's typed
upload / put / get, so the file records what the hand-written copies gave:

    python tests/golden/make_golden_host_transfers.py [out.npz]

host_transfers_compute.npz (beside it, or `compute` + a path) holds the compute
entry points converted later (run_compute_cases), from the commit before
that: every case runs twice and only outputs bit-equal between the two runs
are kept; the others are named on stdout.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pyfasst_amd import _lib  # noqa: E402
import host_transfer_cases as cases  # noqa: E402


def write_compute(out):
    a, b = cases.run_compute_cases(_lib), cases.run_compute_cases(_lib)
    keep = {k: a[k] for k in a if np.array_equal(a[k], b[k])}
    print("not bit-equal between two runs:", sorted(set(a) - set(keep)) or "none")
    np.savez(out, **keep)
    print("wrote %s: %d arrays" % (out, len(keep)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["compute"]:
        write_compute(sys.argv[2] if len(sys.argv) > 2
                      else os.path.join(HERE, "host_transfers_compute.npz"))
    else:
        out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "host_transfers.npz")
        res = cases.run_cases(_lib)
        np.savez(out, **res)
        print("wrote %s: %d arrays" % (out, len(res)))
