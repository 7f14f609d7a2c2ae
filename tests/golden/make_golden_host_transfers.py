"""Write tests/golden/host_transfers.npz: the outputs of the transfer-heavy
stateless calls (tests/host_transfer_cases.py) on an MI355X.

Run once on the commit before the host transfers moved onto DBuf's typed
upload / put / get, so the file records what the hand-written copies gave:

    python tests/golden/make_golden_host_transfers.py [out.npz]
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

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "host_transfers.npz")
    res = cases.run_cases(_lib)
    np.savez(out, **res)
    print("wrote %s: %d arrays" % (out, len(res)))
