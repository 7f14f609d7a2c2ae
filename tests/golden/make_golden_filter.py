"""Generate tests/golden/filter_stft.npz by running the REFERENCE's
filter_stft and filter_conv_stft (tftransforms/stft.py:133-334; the scratch
py2->py3 translation built by oracle/make_scratch_ref.py, as
tests/golden/make_golden_spatial.py does):

    python tests/golden/make_golden_filter.py            # all cases
    python tests/golden/make_golden_filter.py base_m2

Each case runs in a fresh interpreter and leaves /tmp/golden_filter_<case>.npy;
the parent collects them into the one fixture file.  The cases, their seeds
and the calls that draw `data`, `W` and the windows from RandomState(seed) are
tests/filter_stft_ref.py's CASES / seed_of / draw, which the tests call again:
the fixture holds the parameters, the seeds and the reference's outputs only.

The scratch recipe already turns most float sizes and indices of the two
functions into ints.  What it leaves is np.zeros called with float sizes
(stft.py:166, 177, 178, 279, 290, 291: newLengthData is a float), which
NumPy < 1.12 truncated and NumPy today refuses.  The maker therefore gives
the scratch stft module, and that module only, a stand-in for its `np` name
whose `zeros` truncates float sizes to int and which passes everything else
through to NumPy (`_NpTruncZeros` below).  That shim is this file's own code;
nothing under oracle/ changes.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
MAX_BYTES = 900 * 1024


class _NpTruncZeros(object):
    """`np` as NumPy < 1.12 behaved for the sizes of np.zeros."""

    def __init__(self, np):
        self._np = np

    def __getattr__(self, name):
        return getattr(self._np, name)

    def zeros(self, shape, *a, **kw):
        np = self._np
        if np.ndim(shape) == 0:
            shape = int(shape)                       # a negative size still raises
        else:
            shape = [int(s) for s in shape]
        return np.zeros(shape, *a, **kw)


def tmp_of(name):
    return "/tmp/golden_filter_%s.npy" % name


def run_case(name):
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, SCRATCH)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import filter_stft_ref as FR
    import pyfasst.tftransforms.stft as ref
    ref.np = _NpTruncZeros(np)
    y = FR.run_ref(name, mod=ref)
    print(name, FR.CASES[name], y.shape)
    np.save(tmp_of(name), y)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        run_case(sys.argv[2])
        sys.exit(0)
    import numpy as np
    import make_scratch_ref
    import filter_stft_ref as FR
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    out = {}
    if os.path.exists(FR.GOLDEN) and sys.argv[1:]:
        out = dict(np.load(FR.GOLDEN))
    for name in sys.argv[1:] or list(FR.CASES):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name])
        out['y_' + name] = np.load(tmp_of(name))
        out['case_' + name] = np.array(json.dumps(dict(FR.CASES[name], seed=FR.seed_of(name))))
    np.savez_compressed(FR.GOLDEN, **out)
    size = os.path.getsize(FR.GOLDEN)
    print(FR.GOLDEN, size)
    if size > MAX_BYTES:
        raise SystemExit("fixture file of %d bytes passes %d" % (size, MAX_BYTES))
