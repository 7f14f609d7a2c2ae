"""The GEM iteration gives, bit for bit, what it gave while the whole EM engine
was one translation unit (tests/golden/em_split.npz, written by
make_golden_em_split.py on that library): FB, FW, TW, the mixing parameters
and the per-iteration log-likelihoods of ten models, one per launch path of
the E-step, mixing, spectral and renormalisation phases
(tests/em_split_cases.py), whichever unit (fasst_em_estep.hip,
fasst_em_mix.hip, fasst_em_spectral.hip, fasst_em_renorm.hip) a phase lives
in.  The kernels are the same machine code, so the tolerance is 0: any difference is a launch shape, an argument, a stream or
event order, or an LDS ceiling that did not survive the move.

The fixture depends on the device's CU count through configure_model's
schedules (block counts, chunking): it was generated on an MI355X and is
checked on the same machine type; there is no tolerance fallback."""
import os

import numpy as np
import pytest

import em_split_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(golden_dir):
    with np.load(os.path.join(golden_dir, "em_split.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_em_bit_exact(want, name):
    got = cases.run(name)
    names = sorted(k for k in want if k.startswith(name + "_"))
    assert names and names == sorted(got)
    assert got[name + "_done_mask"][0] == cases.N_ITER
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert not np.isnan(got[k]).any(), k
        assert np.array_equal(got[k], want[k]), k
