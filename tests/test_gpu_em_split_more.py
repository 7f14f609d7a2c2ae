"""What tests/test_gpu_em_split.py's ten models do not reach of the mixing,
renormalisation and spectral units (fasst_em_mix.hip, fasst_em_renorm.hip,
fasst_em_spectral.hip), bit for bit against tests/golden/em_split_more.npz,
written by make_golden_em_split.py --more on the library that still held
those phases in fasst_em.hip:

  k, l  GEM runs through k_mix's two wide arms (k_mix<11, 4>: more than four
        statistics per lane; k_mix<11, 16>: R > 16 and the LDS ceiling
        mix_lds_limits raises);
  m     the stand-alone ABI sequence renormalize(), spectral_update(hat_W),
        renormalize(): launch_renorm(c, 0), launch_spectral_prep without the
        fork, launch_w_old and k_rho_from_hatw from the C ABI;
  launch counts: a run of every GEM case a - l with the per-kernel timing on
        records the same number of event pairs per kernel slot as the fixture,
        and leaves the parameters of the unprofiled run bit for bit (a launch
        that lost its timing pair, or moved outside one, passes every numeric
        test).

The tolerance is 0 and the fixture belongs to the MI355X, as in
test_gpu_em_split.py."""
import os

import numpy as np
import pytest

import em_split_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(golden_dir):
    with np.load(os.path.join(golden_dir, "em_split_more.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def plain():
    """The unprofiled run of a GEM case, computed once."""
    runs = {}

    def get(name):
        if name not in runs:
            runs[name] = cases.run(name)
        return runs[name]
    return get


def check_equal(got, want, names):
    assert names and names == sorted(got)
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert not np.isnan(got[k]).any(), k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", ["k", "l"])
def test_em_bit_exact(want, plain, name):
    got = plain(name)
    assert got[name + "_done_mask"][0] == cases.N_ITER
    check_equal(got, want, sorted(k for k in want if k.startswith(name + "_") and k != name + "_launches"))


def test_abi_paths_bit_exact(want):
    check_equal(cases.run_abi("m"), want, sorted(k for k in want if k.startswith("m_")))


@pytest.mark.parametrize("name", sorted(set(cases.ALL_CASES) - {"m"}))
def test_launch_counts(want, plain, name):
    got = cases.run(name, profile=True)
    key = name + "_launches"
    print(name, got[key])
    assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key])
    ref = plain(name)
    check_equal({k: v for k, v in got.items() if k != key}, ref, sorted(ref))
