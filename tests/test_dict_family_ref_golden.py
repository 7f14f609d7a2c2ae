"""The NumPy restatement tests/dict_family_ref.py against the reference's own
numbers (tests/golden/dict_family.npz, written by make_golden_dict_family.py),
and the float64 deviation its device bounds are built on.  CPU only.

The restatement repeats the reference's float64 operations in NumPy, so it is
held to the golden file bit for bit.  generate_WF0_MinQT_chirped does not run
in the reference translation the golden scripts use (`minqt_ran` == 0: a float
window length reaches np.ones); it is pinned by the restatement alone.
"""
import os

import numpy as np
import pytest

import dict_family_ref as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict_family.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(D.ODGD_CASES))
def test_odgd_bit_equal(g, name):
    odgd, spec = D.run_odgd_case(name)
    assert same(odgd, g['odgd_%s_odgd' % name])
    assert same(spec, g['odgd_%s_spec' % name])


@pytest.mark.parametrize("name", sorted(D.CHIRP_CASES))
def test_chirp_bit_equal(g, name):
    odgd, spec = D.run_chirp_case(name)
    assert same(odgd, g['chirp_%s_odgd' % name])
    assert same(spec, g['chirp_%s_spec' % name])


@pytest.mark.parametrize("name", sorted(D.WF0_CASES))
def test_wf0_chirped_bit_equal(g, name):
    F0Table, WF0 = D.generate_WF0_chirped(**D.WF0_CASES[name])
    assert same(F0Table, g['wf0_%s_F0Table' % name])
    assert same(WF0, g['wf0_%s_WF0' % name])


def test_cases_cover_what_they_claim(g):
    kw = D.ODGD_CASES
    n = {k: int(np.floor((v[1]['Fs'] / 2) / v[1]['F0'])) for k, v in kw.items()}
    assert n['one_partial'] == 1 and n['zero_partials'] == 0 and n['many_partials'] == 565
    assert not np.any(g['odgd_zero_partials_odgd']) and not np.any(g['odgd_zero_partials_spec'])
    assert g['odgd_zero_partials_odgd'].shape == (129,)
    shapes = {(v[1]['lengthOdgd'], v[1]['Nfft']) for v in kw.values()}
    assert {(129, 64), (129, 256), (128, 128), (300, 8192), (129, 2)} <= shapes
    assert {v[1]['t0'] for v in kw.values()} == {0.0, 0.37}
    c = D.CHIRP_CASES
    assert c['up']['F1'] < c['up']['F2'] and c['down_t0']['F1'] > c['down_t0']['F2']
    assert c['flat']['F1'] == c['flat']['F2']
    assert g['wf0_mixed_WF0'].shape == (256, 21) and g['wf0_single_WF0'].shape == (256, 1)
    # the two windows do differ on the comb columns, and only there
    d = g['wf0_mixed_WF0'] != g['wf0_sinebell_WF0']
    assert np.all(np.any(d[:, ::3], axis=0)) and not np.any(d[:, 1::3]) and not np.any(d[:, 2::3])


def test_inharmonicity_is_ignored():
    _, kw = D.ODGD_CASES['inharmo']
    a = D.generate_ODGD_spec_inharmo(**kw)
    b = D.generate_ODGD_spec_inharmo(**dict(kw, inharmonicity=0.9))
    assert same(a[0], b[0]) and same(a[1], b[1])
    with pytest.raises(ValueError):
        D.generate_ODGD_spec_inharmo(**dict(kw, analysisWindowType=np.ones(kw['lengthOdgd'])))


def test_window_names():
    with pytest.raises(ValueError):
        D.generate_ODGD_spec(220., 8000., lengthOdgd=64, Nfft=64, analysisWindowType='hann')
    with pytest.raises(ValueError):
        D.generate_ODGD_spec_chirped(210., 230., 8000., lengthOdgd=64, Nfft=64,
                                     analysisWindowType='blackman')
    D.generate_ODGD_spec_chirped(210., 230., 8000., lengthOdgd=64, Nfft=64,
                                 analysisWindowType='hann')


def test_flat_chirp_is_the_comb():
    """F1 == F2: the chirp's phase expression rounds differently from the
    comb's, within the waveform bound."""
    kw = D.CHIRP_CASES['flat']
    oc, sc = D.generate_ODGD_spec_chirped(**kw)
    ckw = {k: v for k, v in kw.items() if k not in ('F1', 'F2')}
    o, s = D.generate_ODGD_spec(kw['F1'], **ckw)
    assert D.colrel(oc, o) < D.WAVEFORM_BOUND and D.colrel(sc, s) < D.SPECTRUM_BOUND


def test_bounds_are_ten_times_the_measured_float64_deviation():
    """the float64 restatement against its own
    np.longdouble evaluation over the test shapes; the named constants are
    that measurement (rounded up), the bounds ten times it."""
    assert D.WAVEFORM_BOUND == 10 * D.MEASURED_WAVEFORM_DEVIATION
    assert D.SPECTRUM_BOUND == 10 * D.MEASURED_SPECTRUM_DEVIATION
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        return   # np.longdouble is float64 on this platform: nothing to measure against
    dev_w, dev_s = D.float64_deviation()
    print("waveform %.4e  spectrum %.4e" % (dev_w, dev_s))
    assert D.MEASURED_WAVEFORM_DEVIATION / 1.5 < dev_w <= D.MEASURED_WAVEFORM_DEVIATION
    assert D.MEASURED_SPECTRUM_DEVIATION / 1.5 < dev_s <= D.MEASURED_SPECTRUM_DEVIATION


def test_golden_within_the_bounds_of_the_yardstick(g):
    """The reference's own float64 numbers sit inside the bounds too."""
    for name, (_, kw) in sorted(D.ODGD_CASES.items()):
        re, im = D.odgd_longdouble(kw['F0'], kw['F0'], kw['Fs'], kw['lengthOdgd'], kw['Ot'],
                                   kw['t0'], False)
        z = np.asarray(re, dtype=np.float64) + 1j * np.asarray(im, dtype=np.float64)
        assert D.colrel(g['odgd_%s_odgd' % name], z) < D.WAVEFORM_BOUND, name
