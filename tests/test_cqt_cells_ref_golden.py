"""tests/cqt_cells_ref.py (the NumPy restatement of the reference CQT / MinQT
with perfRast=0) against the reference's own outputs, tests/golden/cqt_cells.npz.

What only moves data (the scatter, the drop, the fold back into cells) is
bit-equal given equal inputs; the numeric chain (FFT, kernel product,
filtfilt) is the same NumPy / SciPy code as the reference's and is held to the
bound oracle/cqt_ref.py keeps against its own fixtures (1e-12 of the largest
magnitude).
"""
import numpy as np
import pytest
import scipy.interpolate as spinterp

import cqt_cells_ref as C
from helpers import load, rel

NUM = 1e-12


def _cells(g, name, oct_n, prefix='cell'):
    cells = {i: g['%s_%s%d' % (name, prefix, i)] for i in range(oct_n)}
    if '%s_%s_linear' % (name, prefix) in g:
        cells['linear'] = g['%s_%s_linear' % (name, prefix)]
    return cells


@pytest.fixture(scope="module")
def golden():
    return load("cqt_cells")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatement_reproduces_reference(golden, name):
    g = golden
    kind, kw, n = C.CASES[name]
    x = C.signal(name)
    np.testing.assert_array_equal(x, g[name + '_x'])
    assert x.size == n
    o = C.RefCells(kind, **kw)
    np.testing.assert_array_equal(o.scalars(), g[name + '_scalars'])
    cells = o.forward(x)
    np.testing.assert_array_equal(np.array(o.nframes), g[name + '_nframes'])
    ref = _cells(g, name, int(o.octaveNr))
    assert sorted(map(str, cells)) == sorted(map(str, ref))
    for key in ref:
        assert cells[key].shape == ref[key].shape
        assert rel(cells[key], ref[key]) < NUM
    # data movement: from the reference's own cells, bit for bit
    sp = o.cells_to_sp(ref)
    np.testing.assert_array_equal(sp, g[name + '_sp'])
    np.testing.assert_array_equal(o.time_stamps(), g[name + '_tstamps'])
    np.testing.assert_array_equal(o.freq_stamps(), g[name + '_fstamps'])
    assert rel(o.inverse(ref), g[name + '_y']) < NUM
    assert int(g[name + '_del']) == 1      # del transfo erases the cells too
    if name in C.ROUNDTRIP:
        new = C.modify(name, g[name + '_sp'], kw['bins'])
        back = o.sp_to_cells(new)
        rt = _cells(g, name, int(o.octaveNr), 'rt_cell')
        for key in rt:
            np.testing.assert_array_equal(back[key], rt[key])
        assert rel(o.inverse(rt), g[name + '_rt_y']) < NUM


def test_raster_structure(golden):
    """Populated columns are the complex cell samples; the columns between
    them are real; with winNr > 1 the last int(drop*nshifts) columns keep
    their pre-alignment values."""
    g = golden
    for name in sorted(C.CASES):
        kind, kw, _ = C.CASES[name]
        sp = g[name + '_sp']
        atomHOP, first_center, winNr, _, _, oct_n = g[name + '_scalars']
        bins, oct_n, winNr = kw['bins'], int(oct_n), int(winNr)
        for noct in range(1, oct_n):
            ns = 2 ** noct
            rows = sp[bins * (oct_n - noct - 1):bins * (oct_n - noct)]
            between = np.ones(sp.shape[1], dtype=bool)
            between[::ns] = False
            assert np.all(rows[:, between].imag == 0)
            assert np.any(rows[:, ::ns].imag != 0)
            cell = g['%s_cell%d' % (name, noct)]
            d = int(first_center / atomHOP * (2 ** (oct_n - noct - 1) - 1) * ns)
            j = np.arange(d // ns, cell.shape[1] * winNr)
            cols = j * ns - d
            np.testing.assert_array_equal(rows[0, cols], cell[j % winNr, j // winNr])


def test_interpolation_order_is_scipys():
    """interp_magnitudes states the operation order of interp1d(kind='linear')
    (the device kernel follows the same order): bit-equal on random data."""
    rs = np.random.RandomState(3)
    for ns, width in ((2, 365), (4, 365), (8, 252), (4, 80), (2, 7), (16, 33)):
        xint = np.arange(0, width, ns)
        y = np.abs(rs.randn(xint.size)) * 10.0 ** rs.randint(-8, 8, xint.size)
        f = spinterp.interp1d(x=xint, y=y, kind='linear', bounds_error=False, fill_value=0)
        np.testing.assert_array_equal(C.interp_magnitudes(y, ns, width), f(np.arange(width)))
