"""CQT / MinQT with perfRast=0 (the constructors' default) on the GPU against
the reference's own outputs, tests/golden/cqt_cells.npz.

Data movement (which raster column holds what, the zeros, the fold back into
cells) is compared bit for bit with the restatement tests/cqt_cells_ref.py,
given equal cells.  The numeric outputs (cells, interpolated magnitudes,
inverse) are held to TOL = 1e-10 of the largest magnitude, the bound
tests/test_gpu_cqt.py applies to the same FFT / product / filtfilt chain with
perfRast=1.  A case more sensitive than the cqt.npz cases gets that bound
scaled by the ratio, rounded up to one digit.  Largest relative move of the
restatement's output under a 1e-15 relative input perturbation, 5 draws
(tools/cqt_cells_sensitivity.py, on the CPU):

    cqt.npz cases (perfRast=1)   forward <= 1.32e-15   inverse <= 3.02e-15
    cqt12   cells / raster 1.32e-15   inverse 2.35e-15   -> 1e-10, 1e-10
    cqt24   cells / raster 1.53e-15   inverse 1.45e-15   -> 2e-10 (x1.16 -> 2), 1e-10
    mqt12   cells / raster 5.49e-16   inverse 2.43e-15   -> 1e-10, 1e-10
    mqt48   cells / raster 5.55e-16   inverse 2.14e-15   -> 1e-10, 1e-10

The raster is compared row by row as max|diff| / max|row|, so interpolated
magnitudes near zero are held to their own row and no sample is left out.
"""
import numpy as np
import pytest

import cqt_cells_ref as C
from helpers import CQT_CASES, load, rel

pytestmark = pytest.mark.gpu

TOL = 1e-10
FWD_TOL = {"cqt12": TOL, "cqt24": 2 * TOL, "mqt12": TOL, "mqt48": TOL}


def _product(name, **extra):
    from pyfasst_amd.tftransforms import minqt
    kind, kw, _ = C.CASES[name]
    kw = dict(kw, **extra)
    return (minqt.CQTransfo if kind == 'cqt' else minqt.MinQTransfo)(**kw)


def _ref_cells(g, name, oct_n, prefix='cell'):
    cells = {i: g['%s_%s%d' % (name, prefix, i)] for i in range(oct_n)}
    if '%s_%s_linear' % (name, prefix) in g:
        cells['linear'] = g['%s_%s_linear' % (name, prefix)]
    return cells


@pytest.fixture(scope="module")
def golden():
    return load("cqt_cells")


@pytest.fixture(scope="module")
def computed(golden):
    """Each case transformed once: (transform, cells, raster, inverse)."""
    out = {}
    for name in sorted(C.CASES):
        t = _product(name)
        assert t.perfRast == 0
        t.computeTransform(golden[name + '_x'])
        had_sp = hasattr(t, '_spCQT')
        cells = {k: np.array(v) for k, v in t.cellCQT.items()}
        sp = np.array(t.transfo)
        y = t.invertTransform()
        out[name] = (t, cells, sp, y, had_sp)
    return out


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_forward_cells_raster_inverse(golden, computed, name):
    g = golden
    t, cells, sp, y, had_sp = computed[name]
    k = t.cqtkernel
    np.testing.assert_array_equal(
        np.array([k.atomHOP, k.first_center, k.winNr, k.fftHOP, k.FFTLen, t.octaveNr],
                 dtype=np.float64), g[name + '_scalars'])
    np.testing.assert_array_equal(np.array(t.nframes), g[name + '_nframes'])
    assert not had_sp                       # computeTransform leaves only the cells
    assert t.prefixZeros == t.suffixZeros == t.maxBlock == int(k.FFTLen * 2 ** (t.octaveNr - 1))
    assert t.datalen_init == g[name + '_x'].size
    ref = _ref_cells(g, name, int(t.octaveNr))
    assert sorted(map(str, cells)) == sorted(map(str, ref))
    for key in ref:
        assert cells[key].shape == ref[key].shape
        assert rel(cells[key], ref[key]) < FWD_TOL[name], key
    assert sp.shape == g[name + '_sp'].shape
    for r in range(sp.shape[0]):
        assert rel(sp[r], g[name + '_sp'][r]) < FWD_TOL[name], r
    assert y.shape == g[name + '_y'].shape
    assert rel(y, g[name + '_y']) < TOL
    np.testing.assert_array_equal(t.time_stamps, g[name + '_tstamps'])
    np.testing.assert_array_equal(t.freq_stamps, g[name + '_fstamps'])


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_raster_is_the_restatements_given_equal_cells(golden, computed, name):
    """cellCQT2spCQT moves data and interpolates magnitudes in scipy's
    operation order: from the reference's cells the raster is the restatement's
    (and so the reference's) bit for bit; populated columns are complex and are
    the cell samples, interpolated columns have a zero imaginary part."""
    g = golden
    kind, kw, _ = C.CASES[name]
    t = computed[name][0]
    u = _product(name)
    for attr in ('datalen_init', 'maxBlock', 'prefixZeros', 'suffixZeros', 'nframes'):
        setattr(u, attr, getattr(t, attr))
    u.cellCQT = _ref_cells(g, name, int(t.octaveNr))
    sp = u.transfo
    np.testing.assert_array_equal(sp, g[name + '_sp'])
    bins, oct_n = kw['bins'], int(t.octaveNr)
    for noct in range(1, oct_n):
        ns = 2 ** noct
        rows = sp[bins * (oct_n - noct - 1):bins * (oct_n - noct)]
        between = np.ones(sp.shape[1], dtype=bool)
        between[::ns] = False
        assert np.all(rows[:, between].imag == 0)
        assert np.any(rows[:, ::ns].imag != 0)
    # the device's own cells: same structure
    own = computed[name][2]
    o = C.RefCells(kind, **kw)
    o.nframes = t.nframes
    np.testing.assert_array_equal(own, o.cells_to_sp(computed[name][1]))


@pytest.mark.parametrize("name", C.ROUNDTRIP)
def test_transfo_set_cells_inverse(golden, name):
    g = golden
    kind, kw, _ = C.CASES[name]
    t = _product(name)
    t.computeTransform(g[name + '_x'])
    new = C.modify(name, g[name + '_sp'], kw['bins'])
    t.transfo = new
    np.testing.assert_array_equal(t._spCQT, new)
    assert t._spCQT is not new
    rt = _ref_cells(g, name, int(t.octaveNr), 'rt_cell')
    assert sorted(map(str, t.cellCQT)) == sorted(map(str, rt))
    for key in rt:
        np.testing.assert_array_equal(t.cellCQT[key], rt[key])
    y = t.invertTransform()
    assert rel(y, g[name + '_rt_y']) < TOL
    # the spCQT setter re-derives the cells as well (minqt.py:731-735)
    t.spCQT = g[name + '_sp']
    o = C.RefCells(kind, **kw)
    o.nframes = t.nframes
    back = o.sp_to_cells(g[name + '_sp'])
    for key in back:
        np.testing.assert_array_equal(t.cellCQT[key], back[key])
    if kind == 'mqt':
        lin = t.invertLinearPart()
        assert rel(t.invertFromCellCQT() + lin, t.invertTransform()) < 1e-15
        assert np.max(np.abs(lin)) > 0


def test_state_machine_delete_and_recompute(golden, computed):
    g = golden
    name = "cqt12"
    t = _product(name)
    with pytest.raises(AttributeError):
        t.transfo
    t.computeTransform(g[name + '_x'])
    with pytest.raises(AttributeError):     # no _spCQT yet: `del self._spCQT` (minqt.py:668)
        del t.transfo
    sp = np.array(t.transfo)
    assert hasattr(t, '_spCQT')
    del t._spCQT                            # the getter recomputes from the cells
    np.testing.assert_array_equal(t.transfo, sp)
    np.testing.assert_array_equal(t.spCQT, sp)
    del t.transfo                           # "erasing everything" (minqt.py:665-669)
    assert not hasattr(t, '_spCQT') and not hasattr(t, 'cellCQT')
    assert int(g[name + '_del']) == 1
    with pytest.raises(AttributeError):
        t.transfo
    with pytest.raises(ValueError):
        t.transfo = np.zeros((3, 4), dtype=complex)


def test_two_runs_are_bit_equal(golden, computed):
    for name in ("cqt24", "mqt12"):
        t, cells, sp, y, _ = computed[name]
        u = _product(name)
        u.computeTransform(golden[name + '_x'])
        for key in cells:
            np.testing.assert_array_equal(u.cellCQT[key], cells[key])
        np.testing.assert_array_equal(u.transfo, sp)
        np.testing.assert_array_equal(u.invertTransform(), y)


def test_perfrast1_unchanged_beside_a_perfrast0_context(golden):
    from pyfasst_amd.tftransforms import minqt
    g1 = load("cqt")
    name, kind, kw = CQT_CASES[3]           # cqt12
    a = minqt.CQTransfo(perfRast=1, **kw)
    a.computeTransform(g1['x'])
    before = np.array(a.transfo)
    b = minqt.CQTransfo(perfRast=0, **kw)
    b.computeTransform(g1['x'])
    b.transfo
    b.invertTransform()
    a.computeTransform(g1['x'])
    np.testing.assert_array_equal(a.transfo, before)
    assert rel(before, g1['X_' + name]) < TOL


def test_tft_defaults_run_end_to_end():
    from pyfasst_amd.tftransforms import tft
    rs = np.random.RandomState(2)
    x = rs.randn(1500)
    for key, args in (('cqt', dict(fmin=400, fmax=3000, bins=12, fs=8000)),
                      ('mqt', dict(fmax=3000, bins=12, linFTLen=256, fs=8000, fmin=120)),
                      ('minqt', dict(fmax=3000, bins=12, linFTLen=256, fs=8000, fmin=120))):
        t = tft.tftransforms[key](**args)
        assert t.perfRast == 0
        t.computeTransform(x)
        X = t.transfo
        assert X.shape == (int(t.freqbins), int(t.nframes[0] * t.cqtkernel.winNr))
        t.transfo = X
        assert t.invertTransform().shape == x.shape


def test_short_signal_raises_with_perfrast0():
    from pyfasst_amd.tftransforms import minqt
    t = minqt.CQTransfo(fmin=30, fmax=3000, bins=12, fs=8000, atomHopFactor=0.25)
    with pytest.raises(ValueError):
        t.computeTransform(np.zeros(0))
