"""The E-step's balanced schedule (pyfasst_amd/csrc/fasst_esched.h): the
partition arithmetic on the host, and k_estep_mx under both schedules against
the oracle and against each other (run on MI355X).

The interesting cases are forced with FASST_ESTEP_NB on a small shape: F = 33
is three bin tiles, the last with one live bin; T = 16 * 9 + 5 is ten frame
tiles, the last with 5 live frames, so a bin tile has Q = 3 quad-steps (4, 4
and 2 frame tiles: the last one leaves two waves idle) and the work list has
U = 9 units.
  NB = 2   block 0 owns units [0, 4), block 1 [4, 9): each crosses a bin-tile
           boundary inside its range, and bin tile 1 is split over both
  NB = 9   one quad-step per block, three partial slots per bin tile
  NB = 1   one block does everything: two in-kernel epilogue / prologue turns
The deviations are held to the bounds tests/test_gpu_estep_matrix.py holds the
same quantities to, and the two schedules to each other at the same bounds.
Every GPU case prints its deviations ('estep-balanced ...') before asserting.

The E-step runs as one launch over the frames (EArgs.tbase stays 0 in
gem_iteration), so there is no several-launches case to force here.
"""
import ctypes

import numpy as np
import pytest

import fasst_ref as R  # noqa: F401  (the oracle, through test_gpu_parity._c3_like)
from helpers import rel, rel_elem
from test_gpu_parity import _c3_like

F, T, ITERS = 33, 16 * 9 + 5, 2
NBT, NTT, Q = 3, 10, 3


# ------------------------------------------------------------------ host only
def _partition(nbt, q, nb):
    from pyfasst_amd import _lib
    lo = (ctypes.c_longlong * (nb + 1))()
    first = (ctypes.c_int * nbt)()
    nseg = (ctypes.c_int * nbt)()
    mx = ctypes.c_int(0)
    _lib.check(_lib.lib.fasst_estep_partition(nbt, q, nb, lo, first, nseg, ctypes.byref(mx)),
               "fasst_estep_partition")
    return np.array(lo[:]), np.array(first[:]), np.array(nseg[:]), mx.value


def _grid():
    cases = [(129, 157, 512), (129, 157, 1024), (129, 157, 256), (129, 157, 129 * 157),
             (129, 157, 1), (129, 157, 511), (129, 157, 513), (NBT, Q, 2), (NBT, Q, 9),
             (NBT, Q, 1), (1, 1, 1), (1, 7, 3), (7, 1, 3), (7, 1, 7)]
    for nbt in (2, 3, 5, 16):
        for q in (1, 2, 3, 8, 13):
            for nb in sorted({1, 2, 3, nbt, nbt + 1, q, 2 * q + 1, nbt * q - 1, nbt * q}):
                if 1 <= nb <= nbt * q:
                    cases.append((nbt, q, nb))
    return sorted(set(cases))


@pytest.mark.parametrize("nbt,q,nb", _grid())
def test_partition_arithmetic(nbt, q, nb):
    """Every unit is owned exactly once, a bin tile's slots are dense from 0,
    nseg is the number of blocks that meet the bin tile, and the slot count
    the host allocates is the largest nseg."""
    lo, first, nseg, mx = _partition(nbt, q, nb)
    U = nbt * q
    # the blocks tile [0, U) in order: exact floor(b U / NB), no empty block
    assert lo[0] == 0 and lo[nb] == U
    assert np.array_equal(lo, (np.arange(nb + 1, dtype=np.int64) * U) // nb)
    assert np.all(np.diff(lo) >= 1)
    owner = np.repeat(np.arange(nb), np.diff(lo))       # unit -> its one block
    assert owner.shape == (U,)
    tile = np.arange(U) // q
    for bt in range(nbt):
        blocks = np.unique(owner[tile == bt])
        # the blocks that meet the bin tile are first .. first + nseg - 1:
        # their slots (block - first) are 0 .. nseg - 1, each used once
        assert blocks[0] == first[bt]
        assert len(blocks) == nseg[bt]
        assert np.array_equal(blocks - first[bt], np.arange(nseg[bt]))
    assert mx == nseg.max()


def test_partition_benchmark_shape():
    """F = 2049, T = 10000 on 512 resident slots: 39 or 40 quad-steps per
    block, at most two bin tiles per block, at most five slots per bin tile."""
    lo, first, nseg, mx = _partition(129, 157, 512)
    n = np.diff(lo)
    assert set(n) == {39, 40}
    assert np.all((lo[1:] - 1) // 157 - lo[:-1] // 157 <= 1)
    assert mx == 5 and nseg.min() >= 4


def test_partition_refuses_bad_shapes():
    from pyfasst_amd import _lib
    for nbt, q, nb in ((0, 3, 1), (3, 0, 1), (3, 3, 0), (3, 3, 10), (1 << 16, 1 << 15, 4)):
        assert _lib.lib.fasst_estep_partition(nbt, q, nb, None, None, None, None) == \
            _lib.FASST_ERR_SHAPE


# ------------------------------------------------------------------------ GPU
_ORACLE = {}
_RUNS = {}


def _results(m, J, X=None, oracle=False):
    res = {'ll': np.array(m.estim_param_a_post_model())}
    res['params'] = [np.array(m.spat_comps[j]['params']) for j in range(J)]
    res['FB'] = [np.array(m.spec_comps[j]['factor'][0]['FB']) for j in range(J)]
    res['TW'] = [np.array(m.spec_comps[j]['factor'][0]['TW']) for j in range(J)]
    res['absS'] = np.abs(m.separated_images(X) if oracle else m.separated_images())
    for v in res.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return res


def _run(J, K, ranks, sched, nb, monkeypatch, capfd, cache=True):
    """The product's results under one schedule (and the oracle's, once per
    model): sched 'chunk' | 'balanced', nb the balanced block count."""
    key = (J, K, tuple(ranks), sched, nb)
    if cache and key in _RUNS:
        return _RUNS[key], _ORACLE[key[:3]]
    monkeypatch.delenv("FASST_NCHUNK_E", raising=False)
    monkeypatch.setenv("FASST_ESTEP_SCHED", sched)
    monkeypatch.setenv("FASST_VERBOSE", "1")
    if nb:
        monkeypatch.setenv("FASST_ESTEP_NB", str(nb))
    else:
        monkeypatch.delenv("FASST_ESTEP_NB", raising=False)
    m, o, X = _c3_like(F, T, J, K, ranks, ITERS)
    if key[:3] not in _ORACLE:
        _ORACLE[key[:3]] = _results(o, J, X, oracle=True)
    res = _results(m, J)
    err = capfd.readouterr().err
    # the schedule asked for is the one that ran (not clamped or ignored)
    if sched == 'balanced':
        assert "estep %d balanced blocks" % nb in err, err
    else:
        assert "chunks" in err and "balanced" not in err, err
    if cache:
        _RUNS[key] = res
    return res, _ORACLE[key[:3]]


def _deviations(got, ref, J):
    d = {'ll': rel(got['ll'], ref['ll'])}
    for name in ('params', 'FB', 'TW'):
        for j in range(J):
            assert got[name][j].shape == ref[name][j].shape, (name, j)
        d[name] = max(rel(got[name][j], ref[name][j]) for j in range(J))
        if name != 'params':
            d[name + '_elem'] = max(rel_elem(got[name][j], ref[name][j]) for j in range(J))
    assert got['absS'].shape == ref['absS'].shape
    d['absS'] = rel(got['absS'], ref['absS'])
    d['absS_elem'] = rel_elem(got['absS'], ref['absS'])
    return d


def _assert_close(tag, d):
    """The bounds of tests/test_gpu_estep_matrix.py::_run_case."""
    print("estep-balanced %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(d.items()))))
    assert d['ll'] < 1e-10
    for name in ('params', 'FB', 'TW', 'absS'):
        assert d[name] < 1e-8, (name, d[name])
    for name in ('FB_elem', 'TW_elem', 'absS_elem'):
        assert d[name] < 1e-6, (name, d[name])


def _both(J, K, ranks, nb, monkeypatch, capfd):
    bal, ref = _run(J, K, ranks, 'balanced', nb, monkeypatch, capfd)
    chk, _ = _run(J, K, ranks, 'chunk', None, monkeypatch, capfd)
    tag = "J=%d K=%d r=%s NB=%d" % (J, K, "".join(map(str, ranks)), nb)
    _assert_close(tag + " balanced-vs-oracle", _deviations(bal, ref, J))
    _assert_close(tag + " chunk-vs-oracle", _deviations(chk, ref, J))
    _assert_close(tag + " balanced-vs-chunk", _deviations(bal, chk, J))


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2, 9, 1])
def test_boundary_j4(nb, monkeypatch, capfd):
    """J = 4, rank 2, K = 32 (two blocks per CU): a block that crosses a
    bin-tile boundary, a bin tile split over blocks, one quad-step per block,
    and one block for everything."""
    _both(4, 32, [2] * 4, nb, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2, 4])
def test_one_wave_per_simd_j8(nb, monkeypatch, capfd):
    """J = 8, K = 32 (the pipelined V tile, one block per CU, the epilogue one
    bin group at a time): NB = 2 and 4 both split a bin tile."""
    _both(8, 32, [1] * 8, nb, monkeypatch, capfd)


@pytest.mark.gpu
def test_ragged_rank_j2(monkeypatch, capfd):
    """J = 2, K = 16 with ranks (1, 2): the general-rank form (RKU = 0)."""
    _both(2, 16, [1, 2], 2, monkeypatch, capfd)


@pytest.mark.gpu
def test_balanced_is_deterministic(monkeypatch, capfd):
    """The partials are summed in slot order: two runs of the boundary case
    give bit-identical logliks and mixing parameters."""
    a, _ = _run(4, 32, [2] * 4, 'balanced', 2, monkeypatch, capfd, cache=False)
    b, _ = _run(4, 32, [2] * 4, 'balanced', 2, monkeypatch, capfd, cache=False)
    assert np.array_equal(a['ll'], b['ll'])
    for j in range(4):
        assert np.array_equal(a['params'][j], b['params'][j])
        assert np.array_equal(a['FB'][j], b['FB'][j])
        assert np.array_equal(a['TW'][j], b['TW'][j])
