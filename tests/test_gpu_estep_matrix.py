"""Every reachable E-step kernel instantiation, and its frame chunking,
against the oracle (run on MI355X).

Which E-step kernel fasst_run launches is decided from the model's shape, and
the instantiations are not one body with another trip count (MXShape<J>
changes the pair-group packing, the slab layout, the V pipelining, whether W
sits in LDS, the LDS size and the launch bounds), so each one gets a case of
its own here: the 80 k_estep_mx forms, the two k_egen_fused forms and the two
k_egen_point + k_egen_stats forms, the many-source ones and the J <= 8 forms
that never ran chunked also with several frame chunks (FASST_NCHUNK_E).
test_every_reachable_instance_has_a_case (CPU) fails when the parameter lists
below stop covering the set.

Every case prints its deviations ('estep-matrix ...') before asserting.
"""
import numpy as np
import pytest

import fasst_ref as R
from helpers import rel, rel_elem
from test_gpu_parity import _c3_like

# F = 37: three bin tiles of 16, the last with 5 live bins; T = 100: seven
# frame tiles, the last with 4 live frames; the second iteration's E-step runs
# on the W / prep state the fused tail left (w_ready, prep_ready)
F, T, ITERS = 37, 100, 2
# FASST_NCHUNK_E = 3 on seven frame tiles: chunks of 3, 3 and 1 tiles
NCHUNK = 3


def estep_instance(J, K, ranks):
    """The E-step kernel instantiation fasst_run launches for J sources of at
    most K NMF columns each with these spatial ranks.  Restates
    pyfasst_amd/csrc/fasst_em.hip (configure_model), fasst_em_estep.hip and
    fasst_em_estep_mx.h:
      configure_model   KP = K padded to 16 / 32 / 64 / 128 (NKS = KP / 4);
      launch_estep_phase (fasst_em_estep.hip)
                        J > 8 with KP <= 32 -> k_egen_fused<NKS>,
                        J > 8 otherwise -> k_egen_point<NKS> + k_egen_stats,
                        else launch_estep -> k_estep_mx<J, NKS, RKU>;
      estep_dispatch_r / _j (fasst_em_estep_mx.h)
                        RKU = 1 (every rank 1), 2 (every rank 2) or 0
                        (general ranks); KP = 128 has the general form only.
    A change to those functions must be restated here, and the completeness
    test then says which instantiations lost their case.
    """
    ranks = [ranks] * J if np.isscalar(ranks) else list(ranks)
    assert len(ranks) == J
    KP = 16 if K <= 16 else (32 if K <= 32 else (64 if K <= 64 else 128))
    nks = KP // 4
    if J > 8:
        return "fused<%d>" % nks if KP <= 32 else "point<%d>+stats" % nks
    if KP == 128:
        rku = 0
    elif all(r == 1 for r in ranks):
        rku = 1
    elif all(r == 2 for r in ranks):
        rku = 2
    else:
        rku = 0
    return "mx<%d,%d,%d>" % (J, nks, rku)


def _alt(J, first=1):
    """Alternating ranks [first, 3 - first, first, ...]."""
    return [first if j % 2 == 0 else 3 - first for j in range(J)]


def _general(J):
    return _alt(J) if J >= 2 else [3]


# one unaligned K per KP: 12 -> 16, 20 -> 32, 40 -> 64, 100 -> 128
K_OF_KP = {16: 12, 32: 20, 64: 40, 128: 100}


def _mx_matrix():
    """(J, K, ranks) of every k_estep_mx instantiation, from the dispatch
    matrix: J x KP in {16, 32, 64} x {all rank 1, all rank 2, general ranks},
    and the general-rank form at KP = 128."""
    cases = []
    for J in range(1, 9):
        for KP in (16, 32, 64):
            for ranks in ([1] * J, [2] * J, _general(J)):
                cases.append((J, K_OF_KP[KP], ranks))
        cases.append((J, K_OF_KP[128], _general(J)))
    return cases


MX_CASES = _mx_matrix()

# J > 8: family -> (J, K, ranks)
MANY_CASES = [
    # fused<4>
    (9, 12, [1] * 9), (11, 16, _alt(11, 2)), (16, 10, [2] * 16),     # (total ranks 9, 17, 32)
    # fused<8>
    (9, 20, [2] * 9), (12, 32, [1] * 12), (16, 24, [2] * 16),
    # point<16>+stats
    (9, 40, _alt(9)), (12, 48, [1] * 12), (16, 64, [2] * 16),
    # point<32>+stats
    (10, 100, [1] * 10), (12, 72, _alt(12)), (16, 128, [2] * 16),
]

# 'inst' mixing on the two-pass path: (J, K, ranks, F, T)
INST_CASE = (10, 40, [1] * 10, 65, 80)

# J <= 8 forms that never ran with more than one frame chunk: the J > 4
# pipelined form and the KP = 128 forms among them
MX_CHUNKED_CASES = [
    (5, 12, [2] * 5),
    (7, 40, _alt(7)),
    (8, 20, [1] * 8),
    (8, 128, [1] * 8),     # W read from L2 (mx_w_in_lds false)
    (4, 128, [2] * 4),     # one block per CU
    (6, 100, _alt(6)),
    (1, 20, [1]),
    (3, 40, [2] * 3),
]


def _id(case):
    J, K, ranks = case[:3]
    return "%s-J%d-K%d-r%s" % (estep_instance(J, K, ranks), J, K, "".join(map(str, ranks)))


def test_every_reachable_instance_has_a_case():
    """The parameter lists name every reachable instantiation: the 80
    k_estep_mx forms (sweep) and the four many-source forms (each unchunked
    and chunked)."""
    full = set()
    for J in range(1, 9):
        for nks in (4, 8, 16):
            for rku in (1, 2, 0):
                full.add("mx<%d,%d,%d>" % (J, nks, rku))
        full.add("mx<%d,32,0>" % J)
    assert len(full) == 80
    full |= {"fused<4>", "fused<8>", "point<16>+stats", "point<32>+stats"}
    assert len(full) == 84
    mx = [estep_instance(*c) for c in MX_CASES]
    assert len(mx) == 80 and len(set(mx)) == 80
    many = {estep_instance(*c) for c in MANY_CASES}
    assert many == {"fused<4>", "fused<8>", "point<16>+stats", "point<32>+stats"}
    assert set(mx) | many == full
    assert estep_instance(*INST_CASE[:3]) == "point<16>+stats"
    # the chunked J <= 8 cases are forms of the matrix, the J > 4 and KP = 128
    # ones among them
    chunked = {estep_instance(*c) for c in MX_CHUNKED_CASES}
    assert chunked <= set(mx)
    assert {"mx<8,32,0>", "mx<4,32,0>", "mx<7,16,0>"} <= chunked
    # the restated rule itself, at its edges
    assert estep_instance(8, 16, 1) == "mx<8,4,1>"
    assert estep_instance(8, 17, 2) == "mx<8,8,2>"
    assert estep_instance(8, 65, 2) == "mx<8,32,0>"
    assert estep_instance(9, 32, 1) == "fused<8>"
    assert estep_instance(9, 33, 1) == "point<16>+stats"
    assert estep_instance(16, 65, 2) == "point<32>+stats"
    assert estep_instance(1, 64, [3]) == "mx<1,16,0>"


def _inst_like(Fi, Ti, J, K, rank, iters=3):
    """'inst' mixing, product and oracle on identical inputs (built as
    test_gpu_parity.test_inst_many_sources_vs_oracle builds its model)."""
    import pyfasst_amd.audioModel as am
    from pyfasst_amd import synthetic
    from pyfasst_amd.audioObject import SpectralAudio
    X = synthetic.stereo_mixture(Fi, Ti, J=J, K_true=3, rank=1, seed=7)
    np.random.seed(5)
    m = am.MultiChanNMFInst_FASST(SpectralAudio(X=X), nbComps=J, nbNMFComps=K,
                                  spatial_rank=rank, iter_num=iters, wlen=128, hopsize=32)
    o = R.RefFASST(iter_num=iters)
    o.set_transform([X[0], X[1]])
    np.random.seed(5)
    R.init_nmf_inst(o, J, K, rank)
    return m, o, X


# the oracle's results per case, computed once and shared by the unchunked and
# the chunked run (the oracle has no chunks): key -> dict of read-only arrays
_ORACLE = {}


def _oracle_results(key, o, X, J):
    if key not in _ORACLE:
        res = {'ll': np.array(o.estim_param_a_post_model())}
        res['params'] = [np.array(o.spat_comps[j]['params']) for j in range(J)]
        res['FB'] = [np.array(o.spec_comps[j]['factor'][0]['FB']) for j in range(J)]
        res['TW'] = [np.array(o.spec_comps[j]['factor'][0]['TW']) for j in range(J)]
        res['absS'] = np.abs(o.separated_images(X))
        for v in res.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def _run_case(J, K, ranks, chunks, monkeypatch, capfd, shape=None):
    """Build product and oracle, run both, print and assert the deviations:
    the assertions of test_em_stft_domain_vs_oracle plus the elementwise metric
    (helpers.rel_elem, the bound of test_config3_every_point_vs_live_oracle),
    which alone sees a wrong value in a padded last bin / frame or a quiet
    source."""
    if chunks:
        # (read when the model is configured on the device)
        monkeypatch.setenv("FASST_NCHUNK_E", str(chunks))
        monkeypatch.setenv("FASST_VERBOSE", "1")
    else:
        monkeypatch.delenv("FASST_NCHUNK_E", raising=False)
    if shape is None:
        m, o, X = _c3_like(F, T, J, K, ranks, ITERS)
        key = ('conv', F, T, J, K, tuple(ranks))
    else:
        m, o, X = _inst_like(shape[0], shape[1], J, K, ranks[0])
        key = ('inst',) + tuple(shape) + (J, K, tuple(ranks))
    tw0 = max(rel(m.spec_comps[j]['factor'][0]['TW'], o.spec_comps[j]['factor'][0]['TW'])
              for j in range(J))
    ref = _oracle_results(key, o, X, J)
    ll = m.estim_param_a_post_model()
    S = np.abs(m.separated_images())
    err = capfd.readouterr().err if chunks else ""
    d = {'ll': rel(ll, ref['ll'])}
    for name, got in (('params', [m.spat_comps[j]['params'] for j in range(J)]),
                      ('FB', [m.spec_comps[j]['factor'][0]['FB'] for j in range(J)]),
                      ('TW', [m.spec_comps[j]['factor'][0]['TW'] for j in range(J)])):
        for j in range(J):
            assert got[j].shape == ref[name][j].shape, (name, j)
        d[name] = max(rel(got[j], ref[name][j]) for j in range(J))
        if name != 'params':
            d[name + '_elem'] = max(rel_elem(got[j], ref[name][j]) for j in range(J))
    assert S.shape == ref['absS'].shape
    d['absS'] = rel(S, ref['absS'])
    d['absS_elem'] = rel_elem(S, ref['absS'])
    print("estep-matrix %s J=%d K=%d chunks=%d tw0=%.3g %s" % (
        estep_instance(J, K, ranks), J, K, chunks or 1, tw0,
        " ".join("%s=%.3g" % kv for kv in sorted(d.items()))))
    if chunks:
        # a silently clamped chunk count would make this a repeat of the
        # unchunked case (configure_model's FASST_NCHUNK_E clamp in fasst_em.hip)
        assert "estep %d chunks" % chunks in err, err
    assert tw0 < 1e-14
    assert d['ll'] < 1e-10
    for name in ('params', 'FB', 'TW', 'absS'):
        assert d[name] < 1e-8, (name, d[name])
    for name in ('FB_elem', 'TW_elem', 'absS_elem'):
        assert d[name] < 1e-6, (name, d[name])


@pytest.mark.gpu
@pytest.mark.parametrize("case", MX_CASES, ids=_id)
def test_mx_instance_vs_oracle(case, monkeypatch, capfd):
    """J <= 8: each of the 80 k_estep_mx<J, NKS, RKU> instantiations."""
    J, K, ranks = case
    _run_case(J, K, ranks, None, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, NCHUNK], ids=["natural", "chunks3"])
@pytest.mark.parametrize("case", MANY_CASES, ids=_id)
def test_many_sources_instance_vs_oracle(case, chunks, monkeypatch, capfd):
    """J > 8: k_egen_fused<4 / 8> and k_egen_point<16 / 32> + k_egen_stats in
    the three rank forms, with one frame chunk and with three (3, 3 and the
    ragged 1 tile)."""
    J, K, ranks = case
    _run_case(J, K, ranks, chunks, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, NCHUNK], ids=["natural", "chunks3"])
def test_inst_two_pass_vs_oracle(chunks, monkeypatch, capfd):
    """'inst' mixing with J > 8 and KP > 32 (k_egen_point<16> + k_egen_stats;
    T = 80: five frame tiles, chunks of 2, 2 and 1)."""
    J, K, ranks, Fi, Ti = INST_CASE
    _run_case(J, K, ranks, chunks, monkeypatch, capfd, shape=(Fi, Ti))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MX_CHUNKED_CASES, ids=_id)
def test_mx_instance_chunked_vs_oracle(case, monkeypatch, capfd):
    """Three frame chunks on the k_estep_mx forms that never had them."""
    J, K, ranks = case
    _run_case(J, K, ranks, NCHUNK, monkeypatch, capfd)
