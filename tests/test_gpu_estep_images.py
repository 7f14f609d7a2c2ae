"""The single-pass E-step's tile-packed operand images (fasst_em_estep.hip:
k_cx_image, k_tw_image; the image store of the fused k_tw_update; and the
CXI / TWI forms of k_estep_mx, fasst_em_estep_mx.h), selected by
FASST_ESTEP_IMG = 0 | cx | tw | 1 when a context is created.

The images change where the operands are read from, not their values nor any
arithmetic instruction, so every comparison between two image settings here is
bit equality (np.array_equal), never a tolerance: 3 GEM iterations with
FASST_ESTEP_IMG=0 (the plane loads) against each of cx, tw and 1 on fresh
contexts with the same seeds; logliks, mixing parameters, FB, FW and TW.

Shapes (16 x 16 tiles, four waves per block walking frame tiles tt += 4):
  F = 65, T = 77    4 * 16 + 1 bins and 4 * 16 + 13 frames: a ragged last bin
                    tile, a ragged last frame tile, and a last quad-step with
                    one live wave (5 frame tiles)
  F = 33, T = 40    three frame tiles: the only quad-step has three live waves
  F = 200, T = 700  13 bin tiles x 11 quad-steps on 5 balanced blocks: every
                    block walks several bin-tile segments
The staleness tests run one context twice: the Cx image must follow a second
observation, the TW image an upload (fasst_set_spectral) and a restarted batch.
"""
import numpy as np
import pytest

import fasst_ref as R  # noqa: F401  (the oracle, through the imported builders)
from helpers import rel
from test_gpu_fast_tail import _dead_tw, _models

ITERS = 3
IMG_MODES = ["cx", "tw", "1"]


# ------------------------------------------------------------------ host only
def _cx_image(planes, nft, ntt):
    """k_cx_image: planes [4][Tp][Fp] -> flat doubles, record (bt, tt) of 512
    double2 at (bt ntt + tt) 512; element e = 64 piece + lane."""
    img = np.empty(nft * ntt * 512 * 2)
    for bt in range(nft):
        for tt in range(ntt):
            rec = (bt * ntt + tt) * 512
            for e in range(512):
                piece, lane = e >> 6, e & 63
                i, fl, tq = piece >> 1, lane & 15, lane >> 4
                t, f = 16 * tt + tq + 4 * i, 16 * bt + fl
                lo, hi = (2, 3) if piece & 1 else (0, 1)
                img[2 * (rec + e)] = planes[lo, t, f]
                img[2 * (rec + e) + 1] = planes[hi, t, f]
    return img


def _tw_image(TW, J, KP, ntt):
    """k_tw_image / tw_image_store: TW [J][KP][Tp] -> flat doubles, piece
    (tt, j, u) of 64 double2; element e = 64 u + lane."""
    img = np.empty(ntt * J * (KP // 8) * 64 * 2)
    for tt in range(ntt):
        for j in range(J):
            for e in range((KP // 8) * 64):
                u, lane = e >> 6, e & 63
                fl, tq = lane & 15, lane >> 4
                o = ((tt * J + j) * (KP // 8)) * 64 + e
                img[2 * o] = TW[j, tq + 8 * u, 16 * tt + fl]
                img[2 * o + 1] = TW[j, tq + 8 * u + 4, 16 * tt + fl]
    return img


def test_image_index_maps_host():
    """The two layouts restated in NumPy on random padded planes, read back
    as k_estep_mx reads them (a 16-byte load at record base + uniform piece
    offset + lane * 16), reproduce the plane form's c[p][i] and twv[j][s] for
    every lane of every tile, the ragged ones included."""
    rng = np.random.RandomState(3)
    F, T, J, KP = 65, 77, 3, 32
    Fp, Tp = 80, 80
    nft, ntt, NKS = Fp // 16, Tp // 16, KP // 4
    planes = np.zeros((4, Tp, Fp))
    planes[:, :T, :F] = rng.randn(4, T, F)
    TW = np.zeros((J, KP, Tp))
    TW[:, :20, :T] = rng.rand(J, 20, T)
    cxp, twp = _cx_image(planes, nft, ntt), _tw_image(TW, J, KP, ntt)
    assert cxp.size == planes.size and twp.size == TW.size

    def ld16(buf, base_bytes, so, vo):
        o = (base_bytes + so + vo) // 8
        return buf[o], buf[o + 1]

    for bt in range(nft):
        for tt in range(ntt):
            for lane in range(64):
                fl, tq = lane & 15, lane >> 4
                f, t0 = 16 * bt + fl, 16 * tt
                base = (bt * ntt + tt) * 512 * 16
                for i in range(4):
                    d = ld16(cxp, base, (2 * i) * 1024, lane * 16)
                    o = ld16(cxp, base, (2 * i + 1) * 1024, lane * 16)
                    want = planes[:, t0 + tq + 4 * i, f]
                    assert (d[0], d[1], o[0], o[1]) == tuple(want)
                if bt:
                    continue
                base = tt * (J * (NKS // 2) * 64) * 16
                for j in range(J):
                    for u in range(NKS // 2):
                        h = ld16(twp, base, (j * (NKS // 2) + u) * 1024, lane * 16)
                        for s, got in ((2 * u, h[0]), (2 * u + 1, h[1])):
                            assert got == TW[j, tq + 4 * s, t0 + fl]


# ------------------------------------------------------------------------ GPU
def _snapshot(m, ll, J):
    res = {'ll': np.array(ll)}
    res['params'] = [np.array(m.spat_comps[j]['params']) for j in range(J)]
    for key in ('FB', 'FW', 'TW'):
        res[key] = [np.array(m.spec_comps[j]['factor'][0][key]) for j in range(J)]
    return res


def _assert_bit_equal(a, b, tag):
    assert np.array_equal(a['ll'], b['ll']), (tag, 'll', a['ll'], b['ll'])
    for key in ('params', 'FB', 'FW', 'TW'):
        for j, (x, y) in enumerate(zip(a[key], b[key])):
            assert x.shape == y.shape and np.array_equal(x, y), (tag, key, j)


def _env(monkeypatch, img, env):
    for k in ("FASST_ESTEP_SCHED", "FASST_ESTEP_NB", "FASST_NCHUNK_E", "FASST_FAST_TAIL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if img is None:
        monkeypatch.delenv("FASST_ESTEP_IMG", raising=False)
    else:
        monkeypatch.setenv("FASST_ESTEP_IMG", img)


def _gem(monkeypatch, img, args, conv=True, env={}):
    _env(monkeypatch, img, env)
    m, _, _ = _models(*args, conv=conv)
    ll = m.estim_param_a_post_model()
    return _snapshot(m, ll, args[2])


CASES = {
    # (F, T, J, K, rank, iters), conv, environment
    'c3-ragged': ((65, 77, 4, 32, 2, ITERS), True, {}),
    'preload-j2-k64': ((33, 40, 2, 64, 2, ITERS), True, {}),      # NKS = 16, J NKS = 32
    'preload-j3-k32': ((33, 40, 3, 32, 2, ITERS), True, {}),
    # K = 20 is padded to KP = 32 (NKS = 8, not 5): the preload path with zero rows
    'k20-padded': ((33, 40, 4, 20, 2, ITERS), True, {}),
    # TW from the planes beside the Cx image: the pipelined forms VR (J > 4) and
    # CP (J NKS > 32)
    'vr-j6': ((33, 40, 6, 32, 2, ITERS), True, {}),
    'cp-j4-k64': ((33, 40, 4, 64, 2, ITERS), True, {}),
    'segments': ((200, 700, 4, 32, 2, ITERS), True,
                 {"FASST_ESTEP_SCHED": "balanced", "FASST_ESTEP_NB": "5"}),
    'inst': ((65, 77, 4, 32, 2, ITERS), False, {}),
    'unfused-tail': ((65, 77, 4, 32, 2, ITERS), True, {"FASST_FAST_TAIL": "0"}),
}
_PLANES = {}


@pytest.mark.gpu
@pytest.mark.parametrize("img", IMG_MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_images_bit_equal_to_planes(monkeypatch, case, img):
    args, conv, env = CASES[case]
    if case not in _PLANES:
        _PLANES[case] = _gem(monkeypatch, "0", args, conv, env)
    got = _gem(monkeypatch, img, args, conv, env)
    assert np.all(np.isfinite(got['ll']))
    _assert_bit_equal(got, _PLANES[case], "%s img=%s" % (case, img))


@pytest.mark.gpu
def test_images_default_vs_oracle(monkeypatch):
    """The first case under the default setting against the oracle, with the
    checks of tests/test_gpu_parity.py::test_em_stft_domain_vs_oracle."""
    _env(monkeypatch, None, {})
    args = CASES['c3-ragged'][0]
    J = args[2]
    m, o, X = _models(*args)
    ll = m.estim_param_a_post_model()
    llo = o.estim_param_a_post_model()
    assert rel(ll, llo) < 1e-10
    for j in range(J):
        assert rel(m.spat_comps[j]['params'], o.spat_comps[j]['params']) < 1e-8
        assert rel(m.spec_comps[j]['factor'][0]['FB'], o.spec_comps[j]['factor'][0]['FB']) < 1e-8
        assert rel(m.spec_comps[j]['factor'][0]['TW'], o.spec_comps[j]['factor'][0]['TW']) < 1e-8
    assert rel(np.abs(m.separated_images()), np.abs(o.separated_images(X))) < 1e-8


def _host_params(m, J):
    return ([np.array(m.spat_comps[j]['params']) for j in range(J)],
            [{k: np.array(m.spec_comps[j]['factor'][0][k]) for k in ('FB', 'FW', 'TW')}
             for j in range(J)])


def _restore(m, saved, J):
    for j in range(J):
        m.spat_comps[j]['params'] = np.array(saved[0][j])
        for k in ('FB', 'FW', 'TW'):
            m.spec_comps[j]['factor'][0][k] = np.array(saved[1][j][k])


@pytest.mark.gpu
@pytest.mark.parametrize("img", IMG_MODES)
def test_cx_image_follows_a_second_observation(monkeypatch, img):
    """One context: Cx, run, another Cx, run from the same parameters; against
    a fresh context given the second Cx alone."""
    _env(monkeypatch, img, {})
    args = (65, 77, 4, 32, 2, ITERS)
    J = args[2]
    other, _, _ = _models(*args, seed=7)
    cx2 = np.array(other.Cx)
    m, _, _ = _models(*args)
    assert not np.array_equal(cx2, np.array(m.Cx))
    init = _host_params(m, J)
    m.estim_param_a_post_model()
    m.Cx = cx2
    _restore(m, init, J)
    twice = _snapshot(m, m.estim_param_a_post_model(), J)
    f, _, _ = _models(*args)
    f.Cx = cx2
    fresh = _snapshot(f, f.estim_param_a_post_model(), J)
    _assert_bit_equal(twice, fresh, "second Cx img=%s" % img)


@pytest.mark.gpu
@pytest.mark.parametrize("img", IMG_MODES)
def test_tw_image_follows_an_upload(monkeypatch, img):
    """One context run twice, the parameters re-uploaded (fasst_set_spectral)
    in between: the second run starts from the uploaded TW, not from the image
    the first run's last k_tw_update left."""
    _env(monkeypatch, img, {})
    args = (65, 77, 4, 32, 2, ITERS)
    J = args[2]
    m, _, _ = _models(*args)
    init = _host_params(m, J)
    first = _snapshot(m, m.estim_param_a_post_model(), J)
    _restore(m, init, J)
    second = _snapshot(m, m.estim_param_a_post_model(), J)
    _assert_bit_equal(second, first, "re-upload img=%s" % img)


@pytest.mark.gpu
@pytest.mark.parametrize("img", IMG_MODES)
def test_tw_image_after_a_restart(monkeypatch, img):
    """tests/test_gpu_fast_tail.py's restart shape: a dead TW row halts the
    batch, the host redraws TW and uploads it; bit-equal to the plane loads."""
    args = (33, 40, 2, 4, 1, 5)

    def run(mode):
        _env(monkeypatch, mode, {})
        m, _, _ = _models(*args)
        _dead_tw(m)
        np.random.seed(11)
        return _snapshot(m, m.estim_param_a_post_model(), 2)

    _assert_bit_equal(run(img), run("0"), "restart img=%s" % img)
