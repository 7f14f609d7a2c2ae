"""The FP64 MFMA GEMM layer called directly (run on MI355X): every k_gemm
instantiation the library holds and every dispatch arm of dgemm2, through
fasst_gemm_probe / fasst_dgemm2_probe (pyfasst_amd/csrc/fasst_gemm.hip).

The reference is the product itself, in two forms.
  exact    operands are integers in [-8, 8] held as float64.  With K <= 2049
           every partial sum is an integer below 2^53, so any summation order
           and any FMA contraction give the same bits: the check is
           assert_array_equal against the int64 product.  A missing, doubled
           or misplaced k-term anywhere fails it.
  rounded  operands are signed gamma(0.7) draws (several decades); the
           reference is the np.longdouble product and the bound the standard
           forward bound of a K-term inner product in any order,
           |C - C_ref| <= gamma_K (|A| |B|), gamma_K = K u / (1 - K u),
           u = 2^-53, elementwise.
Every case poisons what the kernel must not use or touch: operand padding is
NaN (a NaN in a stored output means a pad element was consumed), C arrives
filled with a sentinel and every element outside its [M][N] block must come
back holding the sentinel's bits, and the guard tails behind the device
buffers must be intact.
"""
import ctypes

import numpy as np
import pytest

from test_gemm_plan import plan

SENT = np.float64(-1.2345678912345e+200)
SENT_BITS = np.array([SENT]).view(np.uint64)[0]
U = 2.0 ** -53


# ------------------------------------------------------------------ operands
def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def _gammas(rng, shape):
    return rng.gamma(0.7, size=shape) * rng.choice([-1.0, 1.0], size=shape)


def _store(mat, ld):
    """mat [rows][cols] as a [rows][ld] array, the padding NaN"""
    out = np.full((mat.shape[0], ld), np.nan)
    out[:, :mat.shape[1]] = mat
    return out


def _exact_ref(a, b):
    return (a.astype(np.int64) @ b.astype(np.int64)).astype(np.float64)


def _assert_rounded(c, a, b, what):
    K = a.shape[1]
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    ref, mag = al @ bl, np.abs(al) @ np.abs(bl)
    gam = np.longdouble(K * U) / (1 - np.longdouble(K * U))
    assert not np.isnan(c).any(), what
    ratio = np.max(np.abs(c.astype(np.longdouble) - ref) / (gam * mag))
    print("gemm-direct %s: max |C - ref| / (gamma_K |A||B|) = %.3g" % (what, float(ratio)))
    assert ratio <= 1.0, what


def _assert_sentinel(block, what):
    assert np.array_equal(block.view(np.uint64), np.full(block.shape, SENT_BITS)), what


# ---------------------------------------------------------------- gemm<> probe
OK, ERR_SHAPE, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 3, 6


def _stop_on_device_error(st):
    """A HIP failure (a kernel fault among them) leaves the device context
    unusable: end the session instead of launching the remaining cases on it."""
    if st == ERR_DEVICE:
        from pyfasst_amd import _lib
        pytest.exit("GEMM probe: device error: %s" % _lib.last_error(), returncode=3)


def gemm_probe(ta, tb, nb, a, bs, pads=(0, 0, 0), use_work=1, bcols=False):
    """a = opA [M][K], bs = nb opB [K][N]; pads = extra lda, ldb, ldc.
    Returns (status, C [nb][M][ldc], nz_ran, guard_ok)."""
    from pyfasst_amd import _lib
    M, K = a.shape
    N = bs[0].shape[1]
    A = _store(a.T if ta else a, (M if ta else K) + pads[0])
    if bcols:
        B = _store(np.concatenate(bs, axis=1), nb * N + pads[1])
    else:
        B = np.stack([_store(b.T if tb else b, (K if tb else N) + pads[1]) for b in bs])
    C = np.full((nb, M, N + pads[2]), SENT)
    nz, ok = ctypes.c_int(-1), ctypes.c_int(-1)
    st = _lib.lib.fasst_gemm_probe(0, ta, tb, nb, M, N, K, _lib.dptr(A), A.shape[-1], _lib.dptr(B),
                                   B.shape[-1], _lib.dptr(C), C.shape[-1],
                                   (1 if use_work else 0) | (2 if bcols else 0),
                                   ctypes.byref(nz), ctypes.byref(ok))
    _stop_on_device_error(st)
    return st, C, nz.value, ok.value


def _operands(kind, nb, M, N, K, seed):
    rng = np.random.default_rng([seed, nb, M, N, K, int(kind == "exact")])
    draw = _ints if kind == "exact" else _gammas
    return draw(rng, (M, K)), [draw(rng, (K, N)) for _ in range(nb)]


def _check_gemm(kind, a, bs, C, N, what):
    for b, bmat in enumerate(bs):
        if kind == "exact":
            np.testing.assert_array_equal(C[b][:, :N], _exact_ref(a, bmat), err_msg="%s b=%d" % (what, b))
        else:
            _assert_rounded(C[b][:, :N], a, bmat, "%s b=%d" % (what, b))
    _assert_sentinel(C[:, :, N:], what)


def _run_gemm(kind, ta, tb, nb, M, N, K, pads=(0, 0, 0), use_work=1, bcols=False, seed=0):
    a, bs = _operands(kind, nb, M, N, K, seed)
    st, C, nz, ok = gemm_probe(ta, tb, nb, a, bs, pads, use_work, bcols)
    what = "gemm<%d,%d,%d> M %d N %d K %d pads %s work %d %s" % (ta, tb, nb, M, N, K, pads, use_work, kind)
    assert st == OK, what
    assert ok == 1, what
    _check_gemm(kind, a, bs, C, N, what)
    return C, nz


INSTANCES = ((0, 0, 1), (1, 0, 1), (1, 0, 2), (1, 0, 4), (0, 1, 1), (0, 1, 2))

# per operand count and tile shape (wgm, wtm, wtn): the interior shape (M, N
# multiples of the block tile, two blocks, K = 32) and two ragged ones (M and N
# one past an MFMA-tile or block-tile edge, or 1; K = 17 and K = 1), all on
# the side of tile_shape's thresholds that selects the shape
SHAPES = {
    1: {(1, 3, 2): ((48, 256, 32), (17, 129, 17), (1, 257, 1)),       # 48 x 128
        (4, 2, 3): ((256, 48, 32), (129, 17, 17), (257, 1, 1)),       # 128 x 48
        (2, 4, 4): ((256, 128, 32), (129, 129, 17), (49, 257, 1))},   # 128 x 128
    2: {(1, 3, 2): ((48, 256, 32), (17, 129, 17), (1, 257, 1)),       # 48 x 128
        (2, 2, 4): ((64, 256, 32), (49, 129, 17), (64, 1, 1)),        # 64 x 128
        (2, 4, 2): ((256, 64, 32), (129, 65, 17), (65, 1, 1))},       # 128 x 64
    4: {(1, 3, 1): ((48, 128, 32), (17, 65, 17), (1, 129, 1)),        # 48 x 64
        (2, 2, 2): ((128, 64, 32), (65, 65, 17), (49, 1, 1))},        # 64 x 64
}
# the 17 k_gemm<TA, TB, NB, WGM, WTM, WTN> the library instantiates
KERNELS = {
    (0, 0, 1, 1, 3, 2), (0, 0, 1, 4, 2, 3), (0, 0, 1, 2, 4, 4),
    (1, 0, 1, 1, 3, 2), (1, 0, 1, 4, 2, 3), (1, 0, 1, 2, 4, 4),
    (0, 1, 1, 1, 3, 2), (0, 1, 1, 4, 2, 3), (0, 1, 1, 2, 4, 4),
    (1, 0, 2, 1, 3, 2), (1, 0, 2, 2, 2, 4), (1, 0, 2, 2, 4, 2),
    (0, 1, 2, 1, 3, 2), (0, 1, 2, 2, 2, 4), (0, 1, 2, 2, 4, 2),
    (1, 0, 4, 1, 3, 1), (1, 0, 4, 2, 2, 2),
}

KERNEL_CASES = [(ta, tb, nb, shape, i) for (ta, tb, nb) in INSTANCES
                for shape in SHAPES[nb] for i in range(3)]
# tile_shape's thresholds: (nb, M, N, shape)
THRESHOLDS = [(2, 48, 50, (1, 3, 2)), (2, 49, 50, (2, 2, 4)), (2, 64, 50, (2, 2, 4)),
              (2, 65, 50, (2, 4, 2)), (1, 65, 48, (4, 2, 3)), (1, 65, 49, (2, 4, 4)),
              (1, 48, 49, (1, 3, 2)), (1, 49, 48, (4, 2, 3)),
              (4, 48, 50, (1, 3, 1)), (4, 49, 50, (2, 2, 2))]
THRESHOLD_CASES = [(ta, tb, nb, M, N, shape) for (ta, tb, nb) in INSTANCES
                   for (tnb, M, N, shape) in THRESHOLDS if tnb == nb]
SPLIT_CASES = [(ta, tb, nb, M, N, K) for (ta, tb, nb) in INSTANCES
               for (M, N) in ((40, 50), (65, 49)) for K in (128, 130, 257, 1030)]


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb,nb,shape,i", KERNEL_CASES)
def test_gemm_every_kernel(ta, tb, nb, shape, i):
    """Interior-only and ragged shapes of each of the 17 kernels; the ragged
    ones with every leading dimension padded, the K = 17 one also on the
    rounded operands."""
    M, N, K = SHAPES[nb][shape][i]
    assert plan(M, N, K, nb)[2] == shape
    pads = (0, 0, 0) if i == 0 else (3, 5, 2)
    _, nz = _run_gemm("exact", ta, tb, nb, M, N, K, pads)
    assert nz == 1
    if i == 1:
        _run_gemm("rounded", ta, tb, nb, M, N, K, pads)
        _run_gemm("exact", ta, tb, nb, M, N, K, (1, 0, 0), use_work=0)


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb,nb,M,N,shape", THRESHOLD_CASES)
def test_gemm_tile_shape_thresholds(ta, tb, nb, M, N, shape):
    assert plan(M, N, 20, nb)[2] == shape
    _run_gemm("exact", ta, tb, nb, M, N, 20, (2, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb,nb,M,N,K", SPLIT_CASES)
def test_gemm_split_k(ta, tb, nb, M, N, K):
    """With a workspace the product runs the planned splits (ragged last chunk
    at K = 130, 257, 1030; 13 splits planned as 16 at K = 1030), without one it
    runs unsplit, and both are the product; the slab reduction has a fixed
    order, so two split runs agree to the bit."""
    nz_plan = plan(M, N, K, nb)[0]
    assert nz_plan > 1
    pads = (1, 3, 0)
    C1, nz = _run_gemm("exact", ta, tb, nb, M, N, K, pads, use_work=1)
    assert nz == nz_plan
    C0, nz = _run_gemm("exact", ta, tb, nb, M, N, K, pads, use_work=0)
    assert nz == 1
    np.testing.assert_array_equal(C0, C1)
    Ca, nz = _run_gemm("rounded", ta, tb, nb, M, N, K, pads, use_work=1)
    assert nz == nz_plan
    Cb, _ = _run_gemm("rounded", ta, tb, nb, M, N, K, pads, use_work=1)
    assert np.array_equal(Ca.view(np.uint64), Cb.view(np.uint64))
    _run_gemm("rounded", ta, tb, nb, M, N, K, pads, use_work=0)


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb,nb", INSTANCES)
def test_gemm_split_k_refuses_a_padded_output(ta, tb, nb):
    """Split-K slabs are reduced into a dense C: ldc != N is FASST_ERR_SHAPE
    before anything is launched, so C comes back untouched.  Without a
    workspace the same call runs unsplit into the padded C."""
    from pyfasst_amd import _lib
    M, N, K = 40, 50, 257
    a, bs = _operands("exact", nb, M, N, K, 1)
    st, C, _, _ = gemm_probe(ta, tb, nb, a, bs, (0, 0, 2), use_work=1)
    assert st == ERR_SHAPE
    assert "ldc" in _lib.last_error()
    _assert_sentinel(C, "refused split")
    _, nz = _run_gemm("exact", ta, tb, nb, M, N, K, (0, 0, 2), use_work=0, seed=1)
    assert nz == 1


@pytest.mark.gpu
@pytest.mark.parametrize("K,use_work", [(70, 0), (257, 1), (257, 0)])
def test_gemm_column_block_operands(K, use_work):
    """The production layout of the two-operand calls: B[1] = B[0] + N in one
    [K][2 N] array."""
    M, N = 50, 37
    _, nz = _run_gemm("exact", 1, 0, 2, M, N, K, (1, 0, 0), use_work, bcols=True)
    assert nz == (plan(M, N, K, 2)[0] if use_work else 1)
    _run_gemm("rounded", 1, 0, 2, M, N, K, (1, 0, 0), use_work, bcols=True)


@pytest.mark.gpu
def test_gemm_full_grid_is_not_split():
    """16 x 131077: 1025 tiles fill the grid, so K = 128 runs unsplit even
    with a workspace on offer."""
    M, N, K = 16, 131077, 128
    assert plan(M, N, K, 1)[0] == 1
    _, nz = _run_gemm("exact", 0, 0, 1, M, N, K, (0, 0, 0), use_work=1)
    assert nz == 1


@pytest.mark.gpu
def test_gemm_probe_refuses_other_forms():
    from pyfasst_amd import _lib
    a, bs = _operands("exact", 4, 8, 8, 8, 0)
    for ta, tb, nb in ((1, 1, 1), (0, 0, 2), (0, 1, 4), (0, 0, 4), (1, 1, 2), (1, 0, 3)):
        st, C, _, _ = gemm_probe(ta, tb, nb, a, bs[:nb])
        assert st == ERR_UNSUPPORTED, (ta, tb, nb)
        assert "not instantiated" in _lib.last_error()
        _assert_sentinel(C, "unsupported form")


@pytest.mark.gpu
def test_gemm_cases_cover_the_17_kernels():
    """The parametrised cases above, through the plan the launch dispatches
    on, name each of the 17 instantiated kernels (and nothing else)."""
    seen = set()
    for ta, tb, nb, shape, i in KERNEL_CASES:
        M, N, K = SHAPES[nb][shape][i]
        seen.add((ta, tb, nb) + plan(M, N, K, nb)[2])
    assert seen == KERNELS and len(KERNELS) == 17
    # every kernel has all three of its cases
    for k in KERNELS:
        assert sum((ta, tb, nb) + shape == k for ta, tb, nb, shape, _ in KERNEL_CASES) == 3
    other = set()
    for ta, tb, nb, M, N, shape in THRESHOLD_CASES:
        other.add((ta, tb, nb) + plan(M, N, 20, nb)[2])
    for ta, tb, nb, M, N, K in SPLIT_CASES:
        other.add((ta, tb, nb) + plan(M, N, K, nb)[2])
    assert other <= KERNELS
    print("gemm-direct coverage: %d/17 k_gemm kernels" % len(seen))


# --------------------------------------------------------------------- dgemm2
BUF, FLAT, B4, A4, A4B4 = 0, 1, 2, 3, 4
# alignment variant -> (lda odd, a_skew, ldb odd, b_skew, flat, arm)
VARIANTS = {
    "buf": (0, 0, 0, 0, 0, BUF),
    "flat": (0, 0, 0, 0, 1, FLAT),
    "a4_odd": (1, 0, 0, 0, 0, A4),
    "a4_skew": (0, 1, 0, 0, 0, A4),
    "b4_odd": (0, 0, 1, 0, 0, B4),
    "b4_skew": (0, 0, 0, 1, 1, B4),      # flat is moot off D2Prod
    "a4b4_odd": (1, 0, 1, 0, 0, A4B4),
    "a4b4_skew": (0, 1, 0, 1, 0, A4B4),
}


def _ld(n, odd, tight):
    """the leading dimension for n columns: n itself when tight (and of the
    parity asked for), else the next value above n of that parity, so that at
    least one NaN pad column follows the rows (for odd n and an even ld it is
    column n, the second half of the last 16-byte load)"""
    if tight:
        assert n % 2 == odd
        return n
    return n + 1 if (n + 1) % 2 == odd else n + 2


def dgemm2_probe(a, b, lda, a_skew, ldb, b_skew, ldc, flat, same=False):
    """a = A [K][M], b = B [K][N].  Returns (status, C [M][ldc], arm)."""
    from pyfasst_amd import _lib
    K, M = a.shape
    N = b.shape[1]
    A = _store(a, max(lda, M))
    B = A if same else _store(b, max(ldb, N))
    C = np.full((max(M, 1), max(ldc, 1)), SENT)
    arm = ctypes.c_int(-1)
    st = _lib.lib.fasst_dgemm2_probe(0, M, N, K, _lib.dptr(A), lda, a_skew, _lib.dptr(B), ldb, b_skew,
                                     _lib.dptr(C), ldc, flat, ctypes.byref(arm))
    _stop_on_device_error(st)
    return st, C, arm.value


def _run_dgemm2(kind, variant, M, N, K, tight=False, seed=0):
    oa, sa, ob, sb, flat, arm_want = VARIANTS[variant]
    rng = np.random.default_rng([seed, M, N, K, int(kind == "exact")])
    draw = _ints if kind == "exact" else _gammas
    a, b = draw(rng, (K, M)), draw(rng, (K, N))
    what = "dgemm2 %s M %d N %d K %d tight %d %s" % (variant, M, N, K, tight, kind)
    st, C, arm = dgemm2_probe(a, b, _ld(M, oa, tight), sa, _ld(N, ob, tight), sb, N + 3, flat)
    assert st == OK, what
    assert arm == arm_want, what
    if kind == "exact":
        np.testing.assert_array_equal(C[:, :N], _exact_ref(a.T, b), err_msg=what)
    else:
        _assert_rounded(C[:, :N], a.T, b, what)
    _assert_sentinel(C[:, N:], what)
    return C


DG_M = (1, 8, 9, 63, 64, 65, 127, 128, 129, 257)
DG_N = (1, 2, 3, 127, 128, 129)
DG_K = (1, 7, 8, 9, 16, 17, 24, 25, 40, 1093)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("M", DG_M)
def test_dgemm2_m_sweep(variant, M):
    """Partial 8 / 16-row groups, the FULL / edge main loops and, for odd M
    under an even lda, the 16-byte load whose second half is the NaN pad."""
    _run_dgemm2("exact", variant, M, 130, 19)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("N", DG_N)
def test_dgemm2_n_sweep(variant, N):
    _run_dgemm2("exact", variant, 65, N, 19)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("K", DG_K)
def test_dgemm2_k_sweep(variant, K):
    """nch = ceil(K / BK) through 1, 2, 3, 4 and past NS for D2Prod (BK 16,
    NS 2) and D2Odd (BK 8, NS 4): the prologue issues min(nch, NS - 1) chunks
    and the counted vmcnt waits shorten with it.  K = 40 also runs rounded."""
    _run_dgemm2("exact", variant, 65, 130, K)
    if K == 40:
        _run_dgemm2("rounded", variant, 65, 130, K)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,M,N", [
    ("buf", 300, 520), ("flat", 300, 520),                                    # 3 x 5 tiles of 128 x 128
    ("a4_odd", 520, 300), ("b4_odd", 520, 300), ("a4b4_odd", 520, 300),       # 3 x 3 tiles of 256 x 128
    ("a4_skew", 520, 300), ("b4_skew", 520, 300), ("a4b4_skew", 520, 300)] +
    [(v, 129, 129) for v in sorted(VARIANTS)])                                # 4 / 2 tiles, fewer than 8
def test_dgemm2_tile_permutation(variant, M, N):
    """Tile counts that are no multiple of the 8 XCDs, and fewer than 8: a
    tile computed twice leaves another uncomputed, which shows as sentinel."""
    _run_dgemm2("exact", variant, M, N, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,M,N", [
    ("buf", 64, 130), ("flat", 64, 130), ("buf", 128, 128), ("flat", 128, 128), ("buf", 8, 2),
    ("flat", 8, 2), ("a4b4_odd", 65, 129), ("a4_odd", 65, 130), ("b4_odd", 64, 129),
    ("a4b4_skew", 64, 130)])
def test_dgemm2_tight_leading_dimensions(variant, M, N):
    """lda = M, ldb = N: the last row's last load ends with the operand (the
    raw-buffer resource's last byte on the BUF arm)."""
    for K in (5, 33):
        _run_dgemm2("exact", variant, M, N, K, tight=True)


@pytest.mark.gpu
def test_dgemm2_flat_matches_buf():
    """The two D2Prod arms differ in how a piece is addressed, not in what is
    summed: bit-identical on the exact operands."""
    for M, N, K in ((65, 130, 40), (129, 127, 1093), (300, 520, 24)):
        Cb = _run_dgemm2("exact", "buf", M, N, K)
        Cf = _run_dgemm2("exact", "flat", M, N, K)
        assert np.array_equal(Cb.view(np.uint64), Cf.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("n,flat,arm_want", [(37, 0, A4B4), (38, 0, BUF), (38, 1, FLAT)])
def test_dgemm2_gram_of_one_buffer(n, flat, arm_want):
    """The NNLS Gram call dgemm2(n, n, m, A, n, A, n, G, n): both operands the
    same device buffer, every leading dimension tight."""
    m = 50
    for kind, draw in (("exact", _ints), ("rounded", _gammas)):
        a = draw(np.random.default_rng([n, flat, int(kind == "exact")]), (m, n))
        st, C, arm = dgemm2_probe(a, a, n, 0, n, 0, n, flat, same=True)
        assert st == OK and arm == arm_want
        if kind == "exact":
            np.testing.assert_array_equal(C, _exact_ref(a.T, a))
        else:
            _assert_rounded(C, a.T, a, "gram n %d flat %d" % (n, flat))


@pytest.mark.gpu
def test_dgemm2_refusals():
    from pyfasst_amd import _lib
    a, b = _ints(np.random.default_rng(0), (6, 10)), _ints(np.random.default_rng(1), (6, 12))
    # M = 0
    st, C, _ = dgemm2_probe(a[:, :0], b, 10, 0, 12, 0, 12, 0)
    assert st == ERR_SHAPE and "dgemm2" in _lib.last_error()
    # lda < M
    st, C, _ = dgemm2_probe(a, b, 9, 0, 12, 0, 12, 0)
    assert st == ERR_SHAPE and "dgemm2" in _lib.last_error()
    _assert_sentinel(C, "lda < M")
    # ldc < N
    st, C, _ = dgemm2_probe(a, b, 10, 0, 12, 0, 11, 0)
    assert st == ERR_SHAPE and "dgemm2" in _lib.last_error()
    _assert_sentinel(C, "ldc < N")


@pytest.mark.gpu
def test_dgemm2_cases_cover_the_five_arms():
    """Every arm is the asserted arm of some variant, and every variant runs
    in all three sweeps."""
    arms = {v[5] for v in VARIANTS.values()}
    assert arms == {BUF, FLAT, B4, A4, A4B4}
    # each 4-byte arm is reached both ways: odd leading dimension, skewed base
    for arm in (A4, B4, A4B4):
        how = {(bool(v[0] or v[2]), bool(v[1] or v[3])) for v in VARIANTS.values() if v[5] == arm}
        assert how == {(True, False), (False, True)}
    print("gemm-direct coverage: %d/5 dgemm2 arms" % len(arms))
