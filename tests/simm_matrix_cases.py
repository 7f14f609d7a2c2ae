"""The SIMM kernel matrix: the host dispatch of pyfasst_amd/csrc/fasst_simm.hip
restated (simm_arms), one case per reachable instantiation (CASES), and the
float64 / longdouble oracle runs the tests compare with (oracle_run).

Importable without a GPU: test_simm_matrix_cases.py checks the table on the
CPU, test_gpu_simm_matrix.py runs it on the MI355X.
"""
import collections
import functools

import numpy as np

import simm_ref

# ---------------------------------------------------------------- the restated dispatch
# fasst_simm.hip's constants, pinned to the source by
# test_simm_matrix_cases.test_dispatch_constants_match_the_source
K_MAX = 8            # kSimmKmax: simm_create refuses K above it
KM_SMALL = 4         # kdispatch: KM = 4 for K <= 4, else KM = 8 (= K_MAX)
SM_RMAX = 48         # kSmRmax, and the `R > 48` tests of wmt_xy / xy_hmt
SM_BODIES = (8, 16, 24, 32, 40, 48)   # the SM_CASE list of refresh_sm
SM_ROWS = 64         # kSmRows: bins per k_simm_sm block
WMT_MAX_CHUNK = 512  # kWmtMaxChunk: bins per k_simm_wmt_xy block
SPLIT_FULL = 0.95    # round_split: a last round this full is taken at once
V16_RULE = "N % 2 == 0 && sp.kchunk % 2 == 0"
DEFAULT_SLOTS = 512  # two resident blocks per CU, 256 CUs


def round_split(units, lo, hi, slots):
    """round_split: the smallest nz in [lo, hi] whose last round of `slots`
    resident blocks is >= 95% full, else the fullest."""
    hi = max(lo, hi)
    best, beff = lo, 0.0
    for nz in range(lo, hi + 1):
        b = units * nz
        rounds = (b + slots - 1) // slots
        eff = float(b) / float(rounds * slots)
        if eff >= SPLIT_FULL:
            return nz
        if eff > beff:
            beff, best = eff, nz
    return best


def wmt_split(F, N, slots=DEFAULT_SLOTS):
    """wmt_split: (nz, kchunk), the bin slabs of k_simm_wmt_xy."""
    bx = (N + 63) // 64
    by_chunk = (F + WMT_MAX_CHUNK - 1) // WMT_MAX_CHUNK
    lo = max(max(1, by_chunk), min(16, (2 * slots + bx - 1) // bx))
    nz = round_split(bx, lo, max(lo, min(16, F // 64)), slots)
    nz = max(nz, by_chunk)
    kchunk = ((F + nz - 1) // nz + 15) // 16 * 16
    return (F + kchunk - 1) // kchunk, kchunk


def hmt_split(F, N, slots=DEFAULT_SLOTS):
    """hmt_split: (nz, kchunk), the frame slabs of k_simm_xy_hmt."""
    by = (F + 63) // 64
    hi = max(1, min(32, N // 256))
    nz = round_split(by, min(hi, max(1, slots // (2 * by))), hi, slots)
    kchunk = ((N + nz - 1) // nz + 31) // 32 * 32
    return (N + kchunk - 1) // kchunk, kchunk


def simm_arms(F, N, K, R, stereo, update_hgamma, compute_error, gemm_kind=0,
              slots=DEFAULT_SLOTS):
    """The instantiations and host branches one simm_iteration launches.
    Restates fasst_simm.hip:
      simm_create     K <= kSimmKmax; mono needs R == 1 or R == N;
      simm_run / SIMM.py of the package
                      mono always updates HGAMMA and never fills recoError,
                      so k_is_partial runs in its stereo form only;
      kdispatch       KM = 4 for K <= 4, else 8, for k_simm_numden,
                      k_hphi_partial, k_hgamma_rows (update_hgamma),
                      k_is_partial (compute_error), k_alpha_partial (stereo),
                      k_simm_wmt_xy and k_simm_xy_hmt;
      FASST_SIMM_GEMM the NF0-sized products on k_dgemm2 (0) or k_gemm (2);
      R > 48          wmt_xy / xy_hmt / refresh_sm leave the fused kernels:
                      materialise_hat + k_simm_xy + the general GEMM
                      (gemm<.., 4> stereo, <.., 2> mono), refresh_sm_gemm;
      refresh_sm      k_simm_sm<RM>, RM = R rounded up to 8;
      xy_hmt          V16 = N even and an even frame chunk;
      wmt_split / hmt_split
                      one slab (nz1) or several (nzN, k_slab_reduce sums > 1);
      c->pend         SF0's column scale, pending after the HPHI update and
                      again after the HGAMMA update, is applied by the next
                      kernel that streams SF0: k_simm_wmt_xy (HM step), then
                      k_simm_xy_hmt (WM step, only when HGAMMA was updated),
                      or k_simm_refresh inside materialise_hat at R > 48;
      mono WM step    HM *= sumWM by row (R == 1) or by column (R == N).
    ST is written 1 / 0.  A change to those functions must be restated here;
    the completeness test then says which arms lost their case."""
    if not 1 <= K <= K_MAX:
        raise ValueError("simm_create: K = %d" % K)
    st = int(bool(stereo))
    if not st:
        if R != 1 and R != N:
            raise ValueError("mono SIMM: R must be 1 or N")
        update_hgamma, compute_error = True, False
    km = KM_SMALL if K <= KM_SMALL else K_MAX
    arms = {"numden<%d,%d>" % (st, km), "hphi_partial<%d,%d>" % (st, km),
            "nf0_dgemm2" if gemm_kind == 0 else "nf0_kgemm"}
    if update_hgamma:
        arms.add("hgamma_rows<%d,%d>" % (st, km))
    if compute_error:
        arms.add("is_partial<%d,%d>" % (st, km))
    if st:
        arms.add("alpha_partial<%d>" % km)
    else:
        arms.add("hm_rowscale" if R == 1 else "hm_colscale")
    if R > SM_RMAX:
        arms |= {"wmt_gemm<%d>" % st, "xy_gemm<%d>" % st, "sm_gemm<%d>" % st,
                 "pend@materialise"}
        return arms
    wz, _ = wmt_split(F, N, slots)
    hz, hchunk = hmt_split(F, N, slots)
    v16 = int(N % 2 == 0 and hchunk % 2 == 0)
    arms |= {"wmt_xy<%d,%d>" % (st, km), "xy_hmt<%d,%d,%d>" % (st, km, v16),
             "sm<%d>" % ((R + 7) // 8 * 8),
             "wmt_nz1" if wz == 1 else "wmt_nzN", "hmt_nz1" if hz == 1 else "hmt_nzN",
             "pend@wmt"}
    if update_hgamma:
        arms.add("pend@hmt")
    return arms


def reachable_arms():
    """Every name simm_arms can return, built from the rules above (not from
    the cases)."""
    full = {"nf0_dgemm2", "nf0_kgemm", "hm_rowscale", "hm_colscale",
            "pend@wmt", "pend@hmt", "pend@materialise",
            "wmt_nz1", "wmt_nzN", "hmt_nz1", "hmt_nzN"}
    full |= {"sm<%d>" % rm for rm in SM_BODIES}
    for st in (0, 1):
        full |= {"wmt_gemm<%d>" % st, "xy_gemm<%d>" % st, "sm_gemm<%d>" % st}
        for km in (KM_SMALL, K_MAX):
            full |= {"numden<%d,%d>" % (st, km), "hphi_partial<%d,%d>" % (st, km),
                     "hgamma_rows<%d,%d>" % (st, km), "wmt_xy<%d,%d>" % (st, km)}
            full |= {"xy_hmt<%d,%d,%d>" % (st, km, v) for v in (0, 1)}
    for km in (KM_SMALL, K_MAX):
        full |= {"is_partial<1,%d>" % km, "alpha_partial<%d>" % km}
    return full


# ---------------------------------------------------------------- the cases
# shape = (F, N, NF0, P, K, R); NF0 and P are odd (or N is) wherever nothing
# else is asked of them, so that the rows of WF0, WGAMMA, HF0, HPHI are not
# 16-byte aligned
Case = collections.namedtuple(
    "Case", "id shape stereo hgamma gemm data_seed init_seed zero iters")


def _case(id, shape, stereo=True, hgamma=True, gemm=0, data_seed=5, init_seed=7, zero=None,
          iters=(1, 2)):
    return Case(id, shape, stereo, hgamma, gemm, data_seed, init_seed, zero, iters)


CASES = [
    # stereo, KM x V16 at R <= 48 (K = 4, 5, 8; N = 66, 67), each on another
    # k_simm_sm<RM> body: R = 5, 8 | 9 | 17, 24 | 25 | 33 | 41, 48
    _case("st-K4-N66-R5", (70, 66, 19, 5, 4, 5)),
    _case("st-K4-N67-R8", (70, 67, 19, 5, 4, 8)),
    _case("st-K5-N66-R9", (70, 66, 19, 5, 5, 9)),
    _case("st-K5-N67-R17", (70, 67, 19, 5, 5, 17)),
    _case("st-K8-N66-R24", (70, 66, 19, 5, 8, 24)),
    _case("st-K8-N67-R25", (70, 67, 19, 5, 8, 25)),
    _case("st-K8-N66-R33", (70, 66, 21, 3, 8, 33)),
    _case("st-K4-N67-R41", (70, 67, 19, 5, 4, 41)),
    _case("st-K5-N66-R48", (70, 66, 19, 5, 5, 48)),
    # R > 48: materialised X, Y and the general GEMM
    _case("st-K8-N67-R49", (70, 67, 19, 5, 8, 49)),
    # updateHGAMMA=False: the WM products find no pending scale (R = 20), the
    # second materialise_hat none (R = 49).  Mono SIMM has no such argument
    # (as in the reference) and always updates HGAMMA.
    _case("st-K8-N66-R20-fixedHG", (70, 66, 19, 5, 8, 20), hgamma=False),
    _case("st-K4-N66-R49-fixedHG", (70, 66, 19, 5, 4, 49), hgamma=False),
    # mono, R = 1 (row scale): KM x V16
    _case("mono-K4-N66-R1", (70, 66, 19, 5, 4, 1), stereo=False, data_seed=6, init_seed=8),
    _case("mono-K3-N67-R1", (70, 67, 19, 5, 3, 1), stereo=False, data_seed=6, init_seed=8),
    _case("mono-K8-N66-R1", (70, 66, 19, 5, 8, 1), stereo=False, data_seed=6, init_seed=8),
    _case("mono-K7-N67-R1", (70, 67, 19, 5, 7, 1), stereo=False, data_seed=6, init_seed=8),
    # mono, R = N (column scale): fused at N = 40 and 47, GEMM path at N = 66
    _case("mono-K4-N40-RN", (70, 40, 19, 5, 4, 40), stereo=False, data_seed=6, init_seed=8),
    _case("mono-K8-N47-RN", (70, 47, 19, 5, 8, 47), stereo=False, data_seed=6, init_seed=8),
    _case("mono-K5-N66-RN", (70, 66, 19, 5, 5, 66), stereo=False, data_seed=6, init_seed=8),
    # frame slabs: hmt_split gives nz = 2 with chunks of 288 frames, the last
    # one ragged (226 / 227 frames, the latter odd)
    _case("st-slabN514-K8-R9", (130, 514, 21, 4, 8, 9)),
    _case("st-slabN515-K4-R40", (130, 515, 21, 4, 4, 40)),
    _case("mono-slabN515-K5-R1", (130, 515, 21, 4, 5, 1), stereo=False, data_seed=6,
          init_seed=8),
    # bin slabs at F > kWmtMaxChunk (11 chunks of 48 bins, the last of 40)
    _case("st-F520-K4-R10", (520, 66, 19, 5, 4, 10)),
    # small bin counts: F = 7 is the one-slab form of k_simm_wmt_xy (F <= 16),
    # F = 17 two slabs of 16 + 1; N = 31 is less than one 64-frame tile
    _case("st-F7-K8-R5", (7, 66, 19, 5, 8, 5)),
    _case("st-F17-N31-K4-R12", (17, 31, 9, 3, 4, 12)),
    _case("mono-F7-K2-R1", (7, 33, 5, 3, 2, 1), stereo=False, data_seed=6, init_seed=8),
    # the 256-frame walker block: one block less a frame, full, plus a frame
    _case("st-N255-K4-R7", (70, 255, 19, 5, 4, 7)),
    _case("st-N256-K8-R16", (70, 256, 19, 5, 8, 16)),
    _case("st-N257-K5-R30", (70, 257, 19, 5, 5, 30)),
    # FASST_SIMM_GEMM=2: the NF0-sized products on the generic k_gemm
    _case("st-kgemm-K5-N67-R17", (70, 67, 19, 5, 5, 17), gemm=2),
    _case("mono-kgemm-K4-N66-R1", (70, 66, 19, 5, 4, 1), stereo=False, gemm=2, data_seed=6,
          init_seed=8),
]

# an all-zero frame and an all-zero bin in both channels: the oracle's
# parameters stay finite, recoError is infinite where it is filled
ZERO_CASE = _case("st-zero-frame3-bin7", (70, 66, 19, 5, 4, 20), zero=(3, 7), iters=(3,))

BY_ID = {c.id: c for c in CASES + [ZERO_CASE]}

ST_NAMES = ('alphaR', 'alphaL', 'HGAMMA', 'HPHI', 'HF0', 'betaR', 'betaL', 'HM', 'WM',
            'recoError')
MONO_NAMES = ('HGAMMA', 'HPHI', 'HF0', 'HM', 'WM', 'recoError')


def names(case):
    return ST_NAMES if case.stereo else MONO_NAMES


def case_arms(case, slots=DEFAULT_SLOTS):
    F, N, _, _, K, R = case.shape
    return simm_arms(F, N, K, R, case.stereo, case.hgamma, True, case.gemm, slots)


@functools.lru_cache(maxsize=None)
def data(shape, seed, zero=None):
    """(SXR, SXL, WF0, WGAMMA), float64, read-only."""
    F, N, NF0, P = shape[:4]
    rs = np.random.RandomState(seed)
    out = [rs.gamma(0.8, 1.0, size=(F, N)), rs.gamma(0.8, 1.0, size=(F, N)),
           rs.gamma(1.0, 1.0, size=(F, NF0)), rs.gamma(1.0, 1.0, size=(F, P))]
    if zero is not None:
        frame, fbin = zero
        for SX in out[:2]:
            SX[:, frame] = 0.0
            SX[fbin, :] = 0.0
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_run(case_id, n_iter, dtype_name):
    """oracle/simm_ref on the case's data in float64 or longdouble, seeded as
    the product's run is; computed once per process, returned read-only.
    (gemm is a device setting: cases that differ only in it share a run.)"""
    case = BY_ID[case_id]
    key = case._replace(id="", gemm=0)
    return _oracle_run(key, n_iter, dtype_name)


@functools.lru_cache(maxsize=None)
def _oracle_run(case, n_iter, dtype_name):
    dt = np.dtype(dtype_name)
    SXR, SXL, WF0, WG = [a.astype(dt) for a in data(case.shape, case.data_seed, case.zero)]
    K, R = case.shape[4:]
    np.random.seed(case.init_seed)
    with np.errstate(divide='ignore', invalid='ignore'):
        if case.stereo:
            out = simm_ref.stereo_simm(SXR, SXL, WF0, WG, K, R, numberOfIterations=n_iter,
                                       updateHGAMMA=case.hgamma, computeError=True)
        else:
            out = simm_ref.simm(SXR, WF0, WG, K, R, numberOfIterations=n_iter)
    out = tuple(np.asarray(a) for a in out)
    for a in out:
        a.setflags(write=False)
    return out
