// FP64 MFMA GEMM host side: split-K planning, launch and the fixed-order
// slab reduction.  Explicit instantiations cover the operand forms the NMF
// and SIMM updates use.
#include "fasst_gemm.h"
#include "fasst_dgemm2.h"

#include <algorithm>

namespace fasst {

__global__ void k_gemm_reduce(const double *__restrict__ part, int nz, size_t slab,
                              double *__restrict__ out, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int z = 0; z < nz; ++z) s += part[z * slab + i];
    out[i] = s;
  }
}

// tile shape per operand count: a WG_M x (4 / WG_M) wave grid of WT_M x WT_N
// MFMA tiles per wave per operand, at most 16 accumulators per wave.  The
// R = 40 accompaniment GEMMs (M or N <= 48) take a 48-wide single-wave strip
// so only the 40 -> 48 pad of the MFMA rows is wasted.
struct TileShape {
  int wgm, wtm, wtn;
};
static TileShape tile_shape(int M, int N, int NB) {
  if (NB == 1) {
    if (M <= 48) return {1, 3, 2};
    if (N <= 48) return {4, 2, 3};
    return {2, 4, 4};
  }
  if (NB == 2) {
    if (M <= 48) return {1, 3, 2};
    if (M <= 64) return {2, 2, 4};
    return {2, 4, 2};
  }
  if (M <= 48) return {1, 3, 1};
  return {2, 2, 2};
}

static void tile_dims(const TileShape &t, int &BM, int &BN) {
  BM = 16 * t.wgm * t.wtm;
  BN = 16 * (4 / t.wgm) * t.wtn;
}

// split K until the grid holds >= 1024 blocks (4 per CU), chunks >= 64
GemmPlan gemm_plan(int M, int N, int K, int NB) {
  GemmPlan p;
  int BM, BN;
  tile_dims(tile_shape(M, N, NB), BM, BN);
  const long tiles = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int nz = 1;
  while (tiles * nz < 1024 && K / (nz * 2) >= 64) nz *= 2;
  p.kchunk = ((K + nz - 1) / nz + kGBK - 1) / kGBK * kGBK;
  p.nz = (K + p.kchunk - 1) / p.kchunk;
  if (p.nz < 1) p.nz = 1;
  return p;
}

template <bool TA, bool TB, int NB, int WGM, int WTM, int WTN>
static int launch_gemm(hipStream_t s, const GemmArgs &g, int nz) {
  constexpr int BM = 16 * WGM * WTM, BN = 16 * (4 / WGM) * WTN;
  const size_t smem = 2 * (size_t)kGBK * (gpitch(BM) + NB * gpitch(BN)) * sizeof(double);
  // the dynamic-LDS limit is a per-device attribute: set it before every
  // launch (a host-side call of a few us) so that a second device, or a
  // concurrent context, never launches before it holds
  if (smem > 64 * 1024)
    FASST_HIP(hipFuncSetAttribute((const void *)k_gemm<TA, TB, NB, WGM, WTM, WTN>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, nz);
  k_gemm<TA, TB, NB, WGM, WTM, WTN><<<grid, 256, smem, s>>>(g);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// dispatch to the instantiations tile_shape can return for this NB
template <bool TA, bool TB, int NB>
static int launch_shape(hipStream_t s, const GemmArgs &g, int nz) {
  const TileShape t = tile_shape(g.M, g.N, NB);
  if constexpr (NB == 1) {
    if (t.wgm == 1) return launch_gemm<TA, TB, NB, 1, 3, 2>(s, g, nz);
    if (t.wgm == 4) return launch_gemm<TA, TB, NB, 4, 2, 3>(s, g, nz);
    return launch_gemm<TA, TB, NB, 2, 4, 4>(s, g, nz);
  } else if constexpr (NB == 2) {
    if (t.wgm == 1) return launch_gemm<TA, TB, NB, 1, 3, 2>(s, g, nz);
    if (t.wtm == 2) return launch_gemm<TA, TB, NB, 2, 2, 4>(s, g, nz);
    return launch_gemm<TA, TB, NB, 2, 4, 2>(s, g, nz);
  } else {
    if (t.wgm == 1) return launch_gemm<TA, TB, NB, 1, 3, 1>(s, g, nz);
    return launch_gemm<TA, TB, NB, 2, 2, 2>(s, g, nz);
  }
}

template <bool TA, bool TB, int NB>
int gemm(hipStream_t s, const double *A, int lda, const double *const *B, int ldb, double *const *C,
         int ldc, int M, int N, int K, double *work, int *nz_ran) {
  GemmPlan p = gemm_plan(M, N, K, NB);
  const bool split = p.nz > 1 && work;
  if (split && ldc != N) {  // split-K outputs must be dense: refuse before any launch
    set_error("gemm: split-K (nz %d) needs ldc == N (ldc %d, N %d)", p.nz, ldc, N);
    return FASST_ERR_SHAPE;
  }
  if (nz_ran) *nz_ran = split ? p.nz : 1;
  GemmArgs g;
  g.A = A;
  g.lda = lda;
  g.ldb = ldb;
  g.M = M;
  g.N = N;
  g.K = K;
  g.kchunk = p.kchunk;
  if (!split) {
    g.kchunk = K;
    g.ldc = ldc;
    g.slab = 0;
    for (int b = 0; b < NB; ++b) {
      g.B[b] = B[b];
      g.C[b] = C[b];
    }
    return launch_shape<TA, TB, NB>(s, g, 1);
  }
  // split-K into work slabs laid out [NB][nz][M][N] (ldc = N)
  const size_t slab = (size_t)M * N;
  g.ldc = N;
  g.slab = slab;
  for (int b = 0; b < NB; ++b) {
    g.B[b] = B[b];
    g.C[b] = work + (size_t)b * p.nz * slab;
  }
  int st = launch_shape<TA, TB, NB>(s, g, p.nz);
  if (st) return st;
  for (int b = 0; b < NB; ++b) {
    k_gemm_reduce<<<(int)std::min<size_t>((slab + 255) / 256, 4096), 256, 0, s>>>(
        work + (size_t)b * p.nz * slab, p.nz, slab, C[b], slab);
    FASST_LAUNCH_CHECK();
  }
  return FASST_OK;
}

// Large plain products on k_dgemm2 (fasst_dgemm2.h) in its product shapes
// (D2Prod, D2Odd).  The dynamic-LDS limit is a per-device attribute: set
// before every launch.
template <class CF, bool A4, bool B4, bool BUF = false>
static int launch_dgemm2(hipStream_t s, Dgemm2Args g) {
  g.mt = (g.M + CF::BM - 1) / CF::BM;
  g.nt = (g.N + CF::BN - 1) / CF::BN;
  FASST_HIP(hipFuncSetAttribute((const void *)k_dgemm2<CF, A4, B4, BUF>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)CF::smem));
  k_dgemm2<CF, A4, B4, BUF><<<g.mt * g.nt, CF::NT, CF::smem, s>>>(g);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// dgemm2's argument check (also what fasst_dgemm2_probe sizes its buffers by)
static int dgemm2_check(int M, int N, int K, int lda, int ldb, int ldc) {
  if (M <= 0 || N <= 0 || K <= 0 || lda < M || ldb < N || ldc < N) {
    set_error("dgemm2: bad shape M %d N %d K %d (lda %d ldb %d ldc %d)", M, N, K, lda, ldb, ldc);
    return FASST_ERR_SHAPE;
  }
  return FASST_OK;
}

int dgemm2(hipStream_t s, int M, int N, int K, const double *A, int lda, const double *B, int ldb,
           double *C, int ldc, bool allow_buf, int *arm) {
  if (int st = dgemm2_check(M, N, K, lda, ldb, ldc)) return st;
  Dgemm2Args g{};
  g.A = A;
  g.B = B;
  g.C = C;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  const bool a16 = lda % 2 == 0 && ((uintptr_t)A & 15) == 0;
  const bool b16 = ldb % 2 == 0 && ((uintptr_t)B & 15) == 0;
  // raw-buffer LDS-DMA pieces (operands within 2 GB: 32-bit byte offsets);
  // the stereo SIMM iteration 9.19 -> 8.80 ms against the flat-address form
  const bool fits = (size_t)K * lda * sizeof(double) < (1ull << 31) &&
                    (size_t)K * ldb * sizeof(double) < (1ull << 31);
  const int which = a16 && b16 ? (fits && allow_buf ? kD2ArmProdBuf : kD2ArmProdFlat)
                               : (a16 ? kD2ArmOddB4 : (b16 ? kD2ArmOddA4 : kD2ArmOddA4B4));
  if (arm) *arm = which;
  switch (which) {
    case kD2ArmProdBuf: return launch_dgemm2<D2Prod, false, false, true>(s, g);
    case kD2ArmProdFlat: return launch_dgemm2<D2Prod, false, false>(s, g);
    case kD2ArmOddB4: return launch_dgemm2<D2Odd, false, true>(s, g);
    case kD2ArmOddA4: return launch_dgemm2<D2Odd, true, false>(s, g);
    default: return launch_dgemm2<D2Odd, true, true>(s, g);
  }
}

size_t gemm_workspace(int M, int N, int K, int NB) {
  GemmPlan p = gemm_plan(M, N, K, NB);
  return p.nz > 1 ? (size_t)NB * p.nz * M * N : 0;
}

template int gemm<false, false, 1>(hipStream_t, const double *, int, const double *const *, int,
                                   double *const *, int, int, int, int, double *, int *);
template int gemm<true, false, 1>(hipStream_t, const double *, int, const double *const *, int,
                                  double *const *, int, int, int, int, double *, int *);
template int gemm<true, false, 2>(hipStream_t, const double *, int, const double *const *, int,
                                  double *const *, int, int, int, int, double *, int *);
template int gemm<true, false, 4>(hipStream_t, const double *, int, const double *const *, int,
                                  double *const *, int, int, int, int, double *, int *);
template int gemm<false, true, 1>(hipStream_t, const double *, int, const double *const *, int,
                                  double *const *, int, int, int, int, double *, int *);
template int gemm<false, true, 2>(hipStream_t, const double *, int, const double *const *, int,
                                  double *const *, int, int, int, int, double *, int *);

// ---------------------------------------------------------------------------
// Test entry points (include/fasst_hip.h): the plan as the host computes it,
// and one gemm<> / dgemm2 call on caller-given operands with guarded buffers.
namespace {

// bit pattern of the guard tails: a finite double no product here computes
constexpr unsigned long long kGuardBits = 0x4757415244454421ull;

// a device buffer of n payload doubles, `skew` doubles past the allocation's
// (16-byte aligned) base, followed by `tail` guard doubles
struct GuardBuf {
  DBuf<double> d;
  size_t n = 0, skew = 0, tail = 0;
  double *p() const { return d.p + skew; }
  int alloc(size_t count, size_t guard, size_t sk = 0) {
    n = count;
    skew = sk;
    tail = guard;
    int st = d.alloc_uninit(sk + count + guard);
    if (st) return st;
    std::vector<unsigned long long> g(sk + guard, kGuardBits);
    FASST_TRY(d.at(0, sk).put(g.data(), sk));   // (the guard words are as wide as a double)
    return d.at(sk + count, guard).put(g.data(), guard);
  }
  int upload(const double *h) { return d.at(skew, n).put(h, n); }
  int download(double *h) const { return d.at(skew, n).get(h, n); }
  // *ok &= every guard double still holds kGuardBits
  int intact(int *ok) const {
    std::vector<unsigned long long> g(skew + tail);
    FASST_TRY(d.at(0, skew).get(g.data(), skew));
    FASST_TRY(d.at(skew + n, tail).get(g.data() + skew, tail));
    for (unsigned long long v : g)
      if (v != kGuardBits) *ok = 0;
    return FASST_OK;
  }
};

struct ProbeStream {
  hipStream_t s = nullptr;
  int create() {
    FASST_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return FASST_OK;
  }
  ~ProbeStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

constexpr size_t kProbeTail = 512;  // guard doubles behind operands and outputs

}  // namespace

}  // namespace fasst

using namespace fasst;

extern "C" {

int fasst_gemm_plan(int M, int N, int K, int NB, int *nz, int *kchunk, int *wgm, int *wtm, int *wtn,
                    long long *work_doubles) {
  if (M < 1 || N < 1 || K < 1 || (NB != 1 && NB != 2 && NB != 4)) {
    set_error("fasst_gemm_plan: need M, N, K >= 1 and NB in {1, 2, 4} (M %d N %d K %d NB %d)", M, N,
              K, NB);
    return FASST_ERR_SHAPE;
  }
  const GemmPlan p = gemm_plan(M, N, K, NB);
  const TileShape t = tile_shape(M, N, NB);
  if (nz) *nz = p.nz;
  if (kchunk) *kchunk = p.kchunk;
  if (wgm) *wgm = t.wgm;
  if (wtm) *wtm = t.wtm;
  if (wtn) *wtn = t.wtn;
  if (work_doubles) *work_doubles = (long long)gemm_workspace(M, N, K, NB);
  return FASST_OK;
}

int fasst_gemm_probe(int device, int ta, int tb, int nb, int M, int N, int K, const double *A,
                     int lda, const double *B, int ldb, double *C, int ldc, int use_work,
                     int *nz_ran, int *guard_ok) {
  const bool with_work = use_work & 1, bcols = use_work & 2;
  if (M < 1 || N < 1 || K < 1 || !A || !B || !C || lda < (ta ? M : K) ||
      ldb < (tb ? K : (bcols ? nb * N : N)) || ldc < N || (use_work & ~3) || (bcols && tb) ||
      nb < 1 || nb > 4) {
    set_error("fasst_gemm_probe: bad arguments (ta %d tb %d nb %d M %d N %d K %d lda %d ldb %d "
              "ldc %d use_work %d)", ta, tb, nb, M, N, K, lda, ldb, ldc, use_work);
    return FASST_ERR_SHAPE;
  }
  typedef int (*gemm_fn)(hipStream_t, const double *, int, const double *const *, int,
                         double *const *, int, int, int, int, double *, int *);
  gemm_fn fn = nullptr;
  if (!ta && !tb && nb == 1) fn = gemm<false, false, 1>;
  if (ta && !tb && nb == 1) fn = gemm<true, false, 1>;
  if (ta && !tb && nb == 2) fn = gemm<true, false, 2>;
  if (ta && !tb && nb == 4) fn = gemm<true, false, 4>;
  if (!ta && tb && nb == 1) fn = gemm<false, true, 1>;
  if (!ta && tb && nb == 2) fn = gemm<false, true, 2>;
  if (!fn) {
    set_error("fasst_gemm_probe: gemm<%d, %d, %d> is not instantiated", ta != 0, tb != 0, nb);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard dg(device);
  const size_t na = (size_t)(ta ? K : M) * lda;
  const size_t nb1 = (size_t)(tb ? N : K) * ldb;      // one B operand (all of them with bcols)
  const size_t nbs = bcols ? nb1 : nb * nb1;
  const size_t nc1 = (size_t)M * ldc;
  const size_t nw = gemm_workspace(M, N, K, nb);
  GuardBuf dA, dB, dC, dW;
  ProbeStream ps;
  int st;
  if ((st = dA.alloc(na, kProbeTail)) || (st = dB.alloc(nbs, kProbeTail)) ||
      (st = dC.alloc(nb * nc1, kProbeTail)) || (st = dA.upload(A)) || (st = dB.upload(B)) ||
      (st = dC.upload(C)) || (st = ps.create()))
    return st;
  // the workspace, then a guard tail of one slab (M N doubles) at least
  if (with_work && (st = dW.alloc(nw, std::max((size_t)M * N, kProbeTail)))) return st;
  FASST_HIP(hipDeviceSynchronize());
  const double *Bs[4] = {nullptr, nullptr, nullptr, nullptr};
  double *Cs[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int b = 0; b < nb; ++b) {
    Bs[b] = dB.p() + (bcols ? (size_t)b * N : b * nb1);
    Cs[b] = dC.p() + b * nc1;
  }
  int ran = 0;
  st = fn(ps.s, dA.p(), lda, Bs, ldb, Cs, ldc, M, N, K, with_work ? dW.p() : nullptr, &ran);
  if (st) return st;
  FASST_HIP(hipStreamSynchronize(ps.s));
  if ((st = dC.download(C))) return st;
  int ok = 1;
  if ((st = dA.intact(&ok)) || (st = dB.intact(&ok)) || (st = dC.intact(&ok)) ||
      (with_work && (st = dW.intact(&ok))))
    return st;
  if (nz_ran) *nz_ran = ran;
  if (guard_ok) *guard_ok = ok;
  return FASST_OK;
}

int fasst_dgemm2_probe(int device, int M, int N, int K, const double *A, int lda, int a_skew,
                       const double *B, int ldb, int b_skew, double *C, int ldc, int flat, int *arm) {
  int st;
  if ((st = dgemm2_check(M, N, K, lda, ldb, ldc))) return st;
  if (!A || !B || !C || (a_skew & ~1) || (b_skew & ~1)) {
    set_error("fasst_dgemm2_probe: bad arguments (a_skew %d b_skew %d)", a_skew, b_skew);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard dg(device);
  const bool same = A == B && lda == ldb && a_skew == b_skew;   // one buffer as both operands
  GuardBuf dA, dB, dC;
  ProbeStream ps;
  // an odd skew + payload keeps the tail 16-byte aligned or not: either is a guard
  if ((st = dA.alloc((size_t)K * lda, kProbeTail, a_skew)) || (st = dA.upload(A)) ||
      (!same && ((st = dB.alloc((size_t)K * ldb, kProbeTail, b_skew)) || (st = dB.upload(B)))) ||
      (st = dC.alloc((size_t)M * ldc, kProbeTail)) || (st = dC.upload(C)) || (st = ps.create()))
    return st;
  FASST_HIP(hipDeviceSynchronize());
  int which = -1;
  st = dgemm2(ps.s, M, N, K, dA.p(), lda, same ? dA.p() : dB.p(), ldb, dC.p(), ldc, !flat, &which);
  if (st) return st;
  FASST_HIP(hipStreamSynchronize(ps.s));
  if ((st = dC.download(C))) return st;
  int ok = 1;
  if ((st = dA.intact(&ok)) || (!same && (st = dB.intact(&ok))) || (st = dC.intact(&ok))) return st;
  if (!ok) {
    set_error("fasst_dgemm2_probe: a guard tail was overwritten");
    return FASST_ERR_DEVICE;
  }
  if (arm) *arm = which;
  return FASST_OK;
}

}  // extern "C"
