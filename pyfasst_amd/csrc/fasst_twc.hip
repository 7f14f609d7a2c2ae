// Discrete-state time weights: TW_constr 'GSMM' / 'SHMM' of
// update_spectral_components (audioModel.py:1728-1928), one active state per
// frame.  Two kernels per iteration, reached only when some source carries a
// constraint (fasst_set_tw_constr):
//   k_tw_statediv  per state k the single-state weight update of TW_all[k]
//                  and the Itakura-Saito divergence to hat_W at the new weight
//                  (:1773-1832);
//   k_tw_decode    the state sequence (GSMM argmin :1840-1847, SHMM Viterbi
//                  :1853-1885), the one-hot TW (:1895-1900) and the prior /
//                  transition counts (:1902-1924).
#include "fasst_ctx.h"
#include "fasst_device.h"
#include "fasst_twc.h"

#include <cmath>

namespace fasst {

constexpr int kTdFrames = 4;     // frames per k_tw_statediv block, one per wave
constexpr int kTvThreads = 128;  // k_tw_decode: one lane per state (K <= 128)
constexpr int kTvChunk = 16;     // frames of ISdiv staged per LDS refill

struct TDArgs {
  const double *TW, *Wkf_old, *Wkf_new, *rho;
  double *twall, *isdiv;
  int F, T, Fp, Tp, KP;
  int K[kMaxJ], kind[kMaxJ];
  int is_hatw;   // the plane holds hat_W itself (the multi-component path's
                 // k_multi_prep rewrote rho in place), not rho
  double omega;
  const int *halt;
};

// One block per (tile of kTdFrames frames, source), wave w owns frame
// t0 + w.  hat_W of the tile is recovered once from the E-step's plane,
// hat_W = rho * max(V_old, eps) with V_old = W_old . TW of the pre-update
// factors (as k_tw_contract does; is_hatw: the plane already is hat_W), kept
// in LDS and reused by the K states.
// Per state the basis column Wb = (FB.FW)[:, k] of the updated factors is
// staged in LDS; a lane sums its bins f = lane, lane + 64, ... in order and
// the wave butterfly finishes: the order does not depend on the grid.
//   V   = max(Wb TW_all[k, t], eps)
//   num = sum_f Wb hat_W / max(V^2, eps),  den = sum_f Wb / V
//   TW_all[k, t] *= (num / max(den, eps))^omega
//   ISdiv[k, t] = sum_f (r - log(max(r, eps)) - 1),  r = hat_W / max(Wb TW_all[k, t], eps)
__global__ __launch_bounds__(64 * kTdFrames) void k_tw_statediv(const TDArgs a) {
  HALT_GUARD(a.halt);
  const int j = blockIdx.y;
  if (!a.kind[j]) return;
  extern __shared__ __align__(16) double td_sm[];
  double *hw = td_sm;                       // [kTdFrames][Fp]
  double *wb = td_sm + kTdFrames * a.Fp;    // [Fp]
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = blockIdx.x * kTdFrames + w;
  const bool tin = t < a.T;
  const int K = a.K[j];
  const size_t jk = (size_t)j * a.KP;
  double *hwt = hw + (size_t)w * a.Fp;
  if (tin) {
    const double *rho = a.rho + ((size_t)j * a.Tp + t) * a.Fp;
    if (a.is_hatw) {
      for (int f = lane; f < a.F; f += 64) hwt[f] = rho[f];
    } else {
      for (int f = lane; f < a.F; f += 64) {
        double v = 0.0;
        for (int k = 0; k < K; ++k)
          v += a.Wkf_old[(jk + k) * a.Fp + f] * a.TW[(jk + k) * a.Tp + t];
        hwt[f] = rho[f] * fmax(v, kEps);
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    __syncthreads();   // the previous column's readers are done
    for (int f = threadIdx.x; f < a.F; f += blockDim.x) wb[f] = a.Wkf_new[(jk + k) * a.Fp + f];
    __syncthreads();
    if (!tin) continue;   // (wave-uniform; the barriers above stay block-wide)
    const size_t o = (jk + k) * a.Tp + t;
    const double a0 = a.twall[o];
    double num = 0.0, den = 0.0;
    for (int f = lane; f < a.F; f += 64) {
      const double wv = wb[f], v = fmax(wv * a0, kEps);
      num += wv * (hwt[f] / fmax(v * v, kEps));
      den += wv * (1.0 / v);
    }
    num = wave_sum(num);
    den = wave_sum(den);
    const double ratio = num / fmax(den, kEps);
    const double a1 = a0 * (a.omega == 1.0 ? ratio : pow(ratio, a.omega));
    double is = 0.0;
    for (int f = lane; f < a.F; f += 64) {
      const double r = hwt[f] / fmax(wb[f] * a1, kEps);
      is += r - log(fmax(r, kEps)) - 1.0;
    }
    is = wave_sum(is);
    if (lane == 0) {
      a.twall[o] = a1;
      a.isdiv[o] = is;
    }
  }
}

struct TVArgs {
  double *TW, *dp;
  const double *twall, *isdiv;
  int *ante, *state;
  int T, Tp, KP;
  int K[kMaxJ], kind[kMaxJ], dpfree[kMaxJ];
  double log1k[kMaxJ];   // log(1 / K) of the Viterbi's initial value (:1853-1856)
  const int *halt;
};

static size_t decode_lds(int K) {
  return ((size_t)K * K + 2 * (size_t)K + (size_t)K * (kTvChunk + 1)) * sizeof(double);
}

// One block per source, lane s = state s.  SHMM: the recursion of :1860-1874
// as written (acc += tmp[ante] + ISdiv, then acc -= min(acc)), the argmin over
// the previous state a loop per lane in ascending order (ties: lowest index),
// ante [T][KP] int32 in device memory, row 0 zero as the reference leaves it;
// backtracking reads ante[state[n]][n - 1] (:1881-1885), staged through LDS
// in chunks of 2 K frames.  Then TW = one-hot of TW_all and, with a free
// prior, the state / transition frequencies.
__global__ __launch_bounds__(kTvThreads) void k_tw_decode(const TVArgs a) {
  HALT_GUARD(a.halt);
  const int j = blockIdx.x, kind = a.kind[j];
  if (!kind) return;
  extern __shared__ __align__(16) double tv_sm[];
  const int K = a.K[j], s = threadIdx.x, T = a.T, KP = a.KP, Tp = a.Tp;
  double *L = tv_sm;                   // [K][K] log(P + eps); later ante chunks / counts
  double *raw = tv_sm + (size_t)K * K;   // [2][K]
  double *isl = raw + 2 * K;           // [K][kTvChunk + 1]
  const double *is = a.isdiv + (size_t)j * KP * Tp;
  const double *twall = a.twall + (size_t)j * KP * Tp;
  double *TW = a.TW + (size_t)j * KP * Tp;
  double *dp = a.dp + (size_t)j * KP * KP;
  int *state = a.state + (size_t)j * Tp;
  int *ante = a.ante + (size_t)j * Tp * KP;
  int *al = reinterpret_cast<int *>(L);
  if (kind == 1) {
    if (s < K) raw[s] = log(dp[s] + kEps);
    __syncthreads();
    for (int t = s; t < T; t += kTvThreads) {
      int best = 0;
      double bv = is[t] - raw[0];
      for (int k = 1; k < K; ++k) {
        const double v = is[(size_t)k * Tp + t] - raw[k];
        if (v < bv) {
          bv = v;
          best = k;
        }
      }
      state[t] = best;
    }
  } else {
    for (int i = s; i < K * K; i += kTvThreads) L[i] = log(dp[(size_t)(i / K) * KP + i % K] + kEps);
    double acc = 0.0, m = 0.0;
    if (s < K) {
      acc = is[(size_t)s * Tp] - a.log1k[j];
      raw[s] = acc;
      ante[s] = 0;
    }
    __syncthreads();
    for (int n = 1; n < T; ++n) {
      const int c = (n - 1) % kTvChunk;
      if (c == 0) {   // frames n .. n + kTvChunk - 1 of ISdiv (the last barrier fences the old chunk)
        for (int i = s; i < K * kTvChunk; i += kTvThreads) {
          const int k = i / kTvChunk, q = i % kTvChunk;
          isl[k * (kTvChunk + 1) + q] = n + q < T ? is[(size_t)k * Tp + n + q] : 0.0;
        }
        __syncthreads();
      }
      const double *prev = raw + ((n - 1) & 1) * K;
      double *cur = raw + (n & 1) * K;
      if (s < K) {
        int bp = 0;
        double bv = (prev[0] - m) - L[s];
        for (int p = 1; p < K; ++p) {
          const double v = (prev[p] - m) - L[(size_t)p * K + s];
          if (v < bv) {
            bv = v;
            bp = p;
          }
        }
        ante[(size_t)n * KP + s] = bp;
        acc = acc + (bv + isl[s * (kTvChunk + 1) + c]);
        cur[s] = acc;
      }
      __syncthreads();
      if (s < K) {
        double mm = cur[0];
        for (int p = 1; p < K; ++p) mm = fmin(mm, cur[p]);
        m = mm;
        acc -= m;
      }
    }
    double *fin = raw + (T & 1) * K;
    if (s < K) fin[s] = acc;
    __syncthreads();   // (also: every lane is past L, reused below)
    int st = 0;
    if (s == 0) {
      double bv = fin[0];
      for (int p = 1; p < K; ++p)
        if (fin[p] < bv) {
          bv = fin[p];
          st = p;
        }
      state[T - 1] = st;
    }
    const int CF = 2 * K;   // ante rows per chunk: 2 K rows of K int32 = the [K][K] doubles of L
    for (int hi = T - 1; hi > 0; hi -= CF) {
      const int lo = hi - CF > 0 ? hi - CF : 0;
      for (int i = s; i < (hi - lo) * K; i += kTvThreads) al[i] = ante[(size_t)(lo + i / K) * KP + i % K];
      __syncthreads();
      if (s == 0)
        for (int n = hi; n > lo; --n) {
          st = al[(n - 1 - lo) * K + st];
          state[n - 1] = st;
        }
      __syncthreads();
    }
  }
  __syncthreads();   // state[] of this block's thread(s) visible to the block
  for (int t = s; t < T; t += kTvThreads) {
    const int st = state[t];
    for (int k = 0; k < K; ++k)
      TW[(size_t)k * Tp + t] = k == st ? twall[(size_t)k * Tp + t] : 0.0;
  }
  if (!a.dpfree[j]) return;
  if (kind == 1) {
    if (s < K) {
      int cnt = 0;
      for (int t = 0; t < T; ++t) cnt += state[t] == s;
      dp[s] = (double)cnt * 1. / (double)T;
    }
  } else {
    for (int i = s; i < K * K; i += kTvThreads) al[i] = 0;
    __syncthreads();
    if (s < K) {
      int den = 0;
      for (int t = 0; t + 1 < T; ++t)
        if (state[t] == s) {
          ++den;
          ++al[s * K + state[t + 1]];
        }
      if (den)   // a state never left keeps its row (:1914)
        for (int q = 0; q < K; ++q) dp[(size_t)s * KP + q] = (double)al[s * K + q] / (double)den;
    }
  }
}

// TW_all on first use: every row = max_k TW[k, t] (:1744-1748)
__global__ void k_twall_init(const double *__restrict__ TW, double *__restrict__ twall, int K,
                             int T, int Tp) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  double m = TW[t];
  for (int k = 1; k < K; ++k) m = fmax(m, TW[(size_t)k * Tp + t]);
  for (int k = 0; k < K; ++k) twall[(size_t)k * Tp + t] = m;
}

constexpr size_t kLdsMax = 160 * 1024;   // LDS of one gfx950 CU

// hat_W of the frame tile and one basis column, every bin of both: a
// constrained source needs (kTdFrames + 1) Fp doubles <= 160 KB, F <= 4096
static size_t statediv_lds(const fasst_ctx *c) {
  return (size_t)(kTdFrames + 1) * c->Fp * sizeof(double);
}

static int twc_alloc(fasst_ctx *c) {
  int st;
  if (statediv_lds(c) > kLdsMax) {   // before anything is allocated
    set_error("TW_constr: a discrete-state TW holds %d frames of hat_W and a basis column in LDS, "
              "%zu bytes at F = %d (max %zu: F <= 4096)", kTdFrames, statediv_lds(c), c->F,
              kLdsMax);
    return FASST_ERR_UNSUPPORTED;
  }
  const size_t nkt = (size_t)c->J * c->KP * c->Tp;
  if (c->twall.n < nkt && (st = c->twall.alloc(nkt))) return st;
  if (c->isdiv.n < nkt && (st = c->isdiv.alloc(nkt))) return st;
  if (c->twante.n < nkt && (st = c->twante.alloc(nkt))) return st;
  const size_t nkk = (size_t)c->J * c->KP * c->KP;
  if (c->twdp.n < nkk && (st = c->twdp.alloc(nkk))) return st;
  if (c->twstate.n < (size_t)c->J * c->Tp && (st = c->twstate.alloc((size_t)c->J * c->Tp))) return st;
  // (the ceilings are per function, not per context: set to the most any
  // context may ask, as set_lds_limits does)
  if (hipFuncSetAttribute((const void *)k_tw_statediv, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)kLdsMax) != hipSuccess ||
      hipFuncSetAttribute((const void *)k_tw_decode, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)decode_lds(kMaxKP)) != hipSuccess) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the TW_constr kernels");
    return FASST_ERR_DEVICE;
  }
  return FASST_OK;
}

int launch_tw_statediv(fasst_ctx *c, double omega, bool plane_is_hatw) {
  TDArgs a{};
  a.TW = c->TW.p;
  a.Wkf_old = c->Wkf.p;
  a.Wkf_new = c->Wkf_new.p;
  a.rho = c->hatW.p;
  a.twall = c->twall.p;
  a.isdiv = c->isdiv.p;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.omega = omega;
  a.is_hatw = plane_is_hatw ? 1 : 0;
  a.halt = c->halt;
  for (int j = 0; j < kMaxJ; ++j) {
    a.K[j] = j < c->J ? c->K[j] : 0;
    a.kind[j] = j < c->J && c->tw_free[j] ? c->twc[j] : 0;
  }
  k_tw_statediv<<<dim3((c->T + kTdFrames - 1) / kTdFrames, c->J), 64 * kTdFrames, statediv_lds(c),
                  c->stream>>>(a);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

int launch_tw_decode(fasst_ctx *c) {
  TVArgs a{};
  a.TW = c->TW.p;
  a.dp = c->twdp.p;
  a.twall = c->twall.p;
  a.isdiv = c->isdiv.p;
  a.ante = c->twante.p;
  a.state = c->twstate.p;
  a.T = c->T;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.halt = c->halt;
  int kmax = 1;
  for (int j = 0; j < kMaxJ; ++j) {
    const bool on = j < c->J && c->tw_free[j] && c->twc[j];
    a.K[j] = j < c->J ? c->K[j] : 0;
    a.kind[j] = on ? c->twc[j] : 0;
    a.dpfree[j] = on ? c->twc_free[j] : 0;
    a.log1k[j] = on ? std::log(1. / (double)c->K[j]) : 0.0;
    if (on) kmax = std::max(kmax, c->K[j]);
  }
  k_tw_decode<<<c->J, kTvThreads, decode_lds(kmax), c->stream>>>(a);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

}  // namespace fasst

using namespace fasst;

extern "C" {

int fasst_set_tw_constr(fasst_ctx *c, int j, int kind, const double *TW_all, const double *dp,
                        int dp_free) {
  if (!c || !c->configured || j < 0 || j >= c->J) {
    set_error("fasst_set_tw_constr: component %d of an unconfigured or smaller model", j);
    return FASST_ERR_SHAPE;
  }
  if (kind < 0 || kind > 2) {
    set_error("fasst_set_tw_constr: kind %d (0 NMF, 1 GSMM, 2 SHMM)", kind);
    return FASST_ERR_UNSUPPORTED;
  }
  if (kind == 0) {
    c->twc[j] = c->twc_free[j] = 0;
    c->anytwc = 0;
    for (int i = 0; i < c->J; ++i) c->anytwc |= c->twc[i] != 0;
    return FASST_OK;
  }
  if (c->nblk[j] != 1 || c->tbl[j][0] > 0) {
    set_error("source %d: a discrete-state TW needs the source's only spectral component, "
              "without time blobs", j);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(c->device);
  int st = twc_alloc(c);
  if (st) return st;
  const int K = c->K[j], KP = c->KP;
  const DSpan<double> twall = c->twall.at((size_t)j * KP * c->Tp, (size_t)KP * c->Tp);
  const DSpan<double> d = c->twdp.at((size_t)j * KP * KP, (size_t)KP * KP);
  FASST_TRY(twall.zero(twall.n, c->stream));
  if (TW_all) {
    FASST_TRY(twall.put_rows(TW_all, K, c->T, c->T, c->Tp, c->stream));
  } else {
    k_twall_init<<<(c->T + 255) / 256, 256, 0, c->stream>>>(c->TW.p + (size_t)j * KP * c->Tp,
                                                           twall.p, K, c->T, c->Tp);
    FASST_LAUNCH_CHECK();
  }
  // the prior: K state probabilities (GSMM) or K x K transitions (SHMM);
  // default 1 / K (:1750-1760)
  std::vector<double> def;
  const int rows = kind == 1 ? 1 : K;
  if (!dp) {
    def.assign((size_t)rows * K, 1. / (double)K);
    dp = def.data();
  }
  FASST_TRY(d.zero(d.n, c->stream));
  FASST_TRY(d.put_rows(dp, rows, K, K, KP, c->stream));
  FASST_TRY(c->twstate.at((size_t)j * c->Tp).zero(c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  c->twc[j] = kind;
  c->twc_free[j] = dp_free ? 1 : 0;
  c->anytwc = 1;
  return FASST_OK;
}

int fasst_get_tw_constr(fasst_ctx *c, int j, double *TW_all, double *dp, int *state) {
  if (!c || !c->configured || j < 0 || j >= c->J || !c->twc[j]) {
    set_error("fasst_get_tw_constr: component %d carries no discrete-state constraint", j);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  const int K = c->K[j], KP = c->KP;
  if (TW_all)
    FASST_TRY(c->twall.at((size_t)j * KP * c->Tp, (size_t)KP * c->Tp)
                  .get_rows(TW_all, K, c->T, c->T, c->Tp, c->stream));
  if (dp)
    FASST_TRY(c->twdp.at((size_t)j * KP * KP, (size_t)KP * KP)
                  .get_rows(dp, c->twc[j] == 1 ? 1 : K, K, K, KP, c->stream));
  if (state) FASST_TRY(c->twstate.at((size_t)j * c->Tp, c->Tp).get(state, c->T, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

}  // extern "C"
