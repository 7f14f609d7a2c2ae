// The spectral phase of the GEM iteration (update_spectral_components,
// audioModel.py:1469-1978) and its operands:
//   k_w_from_fb   W = FB.FW                       (comp_spat_comp_power :485)
//   k_fwh_t       (FW.TW)^T, k_tw_rowsum sum_t TW (launch_spectral_prep)
//   k_fb_contract FB numerator over t (MFMA, :1521-1575)
//   k_fb_update   FB *= (num/den)^omega, W_new = FB.FW
//   k_fw_contract / _reduce / _final   the free FW's update (:1578-1631)
//   k_tw_contract_lds (one component per source) or k_tw_contract<BLK>: TW
//                 numerator / denominator over f (MFMA, :1634-1727)
//   k_tw_update   TW *= (num/den)^omega
//   k_multi_prep, k_tb_*   several spectral components on a source, time blobs
//                 (multi_step)
//   k_rho_from_hatw   the rho planes from a caller's hat_W (fasst_spectral_update)
// Interface: fasst_em.h (launch_w_old: fasst_ctx.h).

#include "fasst_em.h"
#include "fasst_device.h"
#include "fasst_twc.h"

#include <algorithm>

namespace fasst {

// ---------------------------------------------------------------- prep
// W[j] = FB[j] . FW[j], written [KP][Fp] (f contiguous).
// one block per (16-bin tile, source): FB tile and FW staged in LDS; the
// outputs are written bin-fastest (coalesced Wkf rows)
template <bool FWG>   // FWG: FW read from L2 (KP > 64), else staged in LDS
__global__ __launch_bounds__(256) void k_w_from_fb(const double *__restrict__ FB,
                                                   const double *__restrict__ FW,
                                                   double *__restrict__ Wkf,
                                                   double *__restrict__ Wfk, int J, int Fp,
                                                   int KP, const int *halt) {
  HALT_GUARD(halt);
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  double *s_fb = s_m;             // [16][KP + 1]
  double *s_fw = s_m + 16 * (KP + 1);  // [KP][KP] (KP <= 64; else FW is read from L2)
  constexpr bool fwg = FWG;
  const int j = blockIdx.y, f0 = blockIdx.x * 16;
  const double *fw = fwg ? FW + (size_t)j * KP * KP : s_fw;
  for (int idx = threadIdx.x; idx < 16 * KP; idx += blockDim.x) {
    const int fl = idx / KP, q = idx % KP;
    s_fb[fl * (KP + 1) + q] = FB[((size_t)j * Fp + f0 + fl) * KP + q];
  }
  if constexpr (fwg) {
    // KP = 128 on the matrix cores: D[k][f] = sum_q FW[q][k] FB[f][q] per
    // 16 x 16 tile (16x16x4: A = FW^T rows from L2, B = the FB tile in LDS),
    // wave w forming the k tiles w, w + 4, ...; lane (fl, tq) then holds
    // W[k = 16 kc + tq + 4 i][f0 + fl] (128-byte Wkf row pieces)
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, fl = lane & 15, tq = lane >> 4;
    for (int kc = wv; kc < KP / 16; kc += 4) {
      d4 d = d4{0.0, 0.0, 0.0, 0.0};
      for (int q0 = 0; q0 < KP; q0 += 4)
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(fw[(size_t)(q0 + tq) * KP + 16 * kc + fl],
                                                 s_fb[fl * (KP + 1) + q0 + tq], d, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * kc + tq + 4 * i;
        Wkf[((size_t)j * KP + k) * Fp + f0 + fl] = d[i];
        if (Wfk) Wfk[((size_t)j * Fp + f0 + fl) * KP + k] = d[i];
      }
    }
    return;
  }
  if (!fwg)
    for (int idx = threadIdx.x; idx < KP * KP; idx += blockDim.x)
      s_fw[idx] = FW[(size_t)j * KP * KP + idx];
  __syncthreads();
  for (int idx = threadIdx.x; idx < 16 * KP; idx += blockDim.x) {
    const int k = idx / 16, fl = idx % 16;
    double s = 0.0;
    for (int q = 0; q < KP; ++q) s += s_fb[fl * (KP + 1) + q] * fw[q * KP + k];
    Wkf[((size_t)j * KP + k) * Fp + f0 + fl] = s;
    if (Wfk) Wfk[((size_t)j * Fp + f0 + fl) * KP + k] = s;
  }
}

// FWHt[j][t][k] = sum_q FW[j][k][q] TW[j][q][t]; one block per (64-frame
// tile, source): FW and the TW tile staged in LDS, coalesced [t][k] writes.
template <bool FWG>
__global__ __launch_bounds__(256) void k_fwh_t(const double *__restrict__ FW,
                                               const double *__restrict__ TW,
                                               double *__restrict__ FWHt, double *__restrict__ TWt,
                                               int J, int Tp, int KP, const int *halt) {
  HALT_GUARD(halt);
  extern __shared__ __attribute__((aligned(16))) double s_f[];
  // FWG (KP = 128): FW's [KP][KP] copy and the TW tile do not fit LDS
  // together, so FW goes through it in two halves of its rows q (the
  // contraction index), each thread keeping its outputs in registers (FW
  // read straight from L2 was a 1 KB-stride gather per lane: 1.36 ms at
  // J = 8, K = 128)
  constexpr bool fwg = FWG;
  double *s_fw = s_f;                                  // [QH][KP] (q-major, transposed)
  double *s_tw = s_f + (fwg ? 16 * KP : KP * KP);      // [KP][64]
  const int j = blockIdx.y, t0 = blockIdx.x * 64;
  const int tn = min(64, Tp - t0);
  for (int idx = threadIdx.x; idx < KP * 64; idx += blockDim.x) {
    const int q = idx >> 6, tl = idx & 63;
    s_tw[idx] = tl < tn ? TW[((size_t)j * KP + q) * Tp + t0 + tl] : 0.0;
  }
  if constexpr (fwg) {
    // KP = 128 on the matrix cores: wave w forms frames 16 w .. 16 w + 15,
    // D[k][t] = sum_q FW[k][q] TW[q][t] per 16 x 16 tile (16x16x4: A = FW
    // through LDS transposed, QB rows q at a time; B = the TW tile); lane
    // (fl, tq) then holds FWHt[t0 + 16 w + fl][16 kc + tq + 4 i]
    constexpr int KPG = 128, QB = 16;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, fl = lane & 15, tq = lane >> 4;
    d4 d[KPG / 16];
#pragma unroll
    for (int kc = 0; kc < KPG / 16; ++kc) d[kc] = d4{0.0, 0.0, 0.0, 0.0};
    for (int qb = 0; qb < KPG; qb += QB) {
      __syncthreads();   // (qb > 0: the previous chunk's reads are done)
      for (int idx = threadIdx.x; idx < QB * KPG; idx += blockDim.x) {
        const int k = idx / QB, q = idx % QB;   // (coalesced over q in FW's rows)
        s_fw[q * KPG + k] = FW[((size_t)j * KPG + k) * KPG + qb + q];
      }
      __syncthreads();
#pragma unroll
      for (int kc = 0; kc < KPG / 16; ++kc)
#pragma unroll
        for (int q0 = 0; q0 < QB; q0 += 4)
          d[kc] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_fw[(q0 + tq) * KPG + 16 * kc + fl],
                                                       s_tw[(qb + q0 + tq) * 64 + 16 * wv + fl], d[kc], 0, 0,
                                                       0);
    }
    const int tl = 16 * wv + fl;
    if (tl < tn)
#pragma unroll
      for (int kc = 0; kc < KPG / 16; ++kc)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 16 * kc + tq + 4 * i;
          FWHt[((size_t)j * Tp + t0 + tl) * KPG + k] = d[kc][i];
          if (TWt) TWt[((size_t)j * Tp + t0 + tl) * KPG + k] = s_tw[k * 64 + tl];
        }
    return;
  }
  for (int idx = threadIdx.x; idx < KP * KP; idx += blockDim.x) {
    const int k = idx / KP, q = idx % KP;  // stored transposed: s_fw[q][k]
    s_fw[q * KP + k] = FW[(size_t)j * KP * KP + idx];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < tn * KP; idx += blockDim.x) {
    const int tl = idx / KP, k = idx % KP;
    double s = 0.0;
    for (int q = 0; q < KP; ++q) s += s_fw[q * KP + k] * s_tw[q * 64 + tl];
    FWHt[((size_t)j * Tp + t0 + tl) * KP + k] = s;
    if (TWt) TWt[((size_t)j * Tp + t0 + tl) * KP + k] = s_tw[k * 64 + tl];  // H^T (FW update)
  }
}

// sum_t TW[j][k][t] (for mean_t V_j = W_j . sum_t H_j, the hat_Rss diagonal term)
__global__ void k_tw_rowsum(const double *__restrict__ TW, double *__restrict__ hsum, int T,
                            int Tp, const int *halt) {
  HALT_GUARD(halt);
  __shared__ double s[256];
  const double *row = TW + (size_t)blockIdx.x * Tp;
  double x = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) x += row[t];
  s[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) hsum[blockIdx.x] = s[0];
}

// sum_{c < n} p[c * stride] in index order (bit-identical to the plain loop)
// with 8 loads in flight: the chunk reductions below were load-latency bound
__device__ __forceinline__ double chunk_sum(const double *__restrict__ p, size_t stride, int n) {
  double x = 0.0;
  int c = 0;
  for (; c + 8 <= n; c += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(c + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) x += v[u];
  }
  for (; c < n; ++c) x += p[(size_t)c * stride];
  return x;
}

// ---------------------------------------------------------------- FB update
struct BArgs {
  const double *TW, *Wkf, *FWHt, *hatW;
  const double *hatW2;  // DEN: the denominator ratio plane (multi-block update)
  double *bnum;  // [nchunk][J][Fp][KP]
  double *bden;  // DEN: [nchunk][J][Fp][KP]
  int F, T, Fp, Tp, KP, J, ntt, nft, tpc;
  int zbase, tbase;  // this launch's chunks start at partial zbase, frame tile tbase (ntt = end)
  int fb_free[kMaxJ];
  const int *halt;
};

// FB numerator over t (:1521-1575), one wave per (FPW bin tiles, source,
// frame chunk):  num[f][k] = sum_t rho[f][t] (FW.H)^T[t][k] with
// rho = hat_W / V^2 * V formed by the E-step (N1: other_fact_power ==
// spat_comp_power == V).  The denominator sum_t (V * (1/V)) (FW.H)^T[t][k] is
// the f-independent sum_t (FW.H)^T[t][k] = (FW . rowsum(TW))[k] (to one
// rounding of V*(1/V)); k_fb_update forms it from hsum, and only the
// numerator is contracted here: a plain (F x T).(T x K) product whose rho
// tiles arrive bins-on-lanes, i.e. already in the A-operand layout, and whose
// (FW.H)^T B operand is shared by the FPW bin tiles.
// DEN (several spectral components on source j, audioModel.py:1525-1571):
// the numerator plane is (hat_W_j / V_j^2) other and a second plane
// other / V_j is contracted into the denominator the same way.
// Without DEN and FPW even the tiles are interleaved (bin f in tile f mod
// FPW), so each lane's rho values arrive as 16-byte loads (C3: 0.166 ->
// 0.155 ms at FPW = 2, same-box A/B).
template <int NKC, int FPW, bool DEN = false>
__global__ __launch_bounds__(64) void k_fb_contract(const BArgs a) {
  HALT_GUARD(a.halt);
  const int lane = threadIdx.x, fl = lane & 15, tq = lane >> 4;
  const dim3 bi = xcd_block();   // x: bin-tile group, y: source, z: frame chunk
  const int ft0 = bi.x * FPW, j = bi.y;
  if (!a.fb_free[j]) return;
  d4 num[FPW][NKC], den[DEN ? FPW : 1][NKC];
#pragma unroll
  for (int p = 0; p < FPW; ++p)
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) num[p][kc] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < (DEN ? FPW : 1); ++p)
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) den[p][kc] = d4{0.0, 0.0, 0.0, 0.0};
  const int tb = a.tbase + bi.z * a.tpc, te = min(tb + a.tpc, a.ntt);
  const double *rhoj = a.hatW + (size_t)j * a.Tp * a.Fp;
  const double *rdj = DEN ? a.hatW2 + (size_t)j * a.Tp * a.Fp : nullptr;
  for (int tt = tb; tt < te; ++tt) {
    const int t0 = tt * 16;
    double fb[4][NKC];
    const double *fwh = a.FWHt + ((size_t)j * a.Tp + t0 + tq) * a.KP + fl;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) fb[i][kc] = fwh[(size_t)(4 * i) * a.KP + kc * 16];
    if constexpr (FPW % 2 == 0 && !DEN) {
      // the wave's FPW bin tiles interleaved: lane fl loads bins
      // FPW fl .. FPW fl + FPW - 1 of the 16 FPW-bin group with 16-byte loads
      // (tile p = the bins == p mod FPW): 4 rows x 16 FPW contiguous doubles
      // per load instruction instead of 4 x 16
      const int fp = ft0 * 16 + FPW * fl;
      double r[FPW][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = t0 + tq + 4 * i < a.T && fp < a.Fp;
        const double *src = rhoj + (size_t)(t0 + tq + 4 * i) * a.Fp + fp;
#pragma unroll
        for (int h = 0; h < FPW; h += 2) {
          const double2 v = ok ? *(const double2 *)(src + h) : make_double2(0.0, 0.0);
          r[h][i] = v.x;
          r[h + 1][i] = v.y;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < FPW; ++p)
#pragma unroll
          for (int kc = 0; kc < NKC; ++kc) num[p][kc] = mfma4(r[p][i], fb[i][kc], num[p][kc]);
      continue;
    }
#pragma unroll
    for (int p = 0; p < FPW; ++p) {
      if (ft0 + p >= a.nft) break;  // wave-uniform: no bin tile left
      const int f = (ft0 + p) * 16 + fl;
      double r1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        r1[i] = t0 + tq + 4 * i < a.T ? rhoj[(size_t)(t0 + tq + 4 * i) * a.Fp + f] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) num[p][kc] = mfma4(r1[i], fb[i][kc], num[p][kc]);
      if constexpr (DEN) {
        double r2[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          r2[i] = t0 + tq + 4 * i < a.T ? rdj[(size_t)(t0 + tq + 4 * i) * a.Fp + f] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kc = 0; kc < NKC; ++kc) den[p][kc] = mfma4(r2[i], fb[i][kc], den[p][kc]);
      }
    }
  }
  const size_t base = ((size_t)(a.zbase + bi.z) * a.J + j) * a.Fp;
  if constexpr (FPW % 2 == 0 && !DEN) {   // interleaved tiles: tile p holds bins p mod FPW
#pragma unroll
    for (int p = 0; p < FPW; ++p)
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int f = ft0 * 16 + FPW * (tq + 4 * m) + p;
          if (f < a.Fp) a.bnum[(base + f) * a.KP + kc * 16 + fl] = num[p][kc][m];
        }
    return;
  }
#pragma unroll
  for (int p = 0; p < FPW; ++p) {
    if (ft0 + p >= a.nft) break;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const size_t o = (base + (ft0 + p) * 16 + tq + 4 * m) * a.KP + kc * 16 + fl;
        a.bnum[o] = num[p][kc][m];
        if constexpr (DEN) a.bden[o] = den[DEN ? p : 0][kc][m];
      }
  }
}

struct UArgs {
  double *FB;
  const double *FW, *bnum, *hsum;
  const double *bden;  // null: den = FW . rowsum(TW); else contracted per (f, k)
  double *Wkf_new, *Wfk_new;
  int F, Fp, KP, J, nchunk;
  double omega;
  int kb0[kMaxJ], kb1[kMaxJ], fb_free[kMaxJ];  // columns [kb0, kb1) are updated
  // fused tail (pmax non-null): the renormalisation's stage-1 statistics of
  // this block's 16 bins, the FB column maxima [J][nft][KP] (the mixing
  // filters' energy is k_renorm_scales', read after the mixing update)
  double *pmax;
  const int *halt;
};
// FB *= (num / max(den, eps))^omega with den = FW . rowsum(TW) (see
// k_fb_contract) or, for one of several spectral components, the contracted
// denominator; then W_new = FB . FW in both layouts.
template <bool FWG>
__global__ __launch_bounds__(256) void k_fb_update(const UArgs a) {
  HALT_GUARD(a.halt);
  // LDS: FW [KP][KP] | FB rows [16][PB] | den [KP] | W_new rows [16][KP + 1]
  extern __shared__ __attribute__((aligned(16))) double s_fw[];
  const int f0 = blockIdx.x * 16, j = blockIdx.y;
  const int KP = a.KP;
  constexpr bool fwg = FWG;   // FW read from L2 (its [KP][KP] copy would not fit)
  const int PB = fwg ? KP + 1 : KP;   // (odd pitch: the MFMA B reads of 16 rows)
  const double *fw = fwg ? a.FW + (size_t)j * KP * KP : s_fw;
  double *s_fb = s_fw + (fwg ? 0 : KP * KP);
  double *s_den = s_fb + 16 * PB;
  double *s_wn = s_den + KP;
  if (!fwg)
    for (int idx = threadIdx.x; idx < KP * KP; idx += blockDim.x)
      s_fw[idx] = a.FW[(size_t)j * KP * KP + idx];
  for (int k = threadIdx.x; k < KP; k += blockDim.x) s_den[k] = a.hsum[(size_t)j * KP + k];
  __syncthreads();
  double dk = 0.0;
  if (threadIdx.x < KP)
    for (int q = 0; q < KP; ++q) dk += fw[threadIdx.x * KP + q] * s_den[q];
  __syncthreads();
  if (threadIdx.x < KP) s_den[threadIdx.x] = dk;
  __syncthreads();
  for (int idx = threadIdx.x; idx < 16 * KP; idx += blockDim.x) {
    const int fl = idx / KP, k = idx % KP, f = f0 + fl;
    const size_t o = ((size_t)j * a.Fp + f) * KP + k;
    double fb = a.FB[o];
    if (a.fb_free[j] && f < a.F && k >= a.kb0[j] && k < a.kb1[j]) {
      double num = 0.0;
      num = chunk_sum(a.bnum + ((size_t)j * a.Fp + f) * KP + k, (size_t)a.J * a.Fp * KP, a.nchunk);
      const double den =
          a.bden ? chunk_sum(a.bden + ((size_t)j * a.Fp + f) * KP + k, (size_t)a.J * a.Fp * KP,
                             a.nchunk)
                 : s_den[k];
      const double ratio = num / fmax(den, kEps);
      fb *= a.omega == 1.0 ? ratio : pow(ratio, a.omega);
      a.FB[o] = fb;
    }
    s_fb[fl * PB + k] = fb;
  }
  __syncthreads();
  // W_new = FB . FW: [f][k] rows written coalesced over k here, the [k][f]
  // layout from the LDS copy below (coalesced over the 16 bins)
  if constexpr (fwg) {
    // KP = 128 on the matrix cores (as k_w_from_fb): D[k][f] = sum_q FW[q][k]
    // FB[f][q] per 16 x 16 tile, wave w forming the k tiles w, w + 4, ...
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, fl = lane & 15, tq = lane >> 4;
    for (int kc = wv; kc < KP / 16; kc += 4) {
      d4 d = d4{0.0, 0.0, 0.0, 0.0};
      for (int q0 = 0; q0 < KP; q0 += 4)
        d = mfma4(fw[(size_t)(q0 + tq) * KP + 16 * kc + fl], s_fb[fl * PB + q0 + tq], d);
#pragma unroll
      for (int i = 0; i < 4; ++i) s_wn[fl * (KP + 1) + 16 * kc + tq + 4 * i] = d[i];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * KP; idx += blockDim.x) {
      const int fl = idx / KP, k = idx % KP;
      a.Wfk_new[((size_t)j * a.Fp + f0 + fl) * KP + k] = s_wn[fl * (KP + 1) + k];
    }
  } else {
    for (int idx = threadIdx.x; idx < 16 * KP; idx += blockDim.x) {
      const int fl = idx / KP, k = idx % KP, f = f0 + fl;
      double s = 0.0;
      for (int q = 0; q < KP; ++q) s += s_fb[fl * KP + q] * fw[q * KP + k];
      a.Wfk_new[((size_t)j * a.Fp + f) * KP + k] = s;
      s_wn[fl * (KP + 1) + k] = s;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 16 * KP; idx += blockDim.x) {
    const int k = idx / 16, fl = idx % 16;
    a.Wkf_new[((size_t)j * KP + k) * a.Fp + f0 + fl] = s_wn[fl * (KP + 1) + k];
  }
  if (!a.pmax) return;
  // renormalize_parameters' statistics of the updated FB rows (k_renorm_stats
  // per 16-bin block; max_f is exact in any order)
  const int nb = min(16, a.F - f0);
  for (int k = threadIdx.x; k < KP; k += blockDim.x) {
    double m = -INFINITY;
    for (int fl = 0; fl < nb; ++fl) m = fmax(m, s_fb[fl * PB + k]);
    a.pmax[((size_t)j * gridDim.x + blockIdx.x) * KP + k] = m;
  }
}

// ---------------------------------------------------------------- FW update
// update_spectral_components, FW branch (audioModel.py:1578-1631), for the
// sources whose FW_frdm_prior is 'free'.  With one NMF factor other =
// max(V_old, eps) (N1) and the spatial power of the FW step is
// vm = max(V_mid, eps), V_mid = (FB_new FW_old) H (comp_spat_comp_power after
// the FB update, :1582-1588), so
//   num[k1][k2] = sum_f FB_new[f][k1] sum_t (hat_W / vm^2) other H[k2][t]
//   den[k1][k2] = sum_f FB_new[f][k1] sum_t (other / vm) H[k2][t]
// k_fw_contract forms the two ratio tiles (V_old and V_mid on the MFMA pipe,
// hat_W = rho * other from the E-step) and contracts them over t with H^T
// (G[f][k] per frame chunk, the k_fb_contract operand layout); k_fw_reduce
// contracts G with FB_new over bins (partials per bin chunk); k_fw_final
// applies FW *= (num / max(den, eps))^omega.
struct FWArgs {
  const double *TW, *TWt, *Wkf_old, *Wkf_mid, *hatW, *FB;
  double *gnum, *gden;  // [nchunk][J][Fp][KP]
  double *pnum, *pden;  // [nfc][J][KP][KP]
  double *FW;
  int F, T, Fp, Tp, KP, J, ntt, tpc, nchunk, nfc, fpc;
  int K[kMaxJ], fw_free[kMaxJ];
  int kb0[kMaxJ], kb1[kMaxJ];  // the FW block [kb0, kb1)^2 updated (BLK: the V tiles too)
  const double *cp, *pw;       // LAM: corrPen / powers planes of k_multi_prep
  double omega;
  const int *halt;
};

// BLK (one of several spectral components on source j): V_old / V_mid are the
// component's own powers (comp_spat_comp_power(..., spec_comp_ind=[k]),
// :1582-1588) and rho is the plane hat_W_j / max(V_c_old, eps).
template <int NKC, bool BLK = false, bool LAM = false>
__global__ __launch_bounds__(64) void k_fw_contract(const FWArgs a) {
  HALT_GUARD(a.halt);
  constexpr int NKS = 4 * NKC;
  const int lane = threadIdx.x, fl = lane & 15, tq = lane >> 4;
  const int j = blockIdx.y;
  if (!a.fw_free[j]) return;
  const int f0 = blockIdx.x * 16, f = f0 + fl;
  const int KP = a.KP;
  double wo[NKS], wmid[NKS];  // B operands of the V tiles: W[k = tq + 4 s][f]
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    wo[s] = a.Wkf_old[((size_t)j * KP + tq + 4 * s) * a.Fp + f];
    wmid[s] = a.Wkf_mid[((size_t)j * KP + tq + 4 * s) * a.Fp + f];
    if constexpr (BLK) {
      const int k = tq + 4 * s;
      if (k < a.kb0[j] || k >= a.kb1[j]) wo[s] = wmid[s] = 0.0;
    }
  }
  d4 gn[NKC], gd[NKC];
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) gn[kc] = gd[kc] = d4{0.0, 0.0, 0.0, 0.0};
  const double *rhoj = a.hatW + (size_t)j * a.Tp * a.Fp;
  const int tb = blockIdx.z * a.tpc, te = min(tb + a.tpc, a.ntt);
  for (int tt = tb; tt < te; ++tt) {
    const int t0 = tt * 16;
    const double *tw = a.TW + ((size_t)j * KP + tq) * a.Tp + t0 + fl;
    d4 vo = d4{0.0, 0.0, 0.0, 0.0}, vm = vo;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      const double h = tw[(size_t)(4 * s) * a.Tp];
      vo = mfma4(h, wo[s], vo);
      vm = mfma4(h, wmid[s], vm);
    }
    double rn[4], rd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + tq + 4 * i;
      const bool ok = t < a.T && f < a.F;
      const double rho = ok ? rhoj[(size_t)t * a.Fp + f] : 0.0;
      const double other = fmax(vo[i], kEps);
      const double rv = 1.0 / fmax(vm[i], kEps);
      if constexpr (LAM) {   // corrPen terms (audioModel.py:1596-1628)
        const size_t o = (size_t)j * a.Tp * a.Fp + (size_t)t * a.Fp + f;
        const double cp = ok ? a.cp[o] : 0.0, pw = ok ? a.pw[o] : 1.0;
        const double vmm = fmax(vm[i], kEps);
        rn[i] = ok ? ((rho * other) * (rv * rv) + cp * (2.0 * (vmm / pw))) * other : 0.0;
        rd[i] = ok ? other * (rv + cp) : 0.0;
      } else {
        rn[i] = ok ? ((rho * other) * (rv * rv)) * other : 0.0;  // (hat_W / vm^2) other
        rd[i] = ok ? other * rv : 0.0;                           // other (1 / vm)
      }
    }
    const double *ht = a.TWt + ((size_t)j * a.Tp + t0 + tq) * KP + fl;  // H^T[t][k]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        const double h = ht[(size_t)(4 * i) * KP + kc * 16];
        gn[kc] = mfma4(rn[i], h, gn[kc]);
        gd[kc] = mfma4(rd[i], h, gd[kc]);
      }
  }
  const size_t base = ((size_t)blockIdx.z * a.J + j) * a.Fp;
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const size_t o = (base + f0 + tq + 4 * m) * KP + kc * 16 + fl;
      a.gnum[o] = gn[kc][m];
      a.gden[o] = gd[kc][m];
    }
}

// partial FB_new^T G over the bins of chunk blockIdx.x (G summed over the
// frame chunks first, in chunk order)
__global__ __launch_bounds__(256) void k_fw_reduce(const FWArgs a) {
  HALT_GUARD(a.halt);
  const int j = blockIdx.y, fc = blockIdx.x;
  if (!a.fw_free[j]) return;
  const int KP = a.KP, K = a.K[j];
  extern __shared__ __attribute__((aligned(16))) double s_g[];  // [fpc][KP] x 3
  double *s_n = s_g, *s_d = s_g + a.fpc * KP, *s_b = s_g + 2 * a.fpc * KP;
  const int fb = fc * a.fpc, fe = min(fb + a.fpc, a.F), nf = fe - fb;
  for (int idx = threadIdx.x; idx < nf * KP; idx += blockDim.x) {
    const int fl = idx / KP, k = idx % KP, f = fb + fl;
    double n = 0.0, d = 0.0;
    for (int c = 0; c < a.nchunk; ++c) {
      const size_t o = (((size_t)c * a.J + j) * a.Fp + f) * KP + k;
      n += a.gnum[o];
      d += a.gden[o];
    }
    s_n[idx] = n;
    s_d[idx] = d;
    s_b[idx] = a.FB[((size_t)j * a.Fp + f) * KP + k];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
    const int k1 = idx / K, k2 = idx % K;
    double n = 0.0, d = 0.0;
    for (int fl = 0; fl < nf; ++fl) {
      const double b = s_b[fl * KP + k1];
      n += b * s_n[fl * KP + k2];
      d += b * s_d[fl * KP + k2];
    }
    const size_t o = (((size_t)fc * a.J + j) * KP + k1) * KP + k2;
    a.pnum[o] = n;
    a.pden[o] = d;
  }
}

__global__ __launch_bounds__(256) void k_fw_final(const FWArgs a) {
  HALT_GUARD(a.halt);
  const int j = blockIdx.x;
  if (!a.fw_free[j]) return;
  const int KP = a.KP, K = a.K[j];
  double *FW = a.FW + (size_t)j * KP * KP;
  for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
    const int k1 = idx / K, k2 = idx % K;
    double n = 0.0, d = 0.0;
    for (int fc = 0; fc < a.nfc; ++fc) {
      const size_t o = (((size_t)fc * a.J + j) * KP + k1) * KP + k2;
      n += a.pnum[o];
      d += a.pden[o];
    }
    if (k1 < a.kb0[j] || k1 >= a.kb1[j] || k2 < a.kb0[j] || k2 >= a.kb1[j]) continue;
    const double ratio = n / fmax(d, kEps);
    FW[k1 * KP + k2] *= a.omega == 1.0 ? ratio : pow(ratio, a.omega);
  }
}

// ---------------------------------------------------------------- TW update
struct TArgs {
  const double *TW, *Wkf_old, *Wkf_new, *Wfk_new, *hatW;
  double *tnum, *tden;  // [nsplit][J][Tp][KP]
  TwSched ts;           // k_tw_contract_lds<BAL>: its schedule and the partials' slots
  int F, T, Fp, Tp, KP, J, nft, ntt, fpc;
  int tw_free[kMaxJ];
  int kb0[kMaxJ], kb1[kMaxJ];  // BLK: the V tiles sum the columns [kb0, kb1) only
  const double *cp, *pw;       // LAM: corrPen / powers planes of k_multi_prep
  const double *oth;           // TBQ: max(V_c, eps) plane of k_multi_prep
  double omega;
  const int *halt;
};

// TW numerator / denominator over f (:1694-1726), one wave per (TPW frame
// tiles, source, bin chunk):
//   num[k][t] = sum_f W_new[f][k] * V_old * hat_W / V_new^2,
//   den[k][t] = sum_f W_new[f][k] * V_old / V_new
// V_old = W_old . TW, V_new = W_new . TW recomputed in registers, hat_W =
// rho * max(V_old, eps) from the E-step's rho; the W operands (A of the V
// tiles, B of the contraction) are shared by the TPW frame tiles.  Partial
// sums per bin chunk go to tnum / tden.
// BLK (one of several spectral components on source j): V_old / V_new are the
// component's own powers W_c H_c (the reference's spec_comp_ind=[k],
// audioModel.py:1639-1645), and rho is the plane hat_W_j / max(V_c_old, eps).
// TBQ (the TB step of a component with time blobs, :1931-1978): H has moved
// since the step's start, so other = max(V_c_old, eps) comes from a plane,
// hatW is hat_W_j itself, and num's ratio is hat_W / max(V_new^2, eps).
template <int NKC, int TPW, bool BLK = false, bool LAM = false, bool TBQ = false>
__global__ __launch_bounds__(64) void k_tw_contract(const TArgs a) {
  HALT_GUARD(a.halt);
  constexpr int NKS = 4 * NKC;
  const int lane = threadIdx.x, fl = lane & 15, tq = lane >> 4;
  const dim3 bi = xcd_block();   // x: frame-tile group, y: source, z: bin chunk
  const int tt0 = bi.x * TPW, j = bi.y;
  if (!a.tw_free[j]) return;
  double bt[TPW][NKS];
#pragma unroll
  for (int p = 0; p < TPW; ++p) {
    const bool tin = tt0 + p < a.ntt;
    const double *tw = a.TW + ((size_t)j * a.KP + tq) * a.Tp + (tt0 + p) * 16 + fl;
#pragma unroll
    for (int s = 0; s < NKS; ++s) bt[p][s] = tin ? tw[(size_t)(4 * s) * a.Tp] : 0.0;
  }
  d4 num[TPW][NKC], den[TPW][NKC];
#pragma unroll
  for (int p = 0; p < TPW; ++p)
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) num[p][kc] = den[p][kc] = d4{0.0, 0.0, 0.0, 0.0};
  const int fb = bi.z * a.fpc, fe = min(fb + a.fpc, a.nft);
  // the V tiles' bin rows are permuted (lane fl's A row is bin
  // 4 (fl & 3) + (fl >> 2)) so that a lane's four D values are the four
  // consecutive bins 4 tq .. 4 tq + 3: its rho values arrive as two 16-byte
  // loads (C3: 0.401 -> 0.381 ms, same-box A/B); the contraction's B rows
  // (W_new) follow the same order
  const int fpl = 4 * (fl & 3) + (fl >> 2);
  const int bq = 4 * tq, bs = 1;   // D value i is bin f0 + bq + bs i
  const double *wo = a.Wkf_old + ((size_t)j * a.KP + tq) * a.Fp + fpl;
  const double *wn = a.Wkf_new + ((size_t)j * a.KP + tq) * a.Fp + fpl;
  const double *wfk = a.Wfk_new + ((size_t)j * a.Fp + bq) * a.KP + fl;
  const double *hwj = a.hatW + (size_t)j * a.Tp * a.Fp;
  for (int ft = fb; ft < fe; ++ft) {
    const int f0 = ft * 16;
    double ao[NKS], an[NKS], bw[4][NKC];
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      ao[s] = TBQ ? 0.0 : wo[(size_t)(4 * s) * a.Fp + f0];
      an[s] = wn[(size_t)(4 * s) * a.Fp + f0];
      if constexpr (BLK) {
        const int k = tq + 4 * s;
        if (k < a.kb0[j] || k >= a.kb1[j]) ao[s] = an[s] = 0.0;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) bw[i][kc] = wfk[(size_t)(f0 + bs * i) * a.KP + kc * 16];
#pragma unroll
    for (int p = 0; p < TPW; ++p) {
      if (tt0 + p >= a.ntt) break;  // wave-uniform: no frame tile left
      const int t = (tt0 + p) * 16 + fl;
      double h[4];
      {  // (last use of rho: non-temporal)
        typedef double dv2 __attribute__((ext_vector_type(2)));
        const dv2 *hp = (const dv2 *)(hwj + (size_t)t * a.Fp + f0 + bq);
        const dv2 h01 = __builtin_nontemporal_load(hp), h23 = __builtin_nontemporal_load(hp + 1);
        h[0] = h01.x;
        h[1] = h01.y;
        h[2] = h23.x;
        h[3] = h23.y;
      }
      d4 vo = d4{0.0, 0.0, 0.0, 0.0}, vn = vo;
      d4 vo2 = vo, vn2 = vo;
#pragma unroll
      for (int s = 0; s < NKS; s += 2) {
        if constexpr (!TBQ) {
          vo = mfma4(ao[s], bt[p][s], vo);
          vo2 = mfma4(ao[s + 1], bt[p][s + 1], vo2);
        }
        vn = mfma4(an[s], bt[p][s], vn);
        vn2 = mfma4(an[s + 1], bt[p][s + 1], vn2);
      }
      vo += vo2;
      vn += vn2;
      {
        const bool tok = t < a.T;
        double r3[4], r4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double vm = fmax(vn[i], kEps);
          const double rv = rcp_nr(vm);
          const bool ok = tok && f0 + bq + bs * i < a.F;
          const size_t o = (size_t)j * a.Tp * a.Fp + (size_t)t * a.Fp + f0 + bq + bs * i;
          double other, q;
          if constexpr (TBQ) {
            other = ok ? a.oth[o] : 0.0;
            q = h[i] / fmax(vm * vm, kEps);   // hat_W / max(V^2, eps) (:1971-1973)
          } else {
            other = fmax(vo[i], kEps);
            q = (h[i] * other) * (rv * rv);   // hat_W from the E-step's rho
          }
          if constexpr (LAM) {   // corrPen terms (audioModel.py:1650-1719)
            const double cp = ok ? a.cp[o] : 0.0, pw = ok ? a.pw[o] : 1.0;
            r3[i] = ok ? other * (q + cp * (2.0 * (vm / pw))) : 0.0;
            r4[i] = ok ? other * (rv + cp) : 0.0;
          } else {
            r3[i] = ok ? other * q : 0.0;
            r4[i] = ok ? other * rv : 0.0;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kc = 0; kc < NKC; ++kc) {
            num[p][kc] = mfma4(r3[i], bw[i][kc], num[p][kc]);
            den[p][kc] = mfma4(r4[i], bw[i][kc], den[p][kc]);
          }
      }
    }
  }
  const size_t base = ((size_t)bi.z * a.J + j) * a.Tp;
#pragma unroll
  for (int p = 0; p < TPW; ++p) {
    if (tt0 + p >= a.ntt) break;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const size_t o = (base + (tt0 + p) * 16 + tq + 4 * m) * a.KP + kc * 16 + fl;
        a.tnum[o] = num[p][kc][m];
        a.tden[o] = den[p][kc][m];
      }
  }
}

// k_tw_contract's plain form (one spectral component per source, no
// lambdaCorr / time blobs, KP <= 64) with its per-bin-step operands staged in
// LDS by LDS-DMA (raw-buffer loads ... lds: no VGPR cost, NS stages in
// flight): a block of NW waves shares one source and bin chunk, wave w owns
// TPW frame tiles.  Stage c (bin tile fb + c) holds
//   Wo [KP][16]  W_old rows      (Wkf_old: KP / 8 pieces of 8 rows x 128 B;
//                not with SO)
//   Wn [KP][16]  W_new rows      (Wkf_new)
//   Wf [16][KP]  W_new, [f][k]   (Wfk_new, 16 KP contiguous doubles; a row r
//                with bit 2 set has its 128-B halves swapped, so the rows 4
//                apart that one ds_read_b64 lane group reads hit disjoint
//                bank halves; the DMA source applies the same involution)
//   rho [NW][TPW][8 granules][16 frames] x 16 B: the wave's own rho tiles,
//                granule-major so a lane's four consecutive bins are two
//                conflict-free ds_read_b128
// One s_barrier per bin step: wait (counted vmcnt) for the wave's own stage c
// pieces -> barrier -> issue stage c + NS - 1 into the buffer stage c - 1
// left -> compute stage c.  The arithmetic is k_tw_contract's, term for term.
template <int NKC, int NW, int TPW, int NS>
struct TwlCfg {
  static constexpr int NKC_ = NKC, NW_ = NW, TPW_ = TPW, NS_ = NS, NT = 64 * NW;
  static constexpr int KP = 16 * NKC;
  static constexpr int NWO = KP / 8;                // W pieces: Wo, Wn, Wf
  static constexpr int WPI = 3 * NWO;               // 1 KB W pieces per stage
  static constexpr int WD = 128 * WPI;              // W doubles per stage
  static constexpr int WN0 = 16 * KP, WF0 = 32 * KP;   // Wn / Wf offsets
  static constexpr int RD = 256;                    // rho doubles per frame tile
  static constexpr int SS = WD + NW * TPW * RD;     // doubles per stage
  static constexpr size_t smem = (size_t)NS * SS * sizeof(double);
  static constexpr int WPW = (WPI + NW - 1) / NW;   // W pieces per wave (upper bound)
  static constexpr int LPC = WPI / NW + 2 * TPW;    // loads per wave per stage (lower bound)
};

typedef __attribute__((address_space(3))) void lds_void_t;

// (the body is a device function: the host pass of a kernel template
// analyses its body, and the AMDGPU buffer-resource builtins do not exist there)
//
// BAL (the balanced schedule, fasst_twsched.h): a.ts.nb persistent blocks, each
// walking its contiguous range of the (source, frame group, bin step) list one
// segment at a time -- operands, pipeline, stores to the segment's slot -- so
// every block does the same number of bin steps (+-1) and a unit that one
// block finishes alone leaves one partial, not one per bin chunk.
template <class CF, bool BAL>
__device__ __forceinline__ void tw_contract_lds_body(const TArgs &a);
template <class CF, bool BAL = false>
__global__ __launch_bounds__(CF::NT) FASST_NO_LDS_PAIRING
void k_tw_contract_lds(const TArgs a) {
  tw_contract_lds_body<CF, BAL>(a);
}
template <class CF, bool BAL>
__device__ __forceinline__ void tw_contract_lds_body(const TArgs &a) {
  HALT_GUARD(a.halt);
  // one segment: source j, frame group grp, the nst bin steps from bin tile
  // fb, partials to `slot`
  auto segment = [&](int j, int grp, int fb, int nst, int slot) {
    constexpr int NKC = CF::NKC_, NW = CF::NW_, TPW = CF::TPW_, NS = CF::NS_;
    constexpr int KP = CF::KP, NKS = 4 * NKC, SS = CF::SS, WPI = CF::WPI, NWO = CF::NWO;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // (wv through readfirstlane: the compiler then knows it is wave-uniform, so
    // the piece / tile branches below are scalar, not exec-masked waterfalls)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fl = lane & 15, tq = lane >> 4;
    const int tt0 = (grp * NW + wv) * TPW;   // this wave's first frame tile
    // TW operands of the V tiles (resident for the whole bin loop)
    double bt[TPW][NKS];
#pragma unroll
    for (int p = 0; p < TPW; ++p) {
      const bool tin = tt0 + p < a.ntt;
      const double *tw = a.TW + ((size_t)j * a.KP + tq) * a.Tp + (tt0 + p) * 16 + fl;
#pragma unroll
      for (int s = 0; s < NKS; ++s) bt[p][s] = tin ? tw[(size_t)(4 * s) * a.Tp] : 0.0;
    }
    // (retire them before the first DMA: a use of an ordinary load while LDS-DMA
    // is in flight would drain the DMA ring)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // buffer resources: W rows of source j, its rho plane
    const unsigned wbytes = (unsigned)((size_t)KP * a.Fp * sizeof(double));
    const unsigned pbytes = (unsigned)((size_t)a.Tp * a.Fp * sizeof(double));
    const __amdgpu_buffer_rsrc_t rWo = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(a.Wkf_old + (size_t)j * KP * a.Fp), 0, wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rWn = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(a.Wkf_new + (size_t)j * KP * a.Fp), 0, wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rWf = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(a.Wfk_new + (size_t)j * a.Fp * KP), 0, wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(a.hatW + (size_t)j * a.Tp * a.Fp), 0, pbytes, 0x00020000);
    // per-lane byte offsets of this wave's pieces (loop-invariant; the bin
    // step's offset rides in the SGPR soffset)
    constexpr int WPW = CF::WPW;
    static_assert(WPW <= 8, "W pieces per wave");
    unsigned wvo[8];
#pragma unroll
    for (int r = 0; r < WPW; ++r) {
      const int p = wv + NW * r;
      unsigned o = 0;
      if (p < NWO + KP / 8) {          // Wo / Wn: row 8 p' + lane / 8, granule lane % 8
        const int pp = p < NWO ? p : p - NWO, k = 8 * pp + (lane >> 3);
        o = (unsigned)(((size_t)k * a.Fp + 2 * (lane & 7)) * sizeof(double));
      } else if (p < WPI) {            // Wf: LDS position P -> element P ^ swz
        const int P = (p - NWO - KP / 8) * 128 + 2 * lane;
        const int e = P ^ ((((P / KP) >> 2) & 1) << 4);
        o = (unsigned)(e * sizeof(double));
      }
      wvo[r] = o;
    }
    unsigned rvo[TPW][2];
#pragma unroll
    for (int p = 0; p < TPW; ++p) {
      // frame tiles past the last one re-read the last (never used)
      const int tt = min(tt0 + p, a.ntt - 1);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int g = 4 * q + (lane >> 4);
        rvo[p][q] = (unsigned)(((size_t)(tt * 16 + fl) * a.Fp + 2 * g) * sizeof(double));
      }
    }
    auto issue = [&](int c) {   // stage c (bin tile fb + c) into buffer c % NS
      double *st = smem + (c % NS) * SS;
      const int f0 = (fb + c) * 16;
#pragma unroll
      for (int r = 0; r < WPW; ++r) {
        const int p = wv + NW * r;
        // (wave-uniform branches: one resource per call, never a runtime
        // select of a 128-bit resource)
        lds_void_t *d = (lds_void_t *)(st + 128 * p);
        if (p < NWO)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rWo, d, 16, wvo[r], f0 * 8, 0, 0);
        else if (p < NWO + KP / 8)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rWn, d, 16, wvo[r], f0 * 8, 0, 0);
        else if (p < WPI)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rWf, d, 16, wvo[r], f0 * KP * 8, 0, 0);
      }
      double *sr = st + CF::WD + wv * TPW * CF::RD;
#pragma unroll
      for (int p = 0; p < TPW; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rR, (lds_void_t *)(sr + p * CF::RD + 128 * q), 16,
                                                   rvo[p][q], f0 * 8, 0, 0);
    };
    d4 num[TPW][NKC], den[TPW][NKC];
#pragma unroll
    for (int p = 0; p < TPW; ++p)
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) num[p][kc] = den[p][kc] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < NS - 1; ++c)
      if (c < nst) issue(c);
    // lane's LDS read offsets (doubles) inside a stage
    const int fpl = 4 * (fl & 3) + (fl >> 2);   // V-tile bin row permutation (k_tw_contract)
    const int ow = tq * 16 + fpl;   // Wo / Wn: row tq + 4 s at + 64 s
    // Wf element (4 tq + i, 16 kc + fl) sits at (4 tq + i) KP + 16 kc + fl
    // with bit 4 flipped for odd tq: + 16 where the flipped bit was 0 (even kc,
    // or even i at KP = 16, where bit 4 is the row's low bit), - 16 otherwise
    const int s1 = (tq & 1) << 4;
    const int ofp = CF::WF0 + 4 * tq * KP + fl + s1, ofm = ofp - 2 * s1;
    const int orr = CF::WD + wv * TPW * CF::RD + (2 * tq * 16 + fl) * 2;   // granules 2 tq, 2 tq + 1
    for (int c = 0; c < nst; ++c) {
      // this wave's stage c pieces have landed (younger stages may still fly)
      const int ahead = min(NS - 2, nst - 1 - c);
      if (NS >= 3 && ahead >= 1)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CF::LPC < 63 ? CF::LPC : 63) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();   // every wave's stage c is in; stage c - 1 is read
      if (c + NS - 1 < nst) issue(c + NS - 1);
      const double *st = smem + (c % NS) * SS;
#pragma unroll
      for (int p = 0; p < TPW; ++p) {
        if (tt0 + p >= a.ntt) break;  // wave-uniform: no frame tile left
        typedef double dv2 __attribute__((ext_vector_type(2)));
        const dv2 h01 = *(const dv2 *)(st + orr + p * CF::RD);
        const dv2 h23 = *(const dv2 *)(st + orr + p * CF::RD + 32);
        const double h[4] = {h01.x, h01.y, h23.x, h23.y};
        // (this kernel is bound by MFMA + VALU issue, which do not overlap on
        // gfx950: one accumulation chain per V tile, one Newton step on
        // v_rcp_f64, no padding masks -- a bin past F meets W_new's zero rows
        // in the contraction, a frame past T lands in num / den columns
        // k_tw_update never reads, and every padded operand is finite)
        d4 vo = d4{0.0, 0.0, 0.0, 0.0}, vn = vo;
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
          vo = mfma4(st[ow + 64 * s], bt[p][s], vo);
          vn = mfma4(st[CF::WN0 + ow + 64 * s], bt[p][s], vn);
        }
        double r3[4], r4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double vm = vmax_f64(vn[i], kEps);
          double rv = __builtin_amdgcn_rcp(vm);
          rv = fma(fma(-vm, rv, 1.0), rv, rv);
          const double other = vmax_f64(vo[i], kEps);
          r4[i] = other * rv;                // other / V_new
          r3[i] = (h[i] * r4[i]) * r4[i];    // other hat_W / V_new^2, hat_W = rho other
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kc = 0; kc < NKC; ++kc) {
            const bool ev = ((KP == 16 ? i : kc) & 1) == 0;
            const double bw = st[(ev ? ofp : ofm) + i * KP + kc * 16];
            num[p][kc] = mfma4(r3[i], bw, num[p][kc]);
            den[p][kc] = mfma4(r4[i], bw, den[p][kc]);
          }
      }
    }
    const size_t base = ((size_t)slot * a.J + j) * a.Tp;
#pragma unroll
    for (int p = 0; p < TPW; ++p) {
      if (tt0 + p >= a.ntt) break;
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const size_t o = (base + (tt0 + p) * 16 + tq + 4 * m) * a.KP + kc * 16 + fl;
          a.tnum[o] = num[p][kc][m];
          a.tden[o] = den[p][kc][m];
        }
    }
  };
  if constexpr (!BAL) {
    const dim3 bi = xcd_block();   // x: frame-tile group, y: source, z: bin chunk
    const int j = bi.y;
    if (!a.tw_free[j]) return;
    const int fb = bi.z * a.fpc, fe = min(fb + a.fpc, a.nft);
    segment(j, bi.x, fb, fe - fb, bi.z);
  } else {
    // (plain block order: xcd_block()'s placement, consecutive ranges on one
    // XCD, measured the same)
    const int b = blockIdx.x;
    const long long U = tws_steps(a.ts), end = es_lo(b + 1, U, a.ts.nb);
    for (long long s = es_lo(b, U, a.ts.nb); s < end;) {
      const TwSeg g = tws_segment(a.ts, b, s, end);
      s += g.nf;
      const int j = g.u / a.ts.G;
      if (!a.tw_free[j]) continue;   // (the whole block: no barrier is skipped by a part of it)
      segment(j, g.u - j * a.ts.G, g.f0, g.nf, g.slot);
      // The segment's DMA ring is drained (its last bin step waited on
      // vmcnt(0) and issued nothing), and its stores and the next segment's
      // TW loads retire together at that segment's vmcnt(0), before its first
      // DMA.  What is left: every wave has read the last stage before a DMA
      // of the next segment lands in the same buffers.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
}

struct TUArgs {
  double *TW;
  const double *tnum, *tden;
  TwSched ts;   // layout of tnum / tden (fasst_twsched.h; bal == 0: nslot bin chunks)
  int T, Tp, KP, J;
  double omega;
  int kb0[kMaxJ], kb1[kMaxJ], tw_free[kMaxJ];  // rows [kb0, kb1) are updated
  // fused tail (scal non-null): the renormalisation's TW column scale w2
  // (k_renorm_scales) applied after the update to the K[j] live rows, and the
  // restart test's partial sums per block into tpart [slot][ntb]
  const double *scal;
  double *tpart;
  int ntb, K[kMaxJ], soff[kMaxJ];
  // and (FWHt non-null) the next iteration's spectral-update
  // operands from the final TW of its 64 frames: FWHt = (FW TW)^T with the
  // renormalised FW (k_fwh_t's sum), and per-block TW row sums hpart
  // [J][KP][ntb] (k_tw_rowsum's; reduced in k_renorm_tail)
  const double *FW;
  double *FWHt, *hpart;
  // and (with FWHt, twp non-null) the next E-step's TW image (k_tw_image)
  double2 *twp;
  const int *halt;
};
// TW *= (sum_chunks num / max(sum_chunks den, eps))^omega   (:1718-1726)
__global__ __launch_bounds__(256) void k_tw_update(const TUArgs a) {
  HALT_GUARD(a.halt);
  __shared__ double s_r[64][65];
  // (prep: the block's final TW rows [KP][64], padding rows / frames 0)
  extern __shared__ __attribute__((aligned(16))) double s_y[];
  const int j = blockIdx.y, t0 = blockIdx.x * 64;
  // the partials of the block's 64 frames: their unit's own slots, summed in
  // slot order (a frame group is a whole number of 64-frame blocks)
  const int nseg = tws_segments(a.ts, j, t0);
  if (a.scal) {
    // y = fl(fl(TW r) w2): the two roundings of k_tw_update then k_renorm_apply
    const bool fr = a.tw_free[j];
    const double *w2 = a.scal + (size_t)j * (2 + 2 * a.KP) + 2 + a.KP;
    const bool prep = a.FWHt != nullptr;
    if (prep)
      for (int idx = threadIdx.x; idx < a.KP * 64; idx += blockDim.x) s_y[idx] = 0.0;
    // the prep's FW values (4 per thread: all of them at KP = 32) in flight
    // from the start; the source's FW block is in range for every idx < KP^2
    double fwv[4];
    if (prep)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = min((int)threadIdx.x + 256 * e, a.KP * a.KP - 1), k = idx / a.KP, q = idx % a.KP;
        fwv[e] = a.FW[(size_t)j * a.KP * a.KP + (size_t)k * a.KP + q];
      }
    double tsum = 0.0;
    for (int kb = 0; kb < a.K[j]; kb += 64) {
      const int kn = min(64, a.K[j] - kb);
      // the block's TW values in flight before the ratio loads (their two
      // latency chains overlap); raw-buffer loads on the source's plane, an
      // offset past it (elements past kn, frames past Tp) reads 0
      const __amdgpu_buffer_rsrc_t rtw = __builtin_amdgcn_make_buffer_rsrc(
          a.TW + (size_t)j * a.KP * a.Tp, 0, (int)((size_t)a.KP * a.Tp * 8), 0x00020000);
      // (8 per thread: all of them at K <= 32; the rest load in place)
      double xv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int idx = threadIdx.x + 256 * e, kl = idx / 64, tl = idx % 64;
        const unsigned vo = idx < 64 * kn ? (unsigned)(((kb + kl) * a.Tp + t0 + tl) * 8) : 0x7ffffff0u;
        xv[e] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rtw, (int)vo, 0, 0));
      }
      if (fr)
        for (int idx = threadIdx.x; idx < 64 * kn; idx += blockDim.x) {
          const int tl = idx / kn, kl = idx % kn, t = t0 + tl;
          double r = 1.0;
          if (t < a.T) {
            double num = 0.0, den = 0.0;
            for (int c = 0; c < nseg; ++c) {
              const size_t o = (((size_t)c * a.J + j) * a.Tp + t) * a.KP + kb + kl;
              num += a.tnum[o];
              den += a.tden[o];
            }
            const double ratio = num / fmax(den, kEps);
            r = a.omega == 1.0 ? ratio : pow(ratio, a.omega);
          }
          s_r[kl][tl] = r;
        }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int idx = threadIdx.x + 256 * e;
        const int kl = idx / 64, tl = idx % 64, t = t0 + tl, k = kb + kl;
        if (idx < 64 * kn && t < a.T) {
          double *p = a.TW + ((size_t)j * a.KP + k) * a.Tp + t;
          double x = e < 8 ? xv[e < 8 ? e : 0] : *p;
          if (fr && k >= a.kb0[j] && k < a.kb1[j]) x *= s_r[kl][tl];
          const double y = x * w2[k];
          *p = y;
          tsum += y;
          if (prep) s_y[k * 64 + tl] = y;
        }
      }
      __syncthreads();
    }
    tsum = block_sum(tsum, &s_r[0][0]);
    if (threadIdx.x == 0) a.tpart[(size_t)a.soff[j] * a.ntb + blockIdx.x] = tsum;
    if (!prep) return;
    // FW (renormalised by k_renorm_rows, which this launch waits for)
    // transposed into s_r, s_fw[q][k] = FW[k][q], QB rows q at a time (all of
    // them at KP <= 64, the only sizes spectral_update asks this for)
    const int KP = a.KP;
    // the E-step's TW image of the block's (up to) four frame tiles, from the
    // same staged rows (k_tw_image's values: s_y holds the planes' zeros in
    // the padding rows and frames)
    if (a.twp) {
      const int per = (KP / 8) * 64;
      for (int idx = threadIdx.x; idx < 4 * per; idx += blockDim.x) {
        const int w = idx / per, tt = 4 * blockIdx.x + w;
        if (16 * tt < a.Tp)
          tw_image_store(a.twp, tt, j, a.J, KP, idx - w * per,
                         [&](int k, int fl) { return s_y[k * 64 + 16 * w + fl]; });
      }
    }
    double *s_fw = &s_r[0][0];
    const double *gfw = a.FW + (size_t)j * KP * KP;
    const int QB = KP <= 64 ? KP : 32;
    // FWHt^T tiles on the matrix cores: wave w forms frames 16 w .. 16 w + 15,
    // D[k][t] = sum_q FW[k][q] y[q][t] (16x16x4 per 16 k x 4 q); lane (fl,
    // tq) then holds FWHt[16 w + fl][16 kc + tq + 4 i]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, fl = lane & 15, tq = lane >> 4;
    const int tn = min(64, a.Tp - t0);
    d4 d[kMaxKP / 16];
#pragma unroll
    for (int kc = 0; kc < kMaxKP / 16; ++kc) d[kc] = d4{0.0, 0.0, 0.0, 0.0};
    for (int qb = 0; qb < KP; qb += QB) {
      if (QB == KP) {   // (qb = 0: the values loaded at entry, then the rest)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int idx = threadIdx.x + 256 * e;
          if (idx < KP * KP) s_fw[(idx % KP) * KP + idx / KP] = fwv[e];
        }
      }
      for (int idx = threadIdx.x + (QB == KP ? 1024 : 0); idx < QB * KP; idx += blockDim.x) {
        const int k = idx / QB, q = idx % QB;   // (coalesced over q in FW's rows)
        s_fw[q * KP + k] = gfw[(size_t)k * KP + qb + q];
      }
      __syncthreads();
#pragma unroll
      for (int kc = 0; kc < kMaxKP / 16; ++kc)
        if (16 * kc < KP)
          for (int q0 = 0; q0 < QB; q0 += 4)
            d[kc] = mfma4(s_fw[(q0 + tq) * KP + 16 * kc + fl], s_y[(qb + q0 + tq) * 64 + 16 * wv + fl],
                          d[kc]);
      __syncthreads();
    }
    if (16 * wv + fl < tn)
#pragma unroll
      for (int kc = 0; kc < kMaxKP / 16; ++kc)
        if (16 * kc < KP)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            a.FWHt[((size_t)j * a.Tp + t0 + 16 * wv + fl) * KP + 16 * kc + tq + 4 * i] = d[kc][i];
    // row sums over the block's frames (t < T: the padding frames hold 0):
    // one wave per row, lane = frame, the wave's tree
    for (int q = wv; q < KP; q += 4) {
      double h = s_y[q * 64 + lane];
#pragma unroll
      for (int mm = 32; mm > 0; mm >>= 1) h += __shfl_xor(h, mm, 64);
      if (lane == 0) a.hpart[((size_t)j * KP + q) * a.ntb + blockIdx.x] = h;
    }
    return;
  }
  if (!a.tw_free[j]) return;
  // ratios for 64 frames x KP components (coalesced over k), then a
  // transposed, coalesced-over-t read-modify-write of TW
  for (int kb = 0; kb < a.KP; kb += 64) {
    const int kn = min(64, a.KP - kb);
    for (int idx = threadIdx.x; idx < 64 * kn; idx += blockDim.x) {
      const int tl = idx / kn, kl = idx % kn, t = t0 + tl;
      double r = 1.0;
      if (t < a.T) {
        double num = 0.0, den = 0.0;
        for (int c = 0; c < nseg; ++c) {
          const size_t o = (((size_t)c * a.J + j) * a.Tp + t) * a.KP + kb + kl;
          num += a.tnum[o];
          den += a.tden[o];
        }
        const double ratio = num / fmax(den, kEps);
        r = a.omega == 1.0 ? ratio : pow(ratio, a.omega);
      }
      s_r[kl][tl] = r;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * kn; idx += blockDim.x) {
      const int kl = idx / 64, tl = idx % 64, t = t0 + tl, k = kb + kl;
      if (t < a.T && k >= a.kb0[j] && k < a.kb1[j])
        a.TW[((size_t)j * a.KP + k) * a.Tp + t] *= s_r[kl][tl];
    }
    __syncthreads();
  }
}

// ------------------------------------------------- several spectral components
// update_spectral_components (audioModel.py:1479-1727) when source j holds
// several spectral components: they are updated one after the other in the
// reference's key order (block b of every source at step b), each seeing the
// components updated before it.  For block c of source j, with
// V_j = sum of all its components' powers (current parameters), V_c the
// block's own power and hat_W_j the E-step's posterior power:
//   FB: num = ((hat_W_j / max(V_j)^2) max(V_c)) (FW H)^T, den = (max(V_c) /
//       max(V_j)) (FW H)^T (:1513-1575, other = max(V_c): N1)
//   TW: k_tw_contract<BLK> with V_old / V_new of the block and the plane
//       rho_c = hat_W_j / max(V_c_old) (:1634-1727, spec_comp_ind=[k])
// k_multi_prep forms the three planes (rnum, rden, rho_c) of step b from the
// current W (Wkf, all blocks) and TW; at step 0 it also turns the E-step's
// rho_j = hat_W_j / max(V_j) back into hat_W_j in place (the later steps need
// hat_W_j itself, V_j having moved).
struct MPArgs {
  const double *TW, *Wkf;
  double *hatW, *rnum, *rden, *rtw;   // planes [J][Tp][Fp]
  double *rcp, *rpow;                 // LAM: corrPen and max(sum_j V_j, eps) planes
  double *roth;                       // time blobs: max(V_c, eps) at the step's start
  double lambda;
  int F, T, Fp, Tp, KP, J, ntt, tpc, first;
  int on[kMaxJ], kb0[kMaxJ], kb1[kMaxJ];
  const int *halt;
};

// LAM (lambdaCorr > 0, audioModel.py:1484-1507, :1544-1569): the planes
// carry the inter-source correlation penalty of the component's FB step,
//   powers = max(sum_j' V_j', eps) (comp_spat_cmps_powers, summed in source
//   order), minus = max(powers - max(V_j, eps), eps) (the reference's
//   `np.all(minus >= 0)` branch always holds: a sum of non-negative powers is
//   never below one of its terms), cp = lambda minus / max(powers^2, eps)
//   rden = other (1/max(V_j) + cp), rnum = (hat_W/max(V_j)^2 + cp 2 (max(V_j)/powers)) other
// and cp / powers go to two more planes for the FW / TW steps, which use the
// same cp with the component's own power (:1596-1620, :1650-1719).
template <int NKC, bool LAM = false>
__global__ __launch_bounds__(64) void k_multi_prep(const MPArgs a) {
  HALT_GUARD(a.halt);
  constexpr int NKS = 4 * NKC;
  const int lane = threadIdx.x, fl = lane & 15, tq = lane >> 4;
  const int j = blockIdx.y;
  if (!a.on[j]) return;
  const int f0 = blockIdx.x * 16, f = f0 + fl;
  double wj[NKS], wc[NKS];   // B operands of the V tiles: W[k = tq + 4 s][f]
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const int k = tq + 4 * s;
    const double w = a.Wkf[((size_t)j * a.KP + k) * a.Fp + f];
    wj[s] = w;
    wc[s] = k >= a.kb0[j] && k < a.kb1[j] ? w : 0.0;
  }
  const size_t pj = (size_t)j * a.Tp * a.Fp;
  const int tb = blockIdx.z * a.tpc, te = min(tb + a.tpc, a.ntt);
  for (int tt = tb; tt < te; ++tt) {
    const int t0 = tt * 16;
    const double *tw = a.TW + ((size_t)j * a.KP + tq) * a.Tp + t0 + fl;
    d4 vj = d4{0.0, 0.0, 0.0, 0.0}, vc = vj, vall = vj;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      const double h = tw[(size_t)(4 * s) * a.Tp];
      vj = mfma4(h, wj[s], vj);
      vc = mfma4(h, wc[s], vc);
    }
    if constexpr (LAM) {
      for (int jj = 0; jj < a.J; ++jj) {   // sum_j' V_j' in source order
        d4 v = d4{0.0, 0.0, 0.0, 0.0};
        if (jj == j) {
          v = vj;
        } else {
          const double *twj = a.TW + ((size_t)jj * a.KP + tq) * a.Tp + t0 + fl;
          const double *wk = a.Wkf + ((size_t)jj * a.KP + tq) * a.Fp + f;
          for (int s = 0; s < NKS; ++s)
            v = mfma4(twj[(size_t)(4 * s) * a.Tp], wk[(size_t)(4 * s) * a.Fp], v);
        }
        vall += v;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + tq + 4 * i;
      const size_t o = pj + (size_t)t * a.Fp + f;
      if (t >= a.T || f >= a.F) {
        a.rnum[o] = a.rden[o] = a.rtw[o] = 0.0;
        if constexpr (LAM) a.rcp[o] = a.rpow[o] = 0.0;
        if (a.roth) a.roth[o] = 0.0;
        continue;
      }
      const double sj = fmax(vj[i], kEps), sc = fmax(vc[i], kEps);
      double hw;
      if (a.first) {
        hw = a.hatW[o] * sj;   // rho_j max(V_j) (the E-step stored rho_j)
        a.hatW[o] = hw;
      } else {
        hw = a.hatW[o];
      }
      if constexpr (LAM) {
        const double pw = fmax(vall[i], kEps);
        const double minus = fmax(pw - sj, kEps);
        const double cp = a.lambda * minus / fmax(pw * pw, kEps);
        a.rden[o] = sc * (1.0 / sj + cp);
        a.rnum[o] = (hw / (sj * sj) + cp * (2.0 * (sj / pw))) * sc;
        a.rcp[o] = cp;
        a.rpow[o] = pw;
      } else {
        a.rnum[o] = (hw / (sj * sj)) * sc;
        a.rden[o] = sc * (1.0 / sj);
      }
      a.rtw[o] = hw / sc;
      if (a.roth) a.roth[o] = sc;
    }
  }
}

// ---------------------------------------------------------------- time blobs
// A spectral component with time blobs (TB, audioModel.py:430-498) has
// H = TW TB.  Its factor TW ("TWs", block rows x L) and TB (L x T) live in the
// slot buffer tb[j][b] (tb_layout, fasst_device.h) and the block's rows of the model TW hold
// H, so every other kernel (E-step, FB / FW / TW contractions, Wiener) reads
// H unchanged.  Both updates reuse the block's TW contraction, which leaves
// G = W^T R over f per frame in tnum / tden (W = FB FW of the block):
//   TW step (:1665-1691): num = G TB^T, den likewise        (k_tb_tw_red)
//   TB step (:1931-1978): num = TWs^T G, with R's ratio hat_W / max(V^2, eps)
//                         (k_tw_contract<TBQ>, then k_tb_tb_upd)
// the reference's (W TWs)^T R reassociated; H is rebuilt after each (k_tb_h).
struct TBArgs {
  double *tb[kMaxJ];   // the step's slot buffer per source (null: no time blobs)
  int L[kMaxJ], kb0[kMaxJ], kbw[kMaxJ];
  double *TW;
  const double *tnum, *tden;   // [nsplit][J][Tp][KP] of k_tw_contract
  int T, Tp, KP, J, nsplit;
  double omega;
  // iter >= 0 (renormalisation): a halt raised in this same iteration does not
  // stop the kernel (the host reads a consistent TWs / TB), an earlier one does
  const int *flags;
  int iter;
  const int *halt;
};

// TW step: num[k][l] = sum_t G_num[t][k] TB[l][t] (chunks summed first), one
// block per (blob, 16 rows, source)
__global__ __launch_bounds__(256) void k_tb_tw_red(const TBArgs a) {
  if (tb_halted(a.halt, a.flags, a.iter)) return;
  __shared__ double s_red[256];
  const int l = blockIdx.x, k0 = blockIdx.y * 16, j = blockIdx.z;
  if (!a.tb[j] || l >= a.L[j] || k0 >= a.kbw[j]) return;
  const int L = a.L[j], kbw = a.kbw[j], nk = min(16, kbw - k0);
  const TBLayout o = tb_layout(kbw, L, a.Tp);
  const double *TB = a.tb[j] + o.tb + (size_t)l * a.Tp;
  double num[16], den[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) num[i] = den[i] = 0.0;
  for (int t = threadIdx.x; t < a.T; t += blockDim.x) {
    const double bl = TB[t];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i < nk) {
        double sn = 0.0, sd = 0.0;
        for (int c = 0; c < a.nsplit; ++c) {
          const size_t q = (((size_t)c * a.J + j) * a.Tp + t) * a.KP + a.kb0[j] + k0 + i;
          sn += a.tnum[q];
          sd += a.tden[q];
        }
        num[i] += sn * bl;
        den[i] += sd * bl;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < nk) {
      const double rn = block_sum(num[i], s_red), rd = block_sum(den[i], s_red);
      if (threadIdx.x == 0) {
        a.tb[j][o.num + (size_t)(k0 + i) * L + l] = rn;
        a.tb[j][o.den + (size_t)(k0 + i) * L + l] = rd;
      }
    }
  }
}

// TWs *= (num / max(den, eps))^omega   (:1718-1726)
__global__ __launch_bounds__(256) void k_tb_tw_apply(const TBArgs a) {
  if (tb_halted(a.halt, a.flags, a.iter)) return;
  const int j = blockIdx.x;
  if (!a.tb[j]) return;
  const TBLayout o = tb_layout(a.kbw[j], a.L[j], a.Tp);
  double *p = a.tb[j];
  for (int i = threadIdx.x; i < a.kbw[j] * a.L[j]; i += blockDim.x) {
    const double r = p[o.num + i] / fmax(p[o.den + i], kEps);
    p[o.tws + i] *= a.omega == 1.0 ? r : pow(r, a.omega);
  }
}

// TB step: num[l][t] = sum_k TWs[k][l] G_num[t][k], TB *= (num / max(den,
// eps))^omega (:1974-1977); 64 frames per block, accumulators in LDS
__global__ __launch_bounds__(64) void k_tb_tb_upd(const TBArgs a) {
  if (tb_halted(a.halt, a.flags, a.iter)) return;
  extern __shared__ double s_tb[];
  const int j = blockIdx.y;
  if (!a.tb[j]) return;
  const int L = a.L[j], kbw = a.kbw[j], tid = threadIdx.x;
  const TBLayout o = tb_layout(kbw, L, a.Tp);
  double *s_tw = s_tb, *s_num = s_tb + kbw * L, *s_den = s_num + 64 * L;
  for (int i = tid; i < kbw * L; i += 64) s_tw[i] = a.tb[j][o.tws + i];
  for (int l = 0; l < L; ++l) s_num[l * 64 + tid] = s_den[l * 64 + tid] = 0.0;
  __syncthreads();
  const int t = blockIdx.x * 64 + tid;
  if (t >= a.T) return;
  for (int k = 0; k < kbw; ++k) {
    double sn = 0.0, sd = 0.0;
    for (int c = 0; c < a.nsplit; ++c) {
      const size_t q = (((size_t)c * a.J + j) * a.Tp + t) * a.KP + a.kb0[j] + k;
      sn += a.tnum[q];
      sd += a.tden[q];
    }
    for (int l = 0; l < L; ++l) {
      const double w = s_tw[k * L + l];
      s_num[l * 64 + tid] += w * sn;
      s_den[l * 64 + tid] += w * sd;
    }
  }
  double *TB = a.tb[j] + o.tb;
  for (int l = 0; l < L; ++l) {
    const double r = s_num[l * 64 + tid] / fmax(s_den[l * 64 + tid], kEps);
    TB[(size_t)l * a.Tp + t] *= a.omega == 1.0 ? r : pow(r, a.omega);
  }
}

// H = TWs TB into the block's rows of TW (padding frames stay zero)
__global__ __launch_bounds__(256) void k_tb_h(const TBArgs a) {
  if (tb_halted(a.halt, a.flags, a.iter)) return;
  extern __shared__ double s_tw[];
  const int j = blockIdx.y;
  if (!a.tb[j]) return;
  const int L = a.L[j], kbw = a.kbw[j];
  const TBLayout o = tb_layout(kbw, L, a.Tp);
  for (int i = threadIdx.x; i < kbw * L; i += blockDim.x) s_tw[i] = a.tb[j][o.tws + i];
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.Tp) return;
  const double *TB = a.tb[j] + o.tb;
  for (int k = 0; k < kbw; ++k) {
    double h = 0.0;
    for (int l = 0; l < L; ++l) h += s_tw[k * L + l] * TB[(size_t)l * a.Tp + t];
    a.TW[((size_t)j * a.KP + a.kb0[j] + k) * a.Tp + t] = t < a.T ? h : 0.0;
  }
}

// rho_j = hat_W_j / max(V_j, eps) into the [J][Tp][Fp] plane the spectral
// update reads, from a caller's hat_W [J][F][T] (update_spectral_components
// called on its own); V_j from the current parameters (Wkf = FB.FW)
__global__ void k_rho_from_hatw(const double *__restrict__ hw, const double *__restrict__ Wkf,
                                const double *__restrict__ TW, double *__restrict__ rho, int F,
                                int T, int Fp, int Tp, int KP) {
  const int f = blockIdx.x * 64 + (threadIdx.x & 63), t = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int j = blockIdx.z;
  if (f >= F || t >= T) return;
  double v = 0.0;
  for (int k = 0; k < KP; ++k) v += Wkf[((size_t)j * KP + k) * Fp + f] * TW[((size_t)j * KP + k) * Tp + t];
  rho[((size_t)j * Tp + t) * Fp + f] = hw[((size_t)j * F + f) * T + t] / fmax(v, kEps);
}

// ---------------------------------------------------------------- host side
// The spectral update's template arms, chosen from the model in one place:
// `f` receives NKC = KP / 16 as a std::integral_constant<int, 1 | 2 | 4 | 8>
// (launches and occupancy queries alike), and LAM as a std::bool_constant.
template <class F>
static void nkc_dispatch(const fasst_ctx *c, F &&f) {
  switch (c->KP / 16) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;   // KP = 128
  }
}

template <class F>
static void lam_dispatch(const fasst_ctx *c, F &&f) {
  if (c->lambda > 0.0)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// frame tiles per wave of the TW contraction: KP = 128 keeps one (its
// numerator / denominator tiles alone fill 128 VGPRs)
template <int NKC>
constexpr int tpw_for() { return NKC > 4 ? 1 : kTPW; }

// k_tw_contract_lds's shape: 8 waves per block, one frame tile per wave, two
// LDS stages (C3 same-box A/B, k_tw_contract 0.395 ms: NW x TPW x NS = 8 x 1 x
// 2 0.378, 4 x 2 x 2 0.379, 4 x 1 x 3 0.396, 4 x 2 x 3 0.437 ms; the other
// shapes and the register-operand k_tw_contract of rounds 1-4 were deleted
// after the A/B)
template <int NKC>
using TwlShape = TwlCfg<NKC, 8, 1, 2>;

// resident k_tw_contract_lds blocks per CU (bal: of its balanced form), its
// frame-tile groups (units) and the frame tiles of one
int twl_occupancy(const fasst_ctx *c, bool bal, int *units, int *group_tiles) {
  int n = 0;
  nkc_dispatch(c, [&](auto k) {
    using CF = TwlShape<decltype(k)::value>;
    const void *fn = bal ? (const void *)k_tw_contract_lds<CF, true> : (const void *)k_tw_contract_lds<CF>;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CF::smem);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, CF::NT, CF::smem) != hipSuccess) n = 1;
    *group_tiles = CF::NW_ * CF::TPW_;
    *units = (c->ntt + *group_tiles - 1) / *group_tiles;
  });
  return std::max(1, n);
}

// resident k_fb_contract waves per CU
int contract_occupancy(const fasst_ctx *c) {
  int n = 1;
  hipError_t e = hipSuccess;
  nkc_dispatch(c, [&](auto k) {
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_fb_contract<decltype(k)::value, kFPW>,
                                                     64, 0);
  });
  return e == hipSuccess ? std::max(1, n) : 1;
}

// dynamic LDS of the kernels that stage FW ([KP][KP] when KP <= 64) next to
// `rest` doubles
static size_t fw_lds(const fasst_ctx *c, int rest) {
  return (size_t)((c->KP > 64 ? 0 : c->KP * c->KP) + rest) * sizeof(double);
}

// Dynamic-LDS ceilings of the kernels whose launches may pass the 64 KB
// default, raised once per model configuration to the most any structure asks
// of them (not per iteration: the sizes depend only on the model shape, and
// a ceiling above a launch's own size costs nothing)
int spectral_lds_limits() {
  struct L {
    const void *f;
    size_t bytes;
  };
  const L lim[] = {
      {(const void *)k_fw_reduce, (size_t)3 * 32 * kMaxKP * sizeof(double)},
      {(const void *)k_fwh_t<true>, (size_t)(16 + 64) * kMaxKP * sizeof(double)},
  };
  for (const L &l : lim)
    if (hipFuncSetAttribute(l.f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes) != hipSuccess) {
      set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", l.bytes);
      return FASST_ERR_DEVICE;
    }
  return FASST_OK;
}

// W = FB.FW of the current parameters into wkf ([KP][Fp]) and, unless null,
// wfk ([Fp][KP]), on stream s
static void launch_w(fasst_ctx *c, double *wkf, double *wfk, hipStream_t s) {
  (c->KP > 64 ? k_w_from_fb<true> : k_w_from_fb<false>)<<<dim3(c->nft, c->J), 256,
                fw_lds(c, 16 * (c->KP + 1)), s>>>(c->FB.p, c->FW.p, wkf, wfk, c->J, c->Fp, c->KP,
                                                  c->halt);
}

int launch_w_old(fasst_ctx *c) {
  prof_begin(c, KW);
  launch_w(c, c->Wkf.p, nullptr, c->stream);
  prof_end(c, KW);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// Time-blob arguments of step b (only_j as multi_step); which = 0: every
// block with time blobs, 1: those whose TW is free, 2: those whose TB is free
static TBArgs tb_args(const fasst_ctx *c, int b, int only_j, int which, double omega) {
  TBArgs a{};
  for (int j = 0; j < kMaxJ; ++j) {
    bool on = j < c->J && b < c->nblk[j] && c->tbl[j][b] > 0 && (only_j < 0 || j == only_j);
    if (on && which == 1) on = c->btw[j][b] != 0;
    if (on && which == 2) on = c->btb[j][b] != 0;
    a.tb[j] = on ? c->tb[j][b].p : nullptr;
    a.L[j] = on ? c->tbl[j][b] : 0;
    a.kb0[j] = on ? c->kb[j][b] : 0;
    a.kbw[j] = on ? c->kb[j][b + 1] - c->kb[j][b] : 0;
  }
  a.TW = c->TW.p;
  a.tnum = c->tnum.p;
  a.tden = c->tden.p;
  a.T = c->T;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.J = c->J;
  a.nsplit = c->nsplit_t;
  a.omega = omega;
  a.flags = nullptr;
  a.iter = -1;
  a.halt = c->halt;
  return a;
}

static bool tb_any(const TBArgs &a, int *lmax, int *kwmax) {
  bool any = false;
  *lmax = *kwmax = 0;
  for (int j = 0; j < kMaxJ; ++j)
    if (a.tb[j]) {
      any = true;
      *lmax = std::max(*lmax, a.L[j]);
      *kwmax = std::max(*kwmax, a.kbw[j]);
    }
  return any;
}

static int launch_tb_h(fasst_ctx *c, const TBArgs &a) {
  int lmax, kwmax;
  if (!tb_any(a, &lmax, &kwmax)) return FASST_OK;
  k_tb_h<<<dim3((c->Tp + 255) / 256, c->J), 256, (size_t)kwmax * lmax * sizeof(double),
           c->stream>>>(a);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// the renormalisation's refresh of every block with time blobs (after
// k_tb_renorm rescaled TWs / TB; iter as TBArgs::iter)
int launch_tb_refresh(fasst_ctx *c, int iter) {
  for (int b = 0; b < c->maxblk; ++b) {
    TBArgs ta = tb_args(c, b, -1, 0, 1.0);
    ta.flags = c->flags.p;
    ta.iter = iter;
    if (int st = launch_tb_h(c, ta)) return st;
  }
  return FASST_OK;
}

// H = TW TB into the rows of block b of source j (fasst_set_tb)
int launch_tb_set(fasst_ctx *c, int j, int b) {
  return launch_tb_h(c, tb_args(c, b, j, 0, 1.0));
}

// What one spectral step updates: the columns [kb0, kb1) of every source that
// is `on`, under the priors of those columns.  b < 0: every source whole,
// under its source-level priors (spectral_update); otherwise block b of every
// source that has one (only_j < 0) or of source only_j alone, under the
// block's priors (multi_step).  A discrete-state TW (twc) is never updated by
// the contraction: tw is off for it in both forms.
struct Step {
  int on[kMaxJ], kb0[kMaxJ], kb1[kMaxJ], fb[kMaxJ], fw[kMaxJ], tw[kMaxJ];
  bool any_fw;
};

static Step step_of(const fasst_ctx *c, int b = -1, int only_j = -1) {
  Step s{};
  for (int j = 0; j < c->J; ++j) {
    const bool whole = b < 0;
    if (!whole && !(b < c->nblk[j] && (only_j < 0 || j == only_j))) continue;
    s.on[j] = 1;
    s.kb0[j] = whole ? 0 : c->kb[j][b];
    s.kb1[j] = whole ? c->K[j] : c->kb[j][b + 1];
    s.fb[j] = (whole ? c->fb_free[j] : c->bfb[j][b]) != 0;
    s.fw[j] = (whole ? c->fw_free[j] : c->bfw[j][b]) != 0;
    s.tw[j] = (whole ? c->tw_free[j] : c->btw[j][b]) && !c->twc[j];
    s.any_fw |= s.fw[j] != 0;
  }
  return s;
}

// The kernel-argument structs of a GEM iteration, one builder each: value-
// initialised, every field that follows from the context (buffers, shapes,
// chunking, halt) and from the step set here.  What a caller adds is named at
// each builder; a pointer left out stays null.

// the caller adds the planes rnum / rden / rtw / rcp / rpow / roth and `first`
static MPArgs mp_args(const fasst_ctx *c, const Step &s) {
  MPArgs a{};
  a.TW = c->TW.p;
  a.Wkf = c->Wkf.p;
  a.hatW = c->hatW.p;
  a.lambda = c->lambda;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.J = c->J;
  a.ntt = c->ntt;
  a.tpc = c->tpc_b;
  a.halt = c->halt;
  for (int j = 0; j < kMaxJ; ++j) {
    a.on[j] = s.on[j];
    a.kb0[j] = s.kb0[j];
    a.kb1[j] = s.kb1[j];
  }
  return a;
}

// the caller adds the ratio plane hatW and, for the DEN form, hatW2 and bden
static BArgs b_args(const fasst_ctx *c, const Step &s) {
  BArgs a{};
  a.TW = c->TW.p;
  a.Wkf = c->Wkf.p;
  a.FWHt = c->FWHt.p;
  a.bnum = c->bnum.p;
  a.halt = c->halt;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.J = c->J;
  a.ntt = c->ntt;
  a.nft = c->nft;
  a.tpc = c->tpc_b;
  for (int j = 0; j < kMaxJ; ++j) a.fb_free[j] = s.fb[j];
  return a;
}

// the caller adds bden (the contracted denominator) and the fused tail's pmax
static UArgs u_args(const fasst_ctx *c, const Step &s, double omega) {
  UArgs a{};
  a.FB = c->FB.p;
  a.FW = c->FW.p;
  a.bnum = c->bnum.p;
  a.hsum = c->hsum.p;
  a.Wkf_new = c->Wkf_new.p;
  a.Wfk_new = c->Wfk_new.p;
  a.halt = c->halt;
  a.F = c->F;
  a.Fp = c->Fp;
  a.KP = c->KP;
  a.J = c->J;
  a.nchunk = c->nchunk_b;
  a.omega = omega;
  for (int j = 0; j < kMaxJ; ++j) {
    a.kb0[j] = s.kb0[j];
    a.kb1[j] = s.kb1[j];
    a.fb_free[j] = s.fb[j];
  }
  return a;
}

// the caller adds the ratio plane hatW and, for LAM, the planes cp / pw
static FWArgs fw_args(const fasst_ctx *c, const Step &s, double omega) {
  FWArgs a{};
  a.TW = c->TW.p;
  a.TWt = c->TWt.p;
  a.Wkf_old = c->Wkf.p;
  a.Wkf_mid = c->Wkf_new.p;
  a.FB = c->FB.p;
  a.gnum = c->bnum.p;
  a.gden = c->gden.p;
  a.pnum = c->pnum.p;
  a.pden = c->pden.p;
  a.FW = c->FW.p;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.J = c->J;
  a.ntt = c->ntt;
  a.tpc = c->tpc_b;
  a.nchunk = c->nchunk_b;
  a.fpc = fw_fpc(c);
  a.nfc = (c->F + a.fpc - 1) / a.fpc;
  a.omega = omega;
  a.halt = c->halt;
  for (int j = 0; j < kMaxJ; ++j) {
    a.K[j] = j < c->J ? c->K[j] : 0;
    a.fw_free[j] = s.fw[j];
    a.kb0[j] = s.kb0[j];
    a.kb1[j] = s.kb1[j];
  }
  return a;
}

// The layout of tnum / tden in the update at hand: k_tw_contract_lds's
// schedule on the single-component path, the static bin split of
// k_tw_contract<BLK> on the multi-block one
static TwSched tw_layout(const fasst_ctx *c) {
  if (!c->multi) return c->twsched;
  TwSched s{};
  s.nslot = c->nsplit_t;
  return s;
}

// the caller adds the ratio plane hatW and, for LAM / TBQ, the planes cp / pw / oth
static TArgs t_args(const fasst_ctx *c, const Step &s, double omega) {
  TArgs a{};
  a.TW = c->TW.p;
  a.Wkf_old = c->Wkf.p;
  a.Wkf_new = c->Wkf_new.p;
  a.Wfk_new = c->Wfk_new.p;
  a.tnum = c->tnum.p;
  a.tden = c->tden.p;
  a.halt = c->halt;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.J = c->J;
  a.nft = c->nft;
  a.ntt = c->ntt;
  a.fpc = c->fpc_t;
  a.ts = tw_layout(c);
  a.omega = omega;
  for (int j = 0; j < kMaxJ; ++j) {
    a.tw_free[j] = s.tw[j];
    a.kb0[j] = s.kb0[j];
    a.kb1[j] = s.kb1[j];
  }
  return a;
}

// tbw (multi_step: the step's blocks whose TW goes through time blobs, null
// otherwise): those rows are k_tb_tw_red / _apply's, not k_tw_update's.  The
// caller adds the fused tail's scal / tpart / ntb / FWHt / hpart
static TUArgs tu_args(const fasst_ctx *c, const Step &s, double omega, const TBArgs *tbw = nullptr) {
  TUArgs a{};
  a.TW = c->TW.p;
  a.tnum = c->tnum.p;
  a.tden = c->tden.p;
  a.FW = c->FW.p;
  a.halt = c->halt;
  a.T = c->T;
  a.Tp = c->Tp;
  a.KP = c->KP;
  a.J = c->J;
  a.ts = tw_layout(c);
  a.omega = omega;
  for (int j = 0; j < kMaxJ; ++j) {
    a.kb0[j] = s.kb0[j];
    a.kb1[j] = s.kb1[j];
    a.tw_free[j] = s.tw[j] && !(tbw && tbw->tb[j]);
    a.K[j] = j < c->J ? c->K[j] : 0;
    a.soff[j] = j < c->J ? c->soff[j] : 0;
  }
  return a;
}

// the scales and the FB / mixing / FW rescale, after k_fb_update: on the side
// stream beside the TW contraction; ev_scales gates k_tw_update, ev_rows the
// iteration's end
static int launch_tail_side(fasst_ctx *c) {
  hipStream_t side = c->aux;
  FASST_HIP(hipEventRecord(c->ev_tail, c->stream));
  FASST_HIP(hipStreamWaitEvent(c->aux, c->ev_tail, 0));
  if (int st = launch_renorm_side(c, side)) return st;
  // the next iteration's W (the TW contraction still reads Wkf)
  prof_begin(c, KW, side);
  launch_w(c, c->Wkf_next.p, nullptr, side);
  prof_end(c, KW, side);
  FASST_LAUNCH_CHECK();
  FASST_HIP(hipEventRecord(c->ev_rows, c->aux));
  return FASST_OK;
}

// The launches of the spectral update.  `timed`: with the per-kernel timing
// events (spectral_update's launches record them, multi_step's none).

// k_fb_contract, with DEN the contracted denominator of the multi-block update
static void launch_fb_contract(fasst_ctx *c, const BArgs &b, bool den, bool timed) {
  const dim3 g((c->nft + kFPW - 1) / kFPW, c->J, c->nchunk_b);
  if (timed) prof_begin(c, KFBC);
  nkc_dispatch(c, [&](auto n) {
    constexpr int NKC = decltype(n)::value;
    if (den)
      k_fb_contract<NKC, kFPW, true><<<g, 64, 0, c->stream>>>(b);
    else
      k_fb_contract<NKC, kFPW><<<g, 64, 0, c->stream>>>(b);
  });
  if (timed) prof_end(c, KFBC);
}

// k_tw_contract_lds, the TW contraction of the single-component path
static void launch_tw_contract_lds(fasst_ctx *c, const TArgs &t) {
  prof_begin(c, KTWC);
  nkc_dispatch(c, [&](auto n) {
    using CF = TwlShape<decltype(n)::value>;
    const int g = (c->ntt + CF::NW_ * CF::TPW_ - 1) / (CF::NW_ * CF::TPW_);
    if (t.ts.bal)
      k_tw_contract_lds<CF, true><<<t.ts.nb, CF::NT, CF::smem, c->stream>>>(t);
    else
      k_tw_contract_lds<CF><<<dim3(g, c->J, c->nsplit_t), CF::NT, CF::smem, c->stream>>>(t);
  });
  prof_end(c, KTWC);
}

// k_tw_contract<BLK>, the TW contraction of one block (multi_step); tbq: its
// TB-step form
static void launch_tw_contract_blk(fasst_ctx *c, const TArgs &t, bool tbq) {
  nkc_dispatch(c, [&](auto n) {
    constexpr int NKC = decltype(n)::value, TPW = tpw_for<NKC>();
    const dim3 g((c->ntt + TPW - 1) / TPW, c->J, c->nsplit_t);
    lam_dispatch(c, [&](auto l) {
      constexpr bool LAM = decltype(l)::value;
      if (tbq)
        k_tw_contract<NKC, TPW, true, LAM, true><<<g, 64, 0, c->stream>>>(t);
      else
        k_tw_contract<NKC, TPW, true, LAM><<<g, 64, 0, c->stream>>>(t);
    });
  });
}

// The fused-tail pointers of k_fb_update / k_tw_update are null or the
// context's own buffers; anything else is refused here, on the host, before a
// kernel could dereference it (an uninitialised argument struct on the
// multi-block path once sent garbage pointers to the device)
static int check_tail_args(const fasst_ctx *c, const UArgs &u, const TUArgs &tu) {
  const bool ok_u = !u.pmax || u.pmax == c->rpmax2.p;
  const bool ok_t = !tu.scal || (tu.scal == c->rscal.p && tu.tpart == c->rtpart2.p &&
                                 (!tu.FWHt || (tu.FWHt == c->FWHt.p && tu.hpart == c->hpart.p &&
                                               tu.FW == c->FW.p)));
  const bool ok_i = !tu.twp || (tu.FWHt && tu.twp == c->twp.p &&
                                c->twp.n == (size_t)c->ntt * c->J * (c->KP / 8) * 64);
  if (ok_u && ok_t && ok_i) return FASST_OK;
  set_error("internal: fused renormalisation arguments do not point at the context's buffers");
  return FASST_ERR_SHAPE;
}

// k_fb_update, after check_tail_args on the step's two update structs (the
// only launch of k_fb_update; k_tw_update's is launch_tw_update)
static int launch_fb_update(fasst_ctx *c, const UArgs &u, const TUArgs &tu, bool timed) {
  if (int st = check_tail_args(c, u, tu)) return st;
  if (timed) prof_begin(c, KFBU);
  (c->KP > 64 ? k_fb_update<true> : k_fb_update<false>)<<<dim3(c->nft, c->J), 256,
                fw_lds(c, 16 * (c->KP + 1) + c->KP + 16 * (c->KP + 1)),
                c->stream>>>(u);
  if (timed) prof_end(c, KFBU);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// k_tw_update; with the fused tail's FWHt it stages the block's TW rows in LDS
static int launch_tw_update(fasst_ctx *c, const UArgs &u, const TUArgs &tu, bool timed) {
  if (int st = check_tail_args(c, u, tu)) return st;
  if (timed) prof_begin(c, KTWU);
  k_tw_update<<<dim3(c->ntb, c->J), 256, tu.FWHt ? (size_t)c->KP * 64 * sizeof(double) : 0,
                c->stream>>>(tu);
  if (timed) prof_end(c, KTWU);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// The FW update (:1578-1631) of the step's free FW, between its FB and TW
// updates: W_new = FB_new FW_old from k_fb_update is the V_mid operand
// (blk: the component's own V), then W_new is rebuilt with FW_new
static int launch_fw_update(fasst_ctx *c, const FWArgs &w, bool blk, bool timed) {
  if (timed) prof_begin(c, KFWU);
  const dim3 gc(c->nft, c->J, c->nchunk_b);
  nkc_dispatch(c, [&](auto n) {
    constexpr int NKC = decltype(n)::value;
    if (!blk)
      k_fw_contract<NKC><<<gc, 64, 0, c->stream>>>(w);
    else
      lam_dispatch(c, [&](auto l) {
        k_fw_contract<NKC, true, decltype(l)::value><<<gc, 64, 0, c->stream>>>(w);
      });
  });
  const size_t lds = (size_t)3 * w.fpc * c->KP * sizeof(double);   // (ceiling: spectral_lds_limits)
  k_fw_reduce<<<dim3(w.nfc, c->J), 256, lds, c->stream>>>(w);
  k_fw_final<<<c->J, 256, 0, c->stream>>>(w);
  launch_w(c, c->Wkf_new.p, c->Wfk_new.p, c->stream);
  if (timed) prof_end(c, KFWU);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// source j's TW step is the discrete-state one (fasst_set_tw_constr)
static inline bool twc_on(const fasst_ctx *c, int j) { return c->twc[j] && c->tw_free[j]; }

// The discrete-state TW step (:1728-1928) of the marked sources, after the
// FB / FW updates and before W_new replaces W: k_tw_statediv, k_tw_decode.
// plane_is_hatw: c->hatW holds hat_W (multi_step's first k_multi_prep turned
// every source's rho into hat_W in place), else the E-step's rho
static int launch_tw_constr(fasst_ctx *c, double omega, bool plane_is_hatw) {
  bool any = false;
  for (int j = 0; j < c->J; ++j) any |= twc_on(c, j);
  if (!any) return FASST_OK;
  prof_begin(c, KTWD);
  int st = launch_tw_statediv(c, omega, plane_is_hatw);
  prof_end(c, KTWD);
  if (st) return st;
  prof_begin(c, KTWV);
  st = launch_tw_decode(c);
  prof_end(c, KTWV);
  return st;
}

// Spectral update of a model with several spectral components on some source
// (see k_multi_prep): step b updates block b of every source that has one
// (FB, then TW), all launches on c->stream; W = FB FW of the step's result
// becomes the next step's current W.
// one step: block b of every source that has one (only_j < 0), or of source
// only_j alone (lambdaCorr > 0: the penalty couples the sources, so the
// components go one at a time in the reference's key order)
static int multi_step(fasst_ctx *c, double omega, int b, int only_j) {
  const int J = c->J;
  const size_t plane = (size_t)J * c->Tp * c->Fp;
  const Step s = step_of(c, b, only_j);
  const TBArgs tbw = tb_args(c, b, only_j, 1, omega), tbb = tb_args(c, b, only_j, 2, omega);
  int lmax, kwmax;
  const bool any_tbb = tb_any(tbb, &lmax, &kwmax);
  MPArgs mp = mp_args(c, s);
  mp.rnum = c->mplanes.p;
  mp.rden = c->mplanes.p + plane;
  mp.rtw = c->mplanes.p + 2 * plane;
  mp.rcp = c->mplanes.p + 3 * plane;
  mp.rpow = c->mplanes.p + 4 * plane;
  if (any_tbb) mp.roth = c->mplanes.p + 5 * plane;
  mp.first = b == 0;
  BArgs bb = b_args(c, s);
  bb.hatW = mp.rnum;
  bb.hatW2 = mp.rden;
  bb.bden = c->bden.p;
  UArgs u = u_args(c, s, omega);   // (pmax null: no fused-tail statistics on this path)
  u.bden = c->bden.p;
  TArgs t = t_args(c, s, omega);
  t.hatW = mp.rtw;
  t.cp = mp.rcp;
  t.pw = mp.rpow;
  const TUArgs tu = tu_args(c, s, omega, &tbw);   // (scal null: the plain TW update)
  nkc_dispatch(c, [&](auto n) {
    lam_dispatch(c, [&](auto l) {
      k_multi_prep<decltype(n)::value, decltype(l)::value>
          <<<dim3(c->nft, J, c->nchunk_b), 64, 0, c->stream>>>(mp);
    });
  });
  launch_fb_contract(c, bb, true, false);
  FASST_LAUNCH_CHECK();
  if (int st = launch_fb_update(c, u, tu, false)) return st;
  if (s.any_fw) {   // V_mid = (FB_new FW) H of the component
    FWArgs w = fw_args(c, s, omega);
    w.hatW = mp.rtw;
    w.cp = mp.rcp;
    w.pw = mp.rpow;
    if (int st = launch_fw_update(c, w, true, false)) return st;
  }
  launch_tw_contract_blk(c, t, false);
  FASST_LAUNCH_CHECK();
  if (int st = launch_tw_update(c, u, tu, false)) return st;
  if (tb_any(tbw, &lmax, &kwmax)) {   // TW with time blobs (:1665-1691)
    k_tb_tw_red<<<dim3(lmax, (kwmax + 15) / 16, J), 256, 0, c->stream>>>(tbw);
    k_tb_tw_apply<<<J, 256, 0, c->stream>>>(tbw);
    FASST_LAUNCH_CHECK();
    if (int st = launch_tb_h(c, tbw)) return st;
  }
  if (tb_any(tbb, &lmax, &kwmax)) {   // TB (:1931-1978) with the updated H
    TArgs t2 = t;
    t2.hatW = c->hatW.p;
    t2.oth = mp.roth;
    for (int j = 0; j < kMaxJ; ++j) t2.tw_free[j] = tbb.tb[j] != nullptr;
    launch_tw_contract_blk(c, t2, true);
    k_tb_tb_upd<<<dim3((c->T + 63) / 64, J), 64,
                  (size_t)(kwmax * lmax + 2 * 64 * lmax) * sizeof(double), c->stream>>>(tbb);
    FASST_LAUNCH_CHECK();
    if (int st = launch_tb_h(c, tbb)) return st;
  }
  if (c->anytwc && b == 0)   // (a constrained source has one component: block 0)
    if (int st = launch_tw_constr(c, omega, true)) return st;
  // the step's W = FB FW is the current W of the next step (device to device: no DSpan)
  FASST_HIP(hipMemcpyAsync(c->Wkf.p, c->Wkf_new.p, (size_t)J * c->KP * c->Fp * sizeof(double),
                           hipMemcpyDeviceToDevice, c->stream));
  return FASST_OK;
}

static int multi_spectral(fasst_ctx *c, double omega) {
  int st;
  if (c->lambda > 0.0) {
    for (int q = 0; q < c->nseq; ++q)
      if ((st = multi_step(c, omega, c->seq_b[q], c->seq_j[q]))) return st;
    return FASST_OK;
  }
  for (int b = 0; b < c->maxblk; ++b)
    if ((st = multi_step(c, omega, b, -1))) return st;
  return FASST_OK;
}

// (FW.TW)^T and the TW row sums of the previous parameters, the operands of
// the spectral update; fork: on the side stream (joined by the caller
// through ev_join before their first consumer)
int launch_spectral_prep(fasst_ctx *c, bool fork) {
  const int J = c->J;
  hipStream_t side = fork ? c->aux : c->stream;
  if (fork) {
    FASST_HIP(hipEventRecord(c->ev_fork, c->stream));
    FASST_HIP(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
  }
  prof_begin(c, KFWH, side);
  bool any_fw = false;
  for (int j = 0; j < J; ++j) any_fw |= c->fw_free[j] != 0;
  // (KP > 64: 16-row FW chunk + TW tile, 80 KB of LDS, two blocks per CU;
  // ceiling set by spectral_lds_limits)
  (c->KP > 64 ? k_fwh_t<true> : k_fwh_t<false>)<<<dim3((c->Tp + 63) / 64, J), 256,
            c->KP > 64 ? (16 + 64) * c->KP * sizeof(double) : fw_lds(c, c->KP * 64),
            side>>>(c->FW.p, c->TW.p, c->FWHt.p, any_fw ? c->TWt.p : nullptr, J, c->Tp, c->KP,
                    c->halt);
  prof_end(c, KFWH, side);
  FASST_LAUNCH_CHECK();
  prof_begin(c, KROWS, side);
  k_tw_rowsum<<<J * c->KP, 256, 0, side>>>(c->TW.p, c->hsum.p, c->T, c->Tp, c->halt);
  prof_end(c, KROWS, side);
  FASST_LAUNCH_CHECK();
  if (fork) FASST_HIP(hipEventRecord(c->ev_join, c->aux));
  return FASST_OK;
}

// update_spectral_components (audioModel.py:1469-1978) from the rho planes in
// c->hatW (rho_j = hat_W_j / max(V_j, eps), V from the parameters before the
// update), after launch_spectral_prep and launch_w_old.  tail (fast_tail
// models inside gem_iteration): the fused renormalisation tail, its scales /
// rescale forked onto the side stream beside the TW contraction
int spectral_update(fasst_ctx *c, double omega, bool tail) {
  if (c->anytwc && c->lambda > 0.0) {
    set_error("a discrete-state TW (TW_constr GSMM / SHMM) with lambdaCorr > 0 is outside the "
              "HIP path");
    return FASST_ERR_UNSUPPORTED;
  }
  if (c->multi) return multi_spectral(c, omega);
  // spectral update: FB then TW (one NMF factor per source)
  const Step s = step_of(c);
  BArgs b = b_args(c, s);
  b.hatW = c->hatW.p;
  UArgs u = u_args(c, s, omega);
  u.pmax = tail ? c->rpmax2.p : nullptr;
  TArgs t = t_args(c, s, omega);
  t.hatW = c->hatW.p;
  TUArgs tu = tu_args(c, s, omega);
  tu.scal = tail ? c->rscal.p : nullptr;
  tu.tpart = c->rtpart2.p;
  tu.ntb = c->ntb;
  // the next iteration's FWHt / TW row sums formed here too (KP <= 64)
  // (not at KP = 128: its 64 KB TW tile leaves k_tw_update one block per CU,
  // 0.12 -> 0.38 ms at J = 4, more than the 0.23 ms it takes off the E-step)
  const bool prep = tail && c->ftail >= 2 && c->KP <= 64;
  tu.FWHt = prep ? c->FWHt.p : nullptr;
  tu.hpart = c->hpart.p;
  tu.twp = prep && estep_twi(c) ? c->twp.p : nullptr;   // (allocated by the iteration's E-step)
  launch_fb_contract(c, b, false, true);
  FASST_LAUNCH_CHECK();
  // (the mixing update beside the contraction, gem_iteration: its halt flag
  // is final before the first parameter moves)
  if (tail && c->mix_side) FASST_HIP(hipStreamWaitEvent(c->stream, c->ev_mix, 0));
  if (int st = launch_fb_update(c, u, tu, true)) return st;
  if (tail)
    if (int st = launch_tail_side(c)) return st;
  if (s.any_fw) {
    FWArgs w = fw_args(c, s, omega);
    w.hatW = c->hatW.p;
    if (int st = launch_fw_update(c, w, false, true)) return st;
  }
  launch_tw_contract_lds(c, t);
  FASST_LAUNCH_CHECK();
  // (prep reads the renormalised FW: wait for k_renorm_rows, else the scales)
  if (tail) FASST_HIP(hipStreamWaitEvent(c->stream, prep ? c->ev_rows : c->ev_scales, 0));
  if (int st = launch_tw_update(c, u, tu, true)) return st;
  if (c->anytwc) return launch_tw_constr(c, omega, false);
  return FASST_OK;
}

// k_rho_from_hatw into c->hatW from hat_W [J][F][T] on the device, with the
// current Wkf and TW (fasst_spectral_update, after launch_w_old)
int launch_rho_from_hatw(fasst_ctx *c, const double *hat_W_dev) {
  k_rho_from_hatw<<<dim3((c->F + 63) / 64, (c->T + 3) / 4, c->J), 256, 0, c->stream>>>(
      hat_W_dev, c->Wkf.p, c->TW.p, c->hatW.p, c->F, c->T, c->Fp, c->Tp, c->KP);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

}  // namespace fasst
