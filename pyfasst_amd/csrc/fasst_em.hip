// FASST generalized-EM iteration on MI355X (gfx950), FP64 throughout.
//
// One GEM iteration (audioModel.py:384-428) is a fixed sequence of launches
// on the context's stream:
//   k_w_from_fb   W = FB.FW                       (comp_spat_comp_power :485)
//   k_fwh_t       (FW.TW)^T                       (update_spectral_components :1541)
//   k_inst_A      per-bin mixing from 'inst' params (retrieve_subsrc_params :570-574)
//   k_estep<J>    fused E-step: V^T tiles on FP64 MFMA, Sigma_x, 2x2 inverse,
//                 loglik, posterior powers hat_W, per-bin sufficient
//                 statistics (compute_suff_stat :580-764)
//   k_loglik      loglik = -mean(...)             (:660-664)
//   k_mix_conv / k_mix_stats + k_mix_inst          (update_mix_matrix :766-889)
//   k_fb_contract FB numerator/denominator over t (MFMA, :1521-1575)
//   k_fb_update   FB *= (num/den)^omega, W_new = FB.FW
//   k_tw_contract TW numerator/denominator over f (MFMA) + TW update (:1634-1727)
//   k_renorm      renormalize_parameters          (:1980-2040)
// The E-step's kernels and launches are fasst_em_estep.hip's (interface:
// fasst_em.h); the other phases are still in this unit.
#include "fasst_em.h"
#include "fasst_device.h"
#include "fasst_twc.h"

#include <cmath>
#include <cstring>
#include <mutex>

namespace fasst {

static thread_local std::string g_err;
void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

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

// 'inst' mixing replicated over bins: A[r][c][f] = params[c][r], for the
// rows of rowm ('inst' sources; a mixed model's 'conv' rows hold their own
// per-bin filters)
__global__ void k_inst_A(const double2 *__restrict__ Pinst, double2 *__restrict__ A, int R,
                         int F, int Fp, unsigned rowm, const int *halt) {
  HALT_GUARD(halt);
  const int n = R * 2 * Fp;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
    const int f = idx % Fp;
    const int rc = idx / Fp;
    if (rowm >> (rc >> 1) & 1u) A[idx] = f < F ? Pinst[rc] : make_double2(0.0, 0.0);
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

// ---------------------------------------------------------------- mixing
struct MArgs {
  const double *part;  // [slot][Fp][NACC]
  const double *Wkf;   // [J][KP][Fp]   (W before the spectral update)
  const double *hsum;  // [J][KP]       sum_t TW
  double2 *A;          // [R][2][Fp]
  double2 *rss, *rxs;  // inst: [Fp][R][R], [Fp][2][R]
  int *flags;
  int F, Fp, J, R, nacc, conv_update, KP;
  ESched es;           // layout of part
  double invT;
  int jr[kMaxR];
  const int *halt;
};

__device__ __forceinline__ double2 cdiv(double2 a, double2 b) {
  // Smith's algorithm (as the C99 / numpy complex division)
  if (fabs(b.x) >= fabs(b.y)) {
    const double r = b.y / b.x, d = b.x + b.y * r;
    return make_double2((a.x + a.y * r) / d, (a.y - a.x * r) / d);
  }
  const double r = b.x / b.y, d = b.x * r + b.y;
  return make_double2((a.x * r + a.y) / d, (a.y * r - a.x) / d);
}

// One wave per bin f: sufficient statistics -> hat_Rss, hat_Rxs (:698-755),
// hermitised (:734-740); for 'conv' the per-bin solve hat_Rss^T X = hat_Rxs^T
// (:854-863) by LU with partial pivoting on |re|+|im| (LAPACK zgesv), the
// matrix entries spread over the lanes; for 'inst' the per-bin statistics are
// stored for k_mix_inst.
// QM: statistics per lane, ceil(NACC / 64) (2 at J = 4; the J > 8 models
// take the kMaxJ ceiling, the others stay at their own register count)
// RQ: hat_Rss entries per lane, ceil(R^2 / 64) (4 up to R = 16)
template <int QM, int RQ = 4>
__global__ __launch_bounds__(64) void k_mix(const MArgs a) {
  HALT_GUARD(a.halt);
  // LDS sized by this model's J, R, KP (mix_smem): with the kMaxJ / kMaxR /
  // kMaxKP ceilings a block took 19 KB, so only 8 blocks fit a CU and the
  // 2049 bins of C3 ran as two rounds of the whole latency chain
  extern __shared__ __attribute__((aligned(16))) double s_mix[];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int J = a.J, R = a.R, NACC = a.nacc;
  const int W = R + 2;
  double2 *s_A = (double2 *)s_mix;           // [R][2]
  double2 *s_L = s_A + 2 * R;                // [R][R + 2]: [M^T | hat_Rxs^T]
  double2 *s_H = s_L + R * W;                // [R][R]
  double2 *s_mult = s_H + R * R;             // [R]
  double *s_acc = (double *)(s_mult + R);    // [NACC]
  double *s_sv = s_acc + NACC;               // [J]
  double *s_wh0 = s_sv + J;                  // [J * KP] W_j(f, k)
  double *s_wh1 = s_wh0 + J * a.KP;          // [J * KP] sum_t TW_j(k, t)
  const int NP = J * (J + 1) / 2;
  {  // NACC = 72 > 64 lanes for J = 4: a lane sums up to 4 statistics, the
     // loads of all of them for 8 chunks in flight together (chunk order kept)
    constexpr int kQ = QM;
    double x[kQ] = {};
    const size_t cs = (size_t)a.Fp * NACC;
    const double *p0 = a.part + (size_t)f * NACC + lane;
    // the bin's segments, slot order (fasst_esched.h: from the formula)
    const int nseg = es_segments(a.es, f >> 4);
    for (int c = 0; c < nseg; c += 8) {
      double v[kQ][8];
#pragma unroll
      for (int q = 0; q < kQ; ++q)
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[q][u] = (lane + 64 * q < NACC && c + u < nseg) ? p0[(size_t)(c + u) * cs + 64 * q] : 0.0;
#pragma unroll
      for (int q = 0; q < kQ; ++q)
#pragma unroll
        for (int u = 0; u < 8; ++u) x[q] += v[q][u];
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q)
      if (lane + 64 * q < NACC) s_acc[lane + 64 * q] = x[q];
  }
  if (lane < 2 * R) s_A[(lane >> 1) * 2 + (lane & 1)] = a.A[(size_t)lane * a.Fp + f];
  // sum_t V_j(f, t) = sum_k W_j(f, k) sum_t TW_j(k, t): the operands are
  // loaded by all lanes at once (a per-source loop over k was a chain of
  // global-latency round trips), then summed in k order
  for (int i = lane; i < J * a.KP; i += 64) {
    s_wh0[i] = a.Wkf[(size_t)i * a.Fp + f];
    s_wh1[i] = a.hsum[i];
  }
  __syncthreads();
  if (lane < J) {
    double sv = 0.0;
    for (int k = 0; k < a.KP; ++k) sv += s_wh0[lane * a.KP + k] * s_wh1[lane * a.KP + k];
    s_sv[lane] = sv;
  }
  __syncthreads();
  // hat_Rss entries (r1, r2), R^2 <= 256: four per lane at most
  for (int e = lane; e < R * R; e += 64) {
    const int r1 = e / R, r2 = e % R;
    const int j1 = a.jr[r1], j2 = a.jr[r2];
    const int lo = min(j1, j2), hi = max(j1, j2);
    const int p = lo * J - lo * (lo - 1) / 2 + (hi - lo);
    const double n00 = s_acc[4 * p], n11 = s_acc[4 * p + 1];
    const double2 n01 = make_double2(s_acc[4 * p + 2], s_acc[4 * p + 3]);
    const double2 c10 = cconj(s_A[(r1) * 2 + (0)]), c11 = cconj(s_A[(r1) * 2 + (1)]);
    double2 v = cscale(cmul(c10, s_A[(r2) * 2 + (0)]), n00);               // a_r1^H Nsum a_r2
    v = cadd(v, cmul(cmul(c10, n01), s_A[(r2) * 2 + (1)]));
    v = cadd(v, cmul(cmul(c11, cconj(n01)), s_A[(r2) * 2 + (0)]));
    v = cadd(v, cscale(cmul(c11, s_A[(r2) * 2 + (1)]), n11));
    v = cscale(v, a.invT);
    if (r1 == r2) v.x += s_sv[j1] * a.invT;
    s_H[(r1) * R + (r2)] = v;
  }
  __syncthreads();
  double2 hv[RQ];  // hermitised entries of this lane (e = lane + 64 q)
#pragma unroll
  for (int q = 0; q < RQ; ++q) {
    const int e = lane + 64 * q;
    hv[q] = make_double2(0.0, 0.0);
    if (e < R * R) {
      const int r1 = e / R, r2 = e % R;
      const double2 x = s_H[(r1) * R + (r2)], y = s_H[(r2) * R + (r1)];
      hv[q] = cscale(cadd(x, cconj(y)), 0.5);
    }
  }
  if (lane < 2 * R) {  // hat_Rxs[f][c][r] = sum_c' Q_j[c][c'] A_r,c' / T
    const int r = lane >> 1, c = lane & 1;
    const double *qq = s_acc + 4 * NP + 8 * a.jr[r];
    const double2 q0 = make_double2(qq[4 * c + 0], qq[4 * c + 1]);
    const double2 q1 = make_double2(qq[4 * c + 2], qq[4 * c + 3]);
    s_L[(r) * W + (R + c)] = cscale(cadd(cmul(q0, s_A[(r) * 2 + (0)]), cmul(q1, s_A[(r) * 2 + (1)])), a.invT);
  }
  if (!a.conv_update) {
    __syncthreads();
    if (a.rss) {
#pragma unroll
      for (int q = 0; q < RQ; ++q) {
        const int e = lane + 64 * q;
        if (e < R * R) a.rss[((size_t)f * R + e / R) * R + e % R] = hv[q];
      }
      if (lane < 2 * R) {
        const int r = lane >> 1, c = lane & 1;
        a.rxs[((size_t)f * 2 + c) * R + r] = s_L[(r) * W + (R + c)];
      }
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < RQ; ++q) {  // L = hermitised(hat_Rss)^T
    const int e = lane + 64 * q;
    if (e < R * R) s_L[(e % R) * W + (e / R)] = hv[q];
  }
  __syncthreads();
  for (int k = 0; k < R; ++k) {
    // pivot: first row i >= k maximising |re|+|im| of L[i][k]
    double m = -1.0;
    int mi = R;
    if (lane >= k && lane < R) {
      m = fabs(s_L[(lane) * W + (k)].x) + fabs(s_L[(lane) * W + (k)].y);
      mi = lane;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double om = __shfl_xor(m, off, 64);
      const int oi = __shfl_xor(mi, off, 64);
      if (om > m || (om == m && oi < mi)) {
        m = om;
        mi = oi;
      }
    }
    if (m == 0.0) {
      if (lane == 0) {
        atomicOr(a.flags, 1);
        atomicOr(a.flags + kFlagHalt, 1);
      }
      return;
    }
    if (mi != k && lane < W) {
      const double2 t = s_L[(k) * W + (lane)];
      s_L[(k) * W + (lane)] = s_L[(mi) * W + (lane)];
      s_L[(mi) * W + (lane)] = t;
    }
    __syncthreads();
    if (lane > k && lane < R) s_mult[lane] = cmul(s_L[(lane) * W + (k)], cdiv(make_double2(1.0, 0.0), s_L[(k) * W + (k)]));
    __syncthreads();
    const int nr = R - k - 1, nc = W - k - 1;
    for (int e = lane; e < nr * nc; e += 64) {
      const int i = k + 1 + e / nc, c = k + 1 + e % nc;
      s_L[(i) * W + (c)] = csub(s_L[(i) * W + (c)], cmul(s_mult[i], s_L[(k) * W + (c)]));
    }
    __syncthreads();
  }
  for (int i = R - 1; i >= 0; --i) {
    if (lane < 2) {
      double2 x = s_L[(i) * W + (R + lane)];
      for (int q = i + 1; q < R; ++q) x = csub(x, cmul(s_L[(i) * W + (q)], s_L[(q) * W + (R + lane)]));
      s_L[(i) * W + (R + lane)] = cdiv(x, s_L[(i) * W + (i)]);
    }
    __syncthreads();
  }
  if (lane < 2 * R) a.A[(size_t)lane * a.Fp + f] = s_L[(lane >> 1) * W + (R + (lane & 1))];
}

static size_t mix_smem(int J, int R, int KP, int nacc) {
  return (size_t)(2 * R + R * (R + 2) + R * R + R) * sizeof(double2) +
         (size_t)(nacc + J + 2 * J * KP) * sizeof(double);
}

// 'inst' update (:808-839): f-means of the statistics, real R_u x R_u solve.
struct IArgs {
  const double2 *rss, *rxs, *A;
  double2 *Pinst;
  int *flags;
  int F, Fp, R, nu, no;
  int upd[kMaxR], oth[kMaxR];
  const int *halt;
};
__global__ void k_mix_inst(const IArgs a) {
  HALT_GUARD(a.halt);
  __shared__ double s_b[kMaxR][2];
  __shared__ double s_m[kMaxR][kMaxR];
  const int nu = a.nu, R = a.R;
  const int tid = threadIdx.x;
  const int nb = 2 * nu, nm = nu * nu;
  // (2 nu + nu^2 reaches 288 at nu = 16: more entries than threads)
  for (int idx = tid; idx < nb + nm; idx += blockDim.x) {
    double s = 0.0;
    if (idx < nb) {
      const int c = idx / nu, u = idx % nu, ru = a.upd[u];
      for (int f = 0; f < a.F; ++f) {
        double2 x = a.rxs[((size_t)f * 2 + c) * R + ru];
        for (int o = 0; o < a.no; ++o) {
          const int ro = a.oth[o];
          x = csub(x, cmul(a.A[(size_t)(2 * ro + c) * a.Fp + f], a.rss[((size_t)f * R + ro) * R + ru]));
        }
        s += x.x;
      }
      s_b[u][c] = s / a.F;
    } else {
      const int e = idx - nb, u1 = e / nu, u2 = e % nu;
      for (int f = 0; f < a.F; ++f) s += a.rss[((size_t)f * R + a.upd[u1]) * R + a.upd[u2]].x;
      s_m[u1][u2] = s / a.F;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  // (the serial solve on LDS copies: up to 32 x 32 would not fit registers)
  __shared__ double Lm[kMaxR][kMaxR], B[kMaxR][2];
  for (int i = 0; i < nu; ++i) {
    for (int k = 0; k < nu; ++k) Lm[i][k] = s_m[k][i];  // rm^T
    B[i][0] = s_b[i][0];
    B[i][1] = s_b[i][1];
  }
  for (int k = 0; k < nu; ++k) {
    int piv = k;
    double best = fabs(Lm[k][k]);
    for (int i = k + 1; i < nu; ++i)
      if (fabs(Lm[i][k]) > best) {
        best = fabs(Lm[i][k]);
        piv = i;
      }
    if (best == 0.0) {
      atomicOr(a.flags, 1);
      atomicOr(a.flags + kFlagHalt, 1);
      return;
    }
    if (piv != k) {
      for (int c = 0; c < nu; ++c) {
        const double t = Lm[k][c];
        Lm[k][c] = Lm[piv][c];
        Lm[piv][c] = t;
      }
      for (int c = 0; c < 2; ++c) {
        const double t = B[k][c];
        B[k][c] = B[piv][c];
        B[piv][c] = t;
      }
    }
    const double rinv = 1.0 / Lm[k][k];
    for (int i = k + 1; i < nu; ++i) {
      const double l = Lm[i][k] * rinv;
      for (int c = k + 1; c < nu; ++c) Lm[i][c] -= l * Lm[k][c];
      for (int c = 0; c < 2; ++c) B[i][c] -= l * B[k][c];
    }
  }
  for (int i = nu - 1; i >= 0; --i)
    for (int c = 0; c < 2; ++c) {
      double x = B[i][c];
      for (int q = i + 1; q < nu; ++q) x -= Lm[i][q] * B[q][c];
      B[i][c] = x / Lm[i][i];
    }
  for (int u = 0; u < nu; ++u)
    for (int c = 0; c < 2; ++c) a.Pinst[a.upd[u] * 2 + c] = make_double2(B[u][c], 0.0);
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

// ---------------------------------------------------------------- renormalize
struct RArgs {
  double2 *A, *Pinst;
  double *FB, *FW, *TW;
  double *scal;   // [J][2 + 2*KP]: e_j, -, w_j[KP], w2_j[KP] (stage 2 -> 3)
  double *pmax;   // [J][nchunk][KP] column maxima of FB per bin chunk
  double *pe;     // [J][nchunk] partial mixing-filter energy (conv)
  double *tpart;  // [nslot][nchunk] partial sums of the rescaled TW, per block
  int *flags;
  // fused tail (k_renorm_scales / _rows / _tail): k_fb_update's column
  // maxima [J][nstat][KP], k_tw_update's restart sums [nslot][ntb], the
  // E-step's loglik partials
  const double *pmax2, *tpart2, *llpart;
  double *ll_out;
  // k_tw_update's TW row-sum partials [J][KP][ntb] -> hsum [J][KP] (null: the
  // next iteration's k_tw_rowsum forms hsum)
  const double *hpart;
  double *hsum;
  int J;
  double inv_FT;
  int nstat, ntb;
  ESched es;   // layout of llpart
  int F, T, Fp, Tp, KP, nchunk, tpc, fpc, nslot;
  unsigned convm;    // bit j: spatial component j is 'conv' (per-bin filters in A)
  int K[kMaxJ], roff[kMaxJ + 1];
  // spectral components of source j (column blocks of FB / FW / TW) and the
  // slot of block 0
  int nblk[kMaxJ], kb[kMaxJ][kMaxBlk + 1], soff[kMaxJ + 1];
  unsigned tbmask;   // slots with time blobs: their restart test is k_tb_renorm's
  const int *halt;
};

// renormalize_parameters (audioModel.py:1991-2037) in two passes over
// (source, chunk) blocks.  Stage 1: per bin chunk, the column maxima of FB
// and (conv) the partial energy of the mixing filters.  Since x -> fl(x e) is
// monotone for e >= 0, max_f fl(FB e) = fl(e max_f FB): the maxima are taken
// on the raw FB and scaled in stage 2.
__global__ __launch_bounds__(256) void k_renorm_stats(const RArgs a) {
  HALT_GUARD(a.halt);
  __shared__ double s_red[256];
  const int j = blockIdx.y, c = blockIdx.x, KP = a.KP;
  const int fb = c * a.fpc, fe = min(fb + a.fpc, a.F);
  const int groups = blockDim.x / KP, k = threadIdx.x % KP, g = threadIdx.x / KP;
  double m = -INFINITY;
  if (g < groups)
    for (int f = fb + g; f < fe; f += groups) m = fmax(m, a.FB[((size_t)j * a.Fp + f) * KP + k]);
  s_red[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x < KP) {
    double x = s_red[threadIdx.x];
    for (int q = 1; q < groups; ++q) x = fmax(x, s_red[q * KP + threadIdx.x]);
    a.pmax[((size_t)j * a.nchunk + c) * KP + threadIdx.x] = x;
  }
  __syncthreads();
  if (a.convm >> j & 1u) {
    const int r0 = a.roff[j], nr = a.roff[j + 1] - r0, w = fe - fb;
    double e = 0.0;
    for (int idx = threadIdx.x; idx < nr * 2 * w; idx += blockDim.x) {
      const int f = fb + idx % w, rc = idx / w;
      const double2 x = a.A[(size_t)(2 * r0 + rc) * a.Fp + f];
      e += x.x * x.x + x.y * x.y;
    }
    e = block_sum(e, s_red);
    if (threadIdx.x == 0) a.pe[(size_t)j * a.nchunk + c] = e;
  }
}

// Stage 2: every block recombines the (tiny) stage-1 partials into e_j,
// w_j[k] = max_f FB[:,k] e_j (0 -> 1) and w2_j[c] = mean_r FW[r,c] w_j[r]
// (0 -> 1), then scales its chunk: FB rows (FB e / w), TW columns (TW w2,
// with partial sums for the restart test), the mixing filters / sqrt(e).
// FW and the 'inst' parameters are read by every block here, so they are
// rewritten in stage 3 from the scales chunk 0 records.
template <bool BIG>
__global__ __launch_bounds__(256) void k_renorm_apply(const RArgs a) {
  HALT_GUARD(a.halt);
  __shared__ double s_red[256];
  __shared__ double s_w[kMaxKP], s_w2[kMaxKP];
  __shared__ double s_e;
  __shared__ double s_big[64 * 64];   // chunk maxima, then FW_j (KP <= 64; else from L2)
  const int j = blockIdx.y, c = blockIdx.x;
  const int K = a.K[j], KP = a.KP;
  const int r0 = a.roff[j], nr = a.roff[j + 1] - r0;
  // the cross-chunk statistics are loaded by all threads at once and folded
  // in LDS (a per-thread loop over the chunks was a chain of dependent
  // global-latency round trips), in the same order as before
  const bool cj = a.convm >> j & 1u;
  const int ne = cj ? a.nchunk : nr * 2;
  for (int q = threadIdx.x; q < ne; q += blockDim.x) {
    if (cj) {
      s_red[q] = a.pe[(size_t)j * a.nchunk + q];
    } else {
      const double2 x = a.Pinst[2 * r0 + q];
      s_red[q] = x.x * x.x + x.y * x.y;
    }
  }
  constexpr bool big = BIG;   // chunk maxima / FW too large for s_big: read from L2
  const double *pmx = big ? a.pmax + (size_t)j * a.nchunk * KP : s_big;
  const double *fwb = big ? a.FW + (size_t)j * KP * KP : s_big;
  if (!big)
    for (int i = threadIdx.x; i < a.nchunk * KP; i += blockDim.x)
      s_big[i] = a.pmax[(size_t)j * a.nchunk * KP + i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double e = 0.0;
    for (int q = 0; q < ne; ++q) e += s_red[q];
    s_e = e / (double)(cj ? nr * 2 * a.F : nr * 2);
  }
  __syncthreads();
  const double e = s_e;
  if (threadIdx.x < KP) {
    double m = -INFINITY;
    for (int q = 0; q < a.nchunk; ++q) m = fmax(m, pmx[q * KP + threadIdx.x]);
    const double w = m * e;
    s_w[threadIdx.x] = w == 0.0 ? 1.0 : w;
  }
  __syncthreads();
  if (!big)
    for (int i = threadIdx.x; i < KP * KP; i += blockDim.x) s_big[i] = a.FW[(size_t)j * KP * KP + i];
  __syncthreads();
  if (threadIdx.x < K) {
    // FW.mean(axis=0) of the column's own spectral component (block)
    const int cc = threadIdx.x;
    int b = 0;
    while (b + 1 < a.nblk[j] && cc >= a.kb[j][b + 1]) ++b;
    const int r0b = a.kb[j][b], r1b = a.kb[j][b + 1];
    double s = 0.0;
    for (int r = r0b; r < r1b; ++r) s += fwb[r * KP + cc] * s_w[r];
    s /= (double)(r1b - r0b);
    s_w2[cc] = s == 0.0 ? 1.0 : s;
  }
  __syncthreads();
  // FB rows of this chunk (only the K live columns carry data)
  // (element loops below load a batch of kRnB values before storing any, so
  // a thread keeps kRnB memory round trips in flight)
  constexpr int kRnB = 8;
  const int fb = c * a.fpc, fe = min(fb + a.fpc, a.F);
  {
    const int n = (fe - fb) * KP;
    for (int base = threadIdx.x; base < n; base += kRnB * blockDim.x) {
      double x[kRnB];
#pragma unroll
      for (int u = 0; u < kRnB; ++u) {
        const int idx = base + u * blockDim.x;
        x[u] = idx < n ? a.FB[((size_t)j * a.Fp + fb + idx / KP) * KP + idx % KP] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kRnB; ++u) {
        const int idx = base + u * blockDim.x, k = idx % KP;
        if (idx < n && k < K)
          a.FB[((size_t)j * a.Fp + fb + idx / KP) * KP + k] = (x[u] * e) / s_w[k];
      }
    }
  }
  const double se = sqrt(e);
  if (cj) {
    const int w = fe - fb;
    for (int idx = threadIdx.x; idx < nr * 2 * w; idx += blockDim.x) {
      const int f = fb + idx % w, rc = idx / w;
      double2 *p = a.A + (size_t)(2 * r0 + rc) * a.Fp + f;
      *p = make_double2(p->x / se, p->y / se);
    }
  }
  if (c == 0) {  // FW and 'inst' parameters are rewritten in stage 3 (read above)
    double *sc = a.scal + (size_t)j * (2 + 2 * KP);
    if (threadIdx.x == 0) sc[0] = e;
    if (threadIdx.x < KP) {
      sc[2 + threadIdx.x] = s_w[threadIdx.x];
      sc[2 + KP + threadIdx.x] = s_w2[threadIdx.x];
    }
  }
  double *TW = a.TW + (size_t)j * KP * a.Tp;
  const int t0 = c * a.tpc, t1 = min(t0 + a.tpc, a.T);
  const int w = t1 - t0;
  for (int b = 0; b < a.nblk[j]; ++b) {   // one restart sum per spectral component
    const int rb = a.kb[j][b], nrow = a.kb[j][b + 1] - rb;
    double tsum = 0.0;
    if (w > 0)
      for (int base = threadIdx.x; base < nrow * w; base += kRnB * blockDim.x) {
        double x[kRnB];
#pragma unroll
        for (int u = 0; u < kRnB; ++u) {
          const int idx = base + u * blockDim.x;
          x[u] = idx < nrow * w ? TW[(size_t)(rb + idx / w) * a.Tp + t0 + idx % w] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kRnB; ++u) {
          const int idx = base + u * blockDim.x;
          if (idx < nrow * w) {
            const double y = x[u] * s_w2[rb + idx / w];
            TW[(size_t)(rb + idx / w) * a.Tp + t0 + idx % w] = y;
            tsum += y;
          }
        }
      }
    tsum = block_sum(tsum, s_red);
    if (threadIdx.x == 0) a.tpart[(size_t)(a.soff[j] + b) * a.nchunk + c] = tsum;
  }
}

// Stage 3 (one block): FW = FW w / w2, 'inst' parameters / sqrt(e), and the
// restart test sum(TW_j) < eps -> host-side random restart (audioModel.py:2023)
__global__ void k_renorm_final(const RArgs a, int J, int iter) {
  HALT_GUARD(a.halt);
  for (int j = 0; j < J; ++j) {
    const int K = a.K[j], KP = a.KP;
    const double *sc = a.scal + (size_t)j * (2 + 2 * KP);
    double *FW = a.FW + (size_t)j * KP * KP;
    for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
      const int r = idx / K, cc = idx % K;
      FW[r * KP + cc] = (FW[r * KP + cc] * sc[2 + r]) / sc[2 + KP + cc];
    }
    const int r0 = a.roff[j], nr = a.roff[j + 1] - r0;
    if (!(a.convm >> j & 1u) && threadIdx.x < nr * 2) {
      const double se = sqrt(sc[0]);
      double2 *p = a.Pinst + 2 * r0 + threadIdx.x;
      *p = make_double2(p->x / se, p->y / se);
    }
  }
  __shared__ double s_t[kMaxSlot * 64];   // the per-chunk TW sums, loaded at once
  for (int i = threadIdx.x; i < a.nslot * a.nchunk; i += blockDim.x) s_t[i] = a.tpart[i];
  __syncthreads();
  const int sl = threadIdx.x;   // one TW restart test per spectral component
  if (sl >= a.nslot || (a.tbmask >> sl & 1u)) return;
  double s = 0.0;
  for (int c = 0; c < a.nchunk; ++c) s += s_t[sl * a.nchunk + c];
  const int dead = s < kEps ? 1 : 0;
  a.flags[1 + sl] = dead;
  if (dead) {
    a.flags[kFlagHalt] = 1;
    a.flags[kFlagIter] = iter;
  }
}

// Fused tail of gem_iteration (one spectral component per source, no time
// blobs, fixed FW): the same renormalize_parameters (audioModel.py:1991-2037)
// with the FB column maxima taken by k_fb_update, the scales formed once per
// source (k_renorm_scales) after the mixing update, and the FB / mixing / FW
// rescale (k_renorm_rows) on the side stream while the TW contraction runs;
// TW's rescale and restart sums ride in k_tw_update, and k_renorm_tail closes
// the iteration with the restart test and the loglik sum.
//
// k_renorm_scales, one block per source: e_j = mean |params|^2 (the 'conv'
// filters read from A itself, 'inst' from Pinst), w_j[k] = e_j max_f FB[f][k]
// (0 -> 1), w2_j[c] = mean_r FW[r][c] w_j[r] over the K live rows (0 -> 1).
// Every thread issues its loads in batches before using any: the round-5
// form walked the 129 maxima, the energy partials and the K x K FW as chains
// of dependent loads (105 us beside the TW contraction, profiles/r5_bench.txt)
__global__ __launch_bounds__(1024) void k_renorm_scales(const RArgs a) {
  HALT_GUARD(a.halt);
  constexpr int NT = 1024, B = 16;   // threads; loads in flight per thread and batch
  __shared__ double s_red[NT];
  __shared__ double s_w[kMaxKP];
  const int t = threadIdx.x, j = blockIdx.x, K = a.K[j], KP = a.KP, ns = a.nstat;
  const int r0 = a.roff[j], nr = a.roff[j + 1] - r0;
  const bool cj = a.convm >> j & 1u;
  // e_j: the 'conv' filters A[r][c][f] of the source's nr ranks (one batch
  // of loads per thread up to 8 ranks at C3's F)
  const int ne = cj ? nr * 2 * a.F : nr * 2;
  double e = 0.0;
  for (int base = t; base < ne; base += B * NT) {
    double2 x[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int idx = base + u * NT;
      x[u] = idx >= ne ? make_double2(0.0, 0.0)
                       : (cj ? a.A[(size_t)(2 * r0 + idx / a.F) * a.Fp + idx % a.F] : a.Pinst[2 * r0 + idx]);
    }
#pragma unroll
    for (int u = 0; u < B; ++u) e += x[u].x * x[u].x + x[u].y * x[u].y;
  }
  // column maxima over k_fb_update's blocks: thread (g, k) takes blocks
  // q = g mod G (max is exact in any order; 5 per thread at C3)
  const int G = NT / KP;
  double m = -INFINITY;
  for (int q0 = t / KP; q0 < ns; q0 += B * G) {
    double x[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int q = q0 + u * G;
      x[u] = q < ns ? a.pmax2[((size_t)j * ns + q) * KP + t % KP] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < B; ++u) m = fmax(m, x[u]);
  }
  // FW[r][c] of thread (g, c): rows r = g, g + G, ... (all of them in one
  // batch up to K = 64 at KP = 64, K = 32 at KP = 32: one row per thread)
  const int cc = t % KP;
  const double *fw = a.FW + (size_t)j * KP * KP;
  constexpr int RB = 8;
  double fr[RB];
#pragma unroll
  for (int u = 0; u < RB; ++u) {
    const int r = t / KP + u * G;
    fr[u] = r < K && cc < K ? fw[r * KP + cc] : 0.0;
  }
  e = block_sum(e, s_red) / (double)ne;
  s_red[t] = m;
  __syncthreads();
  for (int k = t; k < KP; k += NT) {
    double x = -INFINITY;
    for (int g = 0; g < G; ++g) x = fmax(x, s_red[g * KP + k]);
    const double w = x * e;
    s_w[k] = w == 0.0 ? 1.0 : w;
  }
  __syncthreads();
  // FW.mean(axis=0) of the column's spectral component: the thread's rows,
  // then the groups in order (one row per group: the sequential row order)
  double sp = 0.0;
#pragma unroll
  for (int u = 0; u < RB; ++u) {
    const int r = t / KP + u * G;
    if (r < K) sp += fr[u] * s_w[r];
  }
  for (int r = t / KP + RB * G; r < K; r += G) sp += fw[r * KP + cc] * s_w[r];   // (K > RB G only)
  s_red[t] = sp;
  __syncthreads();
  double *sc = a.scal + (size_t)j * (2 + 2 * KP);
  if (t < KP) {
    double s = 1.0;
    if (t < K) {
      s = 0.0;
      for (int g = 0; g < G; ++g) s += s_red[g * KP + t];
      s /= (double)K;
      if (s == 0.0) s = 1.0;
    }
    sc[2 + t] = s_w[t];
    sc[2 + KP + t] = s;
  }
  if (t == 0) sc[0] = e;
}

// FB rows of 16 bins (FB e / w), the 'conv' filters / sqrt(e); block x = 0
// also rescales FW (FW w / w2) and the 'inst' parameters of its source
__global__ __launch_bounds__(256) void k_renorm_rows(const RArgs a) {
  HALT_GUARD(a.halt);
  const int j = blockIdx.y, f0 = blockIdx.x * 16, K = a.K[j], KP = a.KP;
  const int nb = min(16, a.F - f0);
  const double *sc = a.scal + (size_t)j * (2 + 2 * KP);
  const double e = sc[0], se = sqrt(e);
  for (int idx = threadIdx.x; idx < nb * KP; idx += blockDim.x) {
    const int k = idx % KP;
    double *p = a.FB + ((size_t)j * a.Fp + f0 + idx / KP) * KP + k;
    if (k < K) *p = (*p * e) / sc[2 + k];
  }
  const int r0 = a.roff[j], nr = a.roff[j + 1] - r0;
  if (a.convm >> j & 1u) {
    for (int idx = threadIdx.x; idx < nr * 2 * nb; idx += blockDim.x) {
      double2 *p = a.A + (size_t)(2 * r0 + idx / nb) * a.Fp + f0 + idx % nb;
      *p = make_double2(p->x / se, p->y / se);
    }
  } else if (blockIdx.x == 0 && threadIdx.x < nr * 2) {
    double2 *p = a.Pinst + 2 * r0 + threadIdx.x;
    *p = make_double2(p->x / se, p->y / se);
  }
  if (blockIdx.x == 0) {
    double *FW = a.FW + (size_t)j * KP * KP;
    for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
      const int r = idx / K, cc = idx % K;
      FW[r * KP + cc] = (FW[r * KP + cc] * sc[2 + r]) / sc[2 + KP + cc];
    }
  }
}

// one block: the iteration's loglik (k_loglik's sum) and the TW restart test
// from k_tw_update's partial sums (audioModel.py:2023)
__global__ __launch_bounds__(256) void k_renorm_tail(const RArgs a, int iter) {
  HALT_GUARD(a.halt);
  if (blockIdx.x > 0) {
    // blocks 1..: hsum[r] = sum_t TW row r from k_tw_update's per-block
    // partials, one wave per row (lane-strided, then the wave's tree: a
    // fixed order)
    const int r = (blockIdx.x - 1) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.J * a.KP) return;
    double h = 0.0;
    for (int b = lane; b < a.ntb; b += 64) h += a.hpart[(size_t)r * a.ntb + b];
#pragma unroll
    for (int mm = 32; mm > 0; mm >>= 1) h += __shfl_xor(h, mm, 64);
    if (lane == 0) a.hsum[r] = h;
    return;
  }
  __shared__ double s[256];
  const double x = ll_partial_sum(a.llpart, a.es);
  s[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.ll_out[0] = -(s[0] * a.inv_FT);
  __syncthreads();
  for (int sl = 0; sl < a.nslot; ++sl) {
    double t = 0.0;
    for (int c = threadIdx.x; c < a.ntb; c += 256) t += a.tpart2[(size_t)sl * a.ntb + c];
    t = block_sum(t, s);
    if (threadIdx.x == 0) {
      const int dead = t < kEps ? 1 : 0;
      a.flags[1 + sl] = dead;
      if (dead) {
        a.flags[kFlagHalt] = 1;
        a.flags[kFlagIter] = iter;
      }
    }
  }
}

// ---------------------------------------------------------------- time blobs
// A spectral component with time blobs (TB, audioModel.py:430-498) has
// H = TW TB.  Its factor TW ("TWs", block rows x L) and TB (L x T) live in the
// slot buffer tb[j][b] (tb_layout) and the block's rows of the model TW hold
// H, so every other kernel (E-step, FB / FW / TW contractions, Wiener) reads
// H unchanged.  Both updates reuse the block's TW contraction, which leaves
// G = W^T R over f per frame in tnum / tden (W = FB FW of the block):
//   TW step (:1665-1691): num = G TB^T, den likewise        (k_tb_tw_red)
//   TB step (:1931-1978): num = TWs^T G, with R's ratio hat_W / max(V^2, eps)
//                         (k_tw_contract<TBQ>, then k_tb_tb_upd)
// the reference's (W TWs)^T R reassociated; H is rebuilt after each (k_tb_h).
struct TBLayout {
  size_t tws, tb, num, den, n;   // offsets (doubles) in the slot buffer, total
};
__host__ __device__ inline TBLayout tb_layout(int kbw, int L, int Tp) {
  TBLayout o;
  o.tws = 0;
  o.tb = (size_t)kbw * L;
  o.num = o.tb + (size_t)L * Tp;
  o.den = o.num + (size_t)kbw * L;
  o.n = o.den + (size_t)kbw * L;
  return o;
}

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

__device__ inline bool tb_halted(const int *halt, const int *flags, int iter) {
  if (!halt || !*(volatile const int *)halt) return false;
  return iter < 0 || *(volatile const int *)(flags + kFlagIter) < iter;
}

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

// renormalize_parameters for a component with time blobs (:2019-2033), after
// k_renorm_final: TWs *= w (the FW column means, as the block's H rows got in
// k_renorm_apply), the restart test on sum(TWs), then TB /= m, TWs *= m with
// m = TB.mean(axis=1).  A dead component is left to the host (redraw, then
// the TB step of the renormalisation), one block per (component, source).
struct TBRArgs {
  double *tb[kMaxJ][kMaxBlk];
  int L[kMaxJ][kMaxBlk], kb0[kMaxJ][kMaxBlk], kbw[kMaxJ][kMaxBlk], slot[kMaxJ][kMaxBlk];
  const double *scal;   // RArgs::scal: w2 = FW column means at [j][2 + KP + k]
  int *flags;
  const int *halt;
  int T, Tp, KP, iter;
};
__global__ __launch_bounds__(256) void k_tb_renorm(const TBRArgs a) {
  if (tb_halted(a.halt, a.flags, a.iter)) return;
  __shared__ double s_red[256];
  __shared__ double s_m[kMaxTB];
  const int b = blockIdx.x, j = blockIdx.y;
  double *p = a.tb[j][b];
  if (!p) return;
  const int L = a.L[j][b], kbw = a.kbw[j][b], n = kbw * L;
  const TBLayout o = tb_layout(kbw, L, a.Tp);
  const double *w2 = a.scal + (size_t)j * (2 + 2 * a.KP) + 2 + a.KP + a.kb0[j][b];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double y = p[o.tws + i] * w2[i / L];
    p[o.tws + i] = y;
    s += y;
  }
  s = block_sum(s, s_red);
  const int dead = s < kEps ? 1 : 0;
  if (threadIdx.x == 0) {
    a.flags[1 + a.slot[j][b]] = dead;
    if (dead) {
      a.flags[kFlagHalt] = 1;
      a.flags[kFlagIter] = a.iter;
    }
  }
  if (dead) return;
  double *TB = p + o.tb;
  for (int l = 0; l < L; ++l) {
    double m = 0.0;
    for (int t = threadIdx.x; t < a.T; t += blockDim.x) m += TB[(size_t)l * a.Tp + t];
    m = block_sum(m, s_red) / (double)a.T;
    if (m == 0.0) m = 1.0;
    for (int t = threadIdx.x; t < a.T; t += blockDim.x) TB[(size_t)l * a.Tp + t] /= m;
    if (threadIdx.x == 0) s_m[l] = m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[o.tws + i] *= s_m[i % L];
}

// ---------------------------------------------------------------- host side
static const char *kKernelNames[fasst_ctx::kNK] = {
    "k_w_from_fb", "k_fwh_t", "k_inst_A", "k_estep", "k_loglik", "k_mix",
    "k_mix_inst", "k_fb_contract", "k_fb_update", "k_tw_contract", "k_renorm", "k_tw_update",
    "k_fw_update", "k_tw_rowsum", "k_renorm_tail", "k_tw_statediv", "k_tw_decode",
    "k_sf_gemm", "k_sf_prod", "k_sf_ratio", "k_sf_update", "k_sf_renorm", "k_sf_wiener",
    "k_sf_other", "k_sf_hatw", "k_sf_energy", "k_sf_bary", "k_sf_sparsify",
    "k_sfw_scale", "k_sfw_dgemm2", "k_sfw_update", "k_sfw_renorm"};

// after a device sync: fold the recorded event pairs into the averages
static void prof_collect(fasst_ctx *c) {
  if (!c->prof) return;
  for (int i = 0; i < fasst_ctx::kNK; ++i)
    for (int q = 0; q < fasst_ctx::kProfRing; ++q) {
      if (!c->used[i][q]) continue;
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->ev0[i][q], c->ev1[i][q]) == hipSuccess) {
        c->prof_ms[i] += ms;
        c->prof_cnt[i] += 1;
      }
      c->used[i][q] = 0;
    }
}

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
static int twl_occupancy(const fasst_ctx *c, bool bal, int *units, int *group_tiles) {
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
static int contract_occupancy(const fasst_ctx *c) {
  int n = 1;
  hipError_t e = hipSuccess;
  nkc_dispatch(c, [&](auto k) {
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_fb_contract<decltype(k)::value, kFPW>,
                                                     64, 0);
  });
  return e == hipSuccess ? std::max(1, n) : 1;
}

// bins per block of the FW update's f-contraction (k_fw_reduce holds three
// [fpc][KP] tiles in LDS: 96 KB at KP = 128 with 32 bins)
static int fw_fpc(const fasst_ctx *c) { return c->KP > 64 ? 32 : kFwFpc; }
// dynamic LDS of the kernels that stage FW ([KP][KP] when KP <= 64) next to
// `rest` doubles
static size_t fw_lds(const fasst_ctx *c, int rest) {
  return (size_t)((c->KP > 64 ? 0 : c->KP * c->KP) + rest) * sizeof(double);
}

// Split count c in [1, max_split] for a launch of unit * c equal blocks on
// `cap` resident slots: maximises the filled fraction of the last round
// (unit c / (cap ceil(unit c / cap))), preferring fewer splits within 1.5%.
static int best_split(long unit, long cap, int max_split) {
  max_split = std::max(1, max_split);
  auto eff = [&](int k) {
    const long blocks = unit * k;
    const long rounds = (blocks + cap - 1) / cap;
    return (double)blocks / (double)(rounds * cap);
  };
  double best = 0.0;
  for (int k = 1; k <= max_split; ++k) best = std::max(best, eff(k));
  for (int k = 1; k <= max_split; ++k)
    if (eff(k) >= best - 0.015) return k;
  return 1;
}

// Dynamic-LDS ceilings of the kernels whose launches may pass the 64 KB
// default, raised once per model configuration to the most any structure asks
// of them (not per iteration: the sizes depend only on the model shape, and
// a ceiling above a launch's own size costs nothing)
static int spectral_lds_limits() {
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

static int mix_lds_limits() {
  constexpr int nacc = 4 * (kMaxJ * (kMaxJ + 1) / 2) + 8 * kMaxJ;
  const size_t bytes = mix_smem(kMaxJ, kMaxR, kMaxKP, nacc);
  if (hipFuncSetAttribute((const void *)k_mix<(nacc + 63) / 64, (kMaxR * kMaxR + 63) / 64>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", bytes);
    return FASST_ERR_DEVICE;
  }
  return FASST_OK;
}

int configure_model(fasst_ctx *c, int J, const int *rank, const int *K, const int *convj) {
  if (J < 1 || J > kMaxJ) {
    set_error("J=%d outside the HIP path (1..%d sources)", J, kMaxJ);
    return FASST_ERR_UNSUPPORTED;
  }
  sf_release(c);   // a single-factor model replaces a two-factor one
  int R = 0, kmax = 0;
  for (int j = 0; j < J; ++j) {
    if (rank[j] < 1 || K[j] < 1) {
      set_error("bad rank/K for source %d", j);
      return FASST_ERR_SHAPE;
    }
    R += rank[j];
    kmax = std::max(kmax, K[j]);
  }
  if (R > kMaxR || kmax > kMaxKP) {
    set_error("total rank %d (max %d) / K %d (max %d) outside the HIP path", R, kMaxR, kmax,
              kMaxKP);
    return FASST_ERR_UNSUPPORTED;
  }
  if (int st = spectral_lds_limits()) return st;
  if (int st = estep_lds_limits()) return st;
  if (int st = mix_lds_limits()) return st;
  c->J = J;
  c->R = R;
  c->convm = 0;
  for (int j = 0; j < J; ++j)
    if (convj[j]) c->convm |= 1u << j;
  // conv: every source 'conv' (per-bin mixing update); otherwise the 'inst'
  // update runs over the free 'inst' sources with the rest held fixed
  const int conv = c->convm == (1u << J) - 1u ? 1 : 0;
  c->conv = conv;
  // the E-step addresses TW through a raw buffer resource with 32-bit byte
  // offsets (j KP + 4 s) Tp 8 (k_estep_mx's SA form)
  {
    const int KPc = kmax <= 16 ? 16 : (kmax <= 32 ? 32 : (kmax <= 64 ? 64 : 128));
    if ((size_t)J * KPc * c->Tp * sizeof(double) >= (1ull << 31)) {
      set_error("J %d x K %d x T %d: the TW plane passes the E-step's 2 GB buffer offsets", J,
                KPc, c->T);
      return FASST_ERR_UNSUPPORTED;
    }
  }
  c->KP = kmax <= 16 ? 16 : (kmax <= 32 ? 32 : (kmax <= 64 ? 64 : 128));
  c->roff[0] = 0;
  for (int j = 0; j < J; ++j) {
    c->rank[j] = rank[j];
    c->K[j] = K[j];
    c->roff[j + 1] = c->roff[j] + rank[j];
    c->spat_free[j] = c->fb_free[j] = c->tw_free[j] = 1;
    c->fw_free[j] = 0;
    c->nblk[j] = 1;   // one spectral component per source until fasst_set_blocks
    c->kb[j][0] = 0;
    c->kb[j][1] = K[j];
    c->bfb[j][0] = c->btw[j][0] = 1;
    c->bfw[j][0] = 0;
    c->soff[j] = j;
  }
  c->soff[J] = c->nslot = J;
  c->maxblk = 1;
  c->multi = 0;
  for (int j = 0; j < kMaxJ; ++j)
    for (int b = 0; b < kMaxBlk; ++b) {
      c->tb[j][b].release();
      c->tbl[j][b] = c->btb[j][b] = 0;
    }
  c->anytb = 0;
  for (int j = 0; j < kMaxJ; ++j) c->twc[j] = c->twc_free[j] = 0;
  c->anytwc = 0;
  c->nsrc = 0;
  c->lambda = 0.0;
  c->nseq = 0;
  const int Fp = c->Fp, Tp = c->Tp, KP = c->KP;
  // Launch shapes sized to whole rounds of resident blocks (a partial last
  // round idles most of the chip): E-step blocks = f tiles x frame chunks,
  // FB waves = bin-tile pairs x sources x frame chunks, TW waves = frame-tile
  // pairs x sources x bin chunks.
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess ||
      ncu <= 0)
    ncu = 256;
  const long cap_e = (long)estep_occupancy(c) * ncu;
  // (measured at C3: chunks of >= ~40 frame tiles keep the E-step's per-block
  // prologue/epilogue small; the contractions tolerate finer splits)
  c->nchunk_e = best_split(c->nft, cap_e, c->ntt / 40);
  if (const char *v = getenv("FASST_NCHUNK_E")) c->nchunk_e = std::max(1, std::min(atoi(v), c->ntt));
  c->tpc_e = (c->ntt + c->nchunk_e - 1) / c->nchunk_e;
  c->nchunk_e = (c->ntt + c->tpc_e - 1) / c->tpc_e;
  // The single-pass E-step's schedule (k_estep_mx, J <= 8; fasst_esched.h).
  // FASST_ESTEP_SCHED=chunk | balanced picks it (read here, once per
  // configuration, like FASST_NCHUNK_E), FASST_ESTEP_NB sets the
  // balanced schedule's block count.  Balanced: one round of resident blocks,
  // each at least kEsMinUnits quad-steps (the per-segment prologue / epilogue
  // stays small, as with the chunks of >= 40 frame tiles above) but never
  // fewer blocks than bin tiles.
  c->esched = ESched{};
  c->esched.nbt = c->nft;
  c->esched.nslot = c->nchunk_e;
  {
    // (an explicit FASST_NCHUNK_E asks for the chunk grid)
    bool bal = kEsBalancedDefault && !getenv("FASST_NCHUNK_E");
    if (const char *v = getenv("FASST_ESTEP_SCHED")) bal = !strcmp(v, "balanced");
    const long long Q = (c->ntt + 3) / 4, U = (long long)c->nft * Q;
    if (bal && J <= 8 && U < (1ll << 30)) {
      long long nb = std::min(U, std::max<long long>(c->nft, std::min<long long>(cap_e, U / kEsMinUnits)));
      if (const char *v = getenv("FASST_ESTEP_NB")) nb = atoll(v);
      nb = std::max(1ll, std::min(nb, U));
      c->esched.bal = 1;
      c->esched.nb = (int)nb;
      c->esched.Q = (int)Q;
      c->esched.nslot = es_max_slots(c->nft, (int)Q, (int)nb);
    }
  }
  const long cap_b = (long)contract_occupancy(c) * ncu;
  c->nchunk_b = best_split((long)((c->nft + kFPW - 1) / kFPW) * J, cap_b, c->ntt / 32);
  if (const char *v = getenv("FASST_NCHUNK_B")) c->nchunk_b = std::max(1, std::min(atoi(v), c->ntt));
  c->tpc_b = (c->ntt + c->nchunk_b - 1) / c->nchunk_b;
  c->nchunk_b = (c->ntt + c->tpc_b - 1) / c->tpc_b;
  // (the bin split also multiplies k_tw_update's reduction: a fixed, small
  // split measured best at C3)
  c->nsplit_t = std::max(1, std::min(4, c->nft / 32));
  int tw_units = 0, tw_tiles = 0;
  const long cap_t = (long)twl_occupancy(c, false, &tw_units, &tw_tiles) * ncu;
  if ((long)tw_units * J * c->nsplit_t < cap_t)
    c->nsplit_t = best_split((long)tw_units * J, cap_t, c->nft / 16);
  if (const char *v = getenv("FASST_NSPLIT_T")) c->nsplit_t = std::max(1, std::min(atoi(v), c->nft));
  c->fpc_t = (c->nft + c->nsplit_t - 1) / c->nsplit_t;
  c->nsplit_t = (c->nft + c->fpc_t - 1) / c->fpc_t;
  // k_tw_contract_lds's schedule (the single-component path; fasst_twsched.h).
  // FASST_TWC_SCHED=grid | balanced picks it (read here, once per
  // configuration), FASST_TWC_NB sets the balanced schedule's block count:
  // by default one round of resident blocks.
  c->twsched = TwSched{};
  c->twsched.nslot = c->nsplit_t;
  long cap_tb = 0;
  {
    // (an explicit FASST_NSPLIT_T asks for the grid)
    bool bal = kTwcBalancedDefault && !getenv("FASST_NSPLIT_T");
    if (const char *v = getenv("FASST_TWC_SCHED")) bal = !strcmp(v, "balanced");
    // (k_tw_update's 64-frame blocks each lie inside one frame group)
    if (bal && tw_tiles % 4 == 0 && (long long)J * tw_units * c->nft < (1ll << 30)) {
      cap_tb = (long)twl_occupancy(c, true, &tw_units, &tw_tiles) * ncu;
      long long nb = cap_tb;
      if (const char *v = getenv("FASST_TWC_NB")) nb = atoll(v);
      c->twsched = tws_make(J, tw_units, 16 * tw_tiles, c->nft, nb);
    }
  }
  if (getenv("FASST_VERBOSE"))
    fprintf(stderr,
            "fasst: %d CUs; estep %d %s, %d slots (cap %ld blocks); fb %d chunks (cap %ld); tw %d "
            "%s, %d slots (cap %ld)\n",
            ncu, c->esched.bal ? c->esched.nb : c->nchunk_e,
            c->esched.bal ? "balanced blocks" : "chunks", c->esched.nslot, cap_e, c->nchunk_b, cap_b,
            c->twsched.bal ? c->twsched.nb : c->nsplit_t, c->twsched.bal ? "persistent blocks" : "splits",
            c->twsched.nslot, c->twsched.bal ? cap_tb : cap_t);
  const int NP = J * (J + 1) / 2;
  c->nacc = 4 * NP + 8 * J;
  int st;
#define ALLOC(buf, n) \
  if ((st = c->buf.alloc(n)) != FASST_OK) return st
  ALLOC(FB, (size_t)J * Fp * KP);
  ALLOC(FW, (size_t)J * KP * KP);
  ALLOC(TW, (size_t)J * KP * Tp);
  ALLOC(Wkf, (size_t)J * KP * Fp);
  ALLOC(Wkf_new, (size_t)J * KP * Fp);
  ALLOC(Wfk_new, (size_t)J * Fp * KP);
  ALLOC(FWHt, (size_t)J * Tp * KP);
  ALLOC(hatW, (size_t)J * Tp * Fp);
  ALLOC(A, (size_t)R * 2 * Fp);
  ALLOC(Pinst, (size_t)R * 2);
  // (+8 chunks: the interleaved E-step / FB ranges round their chunks up)
  ALLOC(epart, (size_t)(c->esched.nslot + 8) * Fp * c->nacc);
  ALLOC(llpart, (size_t)(c->esched.nslot + 8) * c->nft);
  ALLOC(bnum, (size_t)(c->nchunk_b + 8) * J * Fp * KP);
  // FW update (free FW only, allocated with the model so set_spectral may switch it on)
  ALLOC(gden, (size_t)c->nchunk_b * J * Fp * KP);
  ALLOC(TWt, (size_t)J * Tp * KP);
  ALLOC(pnum, (size_t)((c->F + fw_fpc(c) - 1) / fw_fpc(c)) * J * KP * KP);
  ALLOC(pden, (size_t)((c->F + fw_fpc(c) - 1) / fw_fpc(c)) * J * KP * KP);
  // (the multi-block path keeps the static split whatever the schedule)
  const int tslots = std::max(c->nsplit_t, c->twsched.nslot);
  ALLOC(tnum, (size_t)tslots * J * Tp * KP);
  ALLOC(tden, (size_t)tslots * J * Tp * KP);
  ALLOC(rss, conv ? 0 : (size_t)Fp * R * R);
  ALLOC(rxs, conv ? 0 : (size_t)Fp * 2 * R);
  ALLOC(flags, kNFlags);
  ALLOC(hsum, (size_t)J * KP);
  // renormalisation chunks (every stage-2 block re-reduces all stage-1
  // partials, so more chunks measured slower at C3)
  c->nchunk_r = std::max(1, std::min(64, std::min((c->T + 255) / 256, (c->F + 15) / 16)));
  ALLOC(rscal, (size_t)J * (2 + 2 * KP));
  ALLOC(rpmax, (size_t)J * c->nchunk_r * KP);
  ALLOC(rpe, (size_t)J * c->nchunk_r);
  ALLOC(rtpart, (size_t)kMaxSlot * c->nchunk_r);
  c->ntb = (Tp + 63) / 64;
  ALLOC(rpmax2, (size_t)J * c->nft * KP);
  ALLOC(rtpart2, (size_t)kMaxSlot * c->ntb);
  ALLOC(Wkf_next, (size_t)J * KP * Fp);
  ALLOC(hpart, (size_t)J * KP * c->ntb);
  if (J > 8 && KP > 32) {   // the two-pass E-step's scratch: V_j, N, P planes and per-tile logliks
    ALLOC(vgen, (size_t)J * Tp * Fp);
    ALLOC(npgen, (size_t)12 * Tp * Fp);
    ALLOC(lgen, (size_t)c->ntt * c->nft);
  } else {
    c->vgen.release();
    c->npgen.release();
    c->lgen.release();
  }
  c->w_ready = c->prep_ready = 0;
  // the E-step's operand images follow the model: the TW image its J and KP
  // (re-allocated by the next iteration), the Cx image whether it is read
  c->twp.release();
  if (!estep_cxi(c)) {
    c->cxp.release();
    c->cxp_valid = false;
  }
#undef ALLOC
  c->configured = 1;
  return FASST_OK;
}

int build_inst_A(fasst_ctx *c) {
  if (c->conv) return FASST_OK;
  unsigned rowm = 0;
  for (int j = 0; j < c->J; ++j)
    if (!(c->convm >> j & 1u))
      for (int r = c->roff[j]; r < c->roff[j + 1]; ++r) rowm |= 1u << r;
  prof_begin(c, KINSTA);
  k_inst_A<<<egrid((size_t)c->R * 2 * c->Fp), 256, 0, c->stream>>>(c->Pinst.p, c->A.p, c->R,
                                                                        c->F, c->Fp, rowm, c->halt);
  prof_end(c, KINSTA);
  FASST_LAUNCH_CHECK();
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

static void update_multi(fasst_ctx *c) {
  c->anytb = 0;
  for (int j = 0; j < c->J; ++j)
    for (int b = 0; b < c->nblk[j]; ++b) c->anytb |= c->tbl[j][b] > 0;
  c->multi = c->maxblk > 1 || c->lambda > 0.0 || c->anytb;
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

static RArgs renorm_args(fasst_ctx *c) {
  RArgs r{};
  r.A = c->A.p;
  r.Pinst = c->Pinst.p;
  r.FB = c->FB.p;
  r.FW = c->FW.p;
  r.TW = c->TW.p;
  r.scal = c->rscal.p;
  r.pmax = c->rpmax.p;
  r.pe = c->rpe.p;
  r.tpart = c->rtpart.p;
  r.flags = c->flags.p;
  r.halt = c->halt;
  r.F = c->F;
  r.T = c->T;
  r.Fp = c->Fp;
  r.Tp = c->Tp;
  r.KP = c->KP;
  r.convm = c->convm;
  r.nchunk = c->nchunk_r;
  r.tpc = (c->T + c->nchunk_r - 1) / c->nchunk_r;
  r.fpc = (c->F + c->nchunk_r - 1) / c->nchunk_r;
  r.nslot = c->nslot;
  r.tbmask = 0;
  for (int j = 0; j < c->J; ++j)
    for (int b = 0; b < c->nblk[j]; ++b)
      if (c->tbl[j][b] > 0) r.tbmask |= 1u << (c->soff[j] + b);
  for (int j = 0; j < kMaxJ; ++j) {
    r.K[j] = j < c->J ? c->K[j] : 0;
    r.nblk[j] = j < c->J ? c->nblk[j] : 0;
    for (int b = 0; b <= kMaxBlk; ++b) r.kb[j][b] = j < c->J ? c->kb[j][b] : 0;
  }
  for (int j = 0; j <= kMaxJ; ++j) {
    r.roff[j] = j <= c->J ? c->roff[j] : c->R;
    r.soff[j] = j <= c->J ? c->soff[j] : c->nslot;
  }
  r.pmax2 = c->rpmax2.p;
  r.tpart2 = c->rtpart2.p;
  r.llpart = c->llpart.p;
  r.ll_out = nullptr;
  r.inv_FT = 1.0 / ((double)c->F * (double)c->T);
  r.nstat = c->nft;
  r.ntb = c->ntb;
  r.es = c->esched;
  return r;
}

static int launch_renorm(fasst_ctx *c, int iter) {
  RArgs r = renorm_args(c);
  prof_begin(c, KREN);
  k_renorm_stats<<<dim3(c->nchunk_r, c->J), 256, 0, c->stream>>>(r);
  if (c->nchunk_r * c->KP > 64 * 64 || c->KP > 64)
    k_renorm_apply<true><<<dim3(c->nchunk_r, c->J), 256, 0, c->stream>>>(r);
  else
    k_renorm_apply<false><<<dim3(c->nchunk_r, c->J), 256, 0, c->stream>>>(r);
  k_renorm_final<<<1, 256, 0, c->stream>>>(r, c->J, iter);
  FASST_LAUNCH_CHECK();
  if (c->anytb) {
    TBRArgs tr{};
    tr.scal = c->rscal.p;
    tr.flags = c->flags.p;
    tr.halt = c->halt;
    tr.T = c->T;
    tr.Tp = c->Tp;
    tr.KP = c->KP;
    tr.iter = iter;
    for (int j = 0; j < kMaxJ; ++j)
      for (int b = 0; b < kMaxBlk; ++b) {
        const bool on = j < c->J && b < c->nblk[j] && c->tbl[j][b] > 0;
        tr.tb[j][b] = on ? c->tb[j][b].p : nullptr;
        tr.L[j][b] = on ? c->tbl[j][b] : 0;
        tr.kb0[j][b] = on ? c->kb[j][b] : 0;
        tr.kbw[j][b] = on ? c->kb[j][b + 1] - c->kb[j][b] : 0;
        tr.slot[j][b] = on ? c->soff[j] + b : 0;
      }
    k_tb_renorm<<<dim3(kMaxBlk, c->J), 256, 0, c->stream>>>(tr);
    FASST_LAUNCH_CHECK();
    for (int b = 0; b < c->maxblk; ++b) {
      TBArgs ta = tb_args(c, b, -1, 0, 1.0);
      ta.flags = c->flags.p;
      ta.iter = iter;
      if (int st = launch_tb_h(c, ta)) return st;
    }
  }
  prof_end(c, KREN);
  return FASST_OK;
}

// gem_iteration's fused renormalisation tail (§3.3a of DESIGN.md; see
// k_renorm_scales), the default for the structures it covers: one spectral
// component per source (!multi), no time blobs (!anytb), no free FW.  The
// context's ftail (FASST_FAST_TAIL, read at creation) selects the form:
//   0  the unfused k_renorm_stats / _apply / _final (the A/B reference);
//   1  the fused tail: k_fb_update's stage-1 statistics, k_renorm_scales /
//      _rows and the next W on the side stream beside the TW contraction,
//      the TW rescale inside k_tw_update, k_renorm_tail;
//   2  (default) as 1, and at KP <= 64 k_tw_update also forms the next
//      iteration's (FW.TW)^T and TW row-sum partials (reduced into hsum by
//      k_renorm_tail), so the next iteration of the batch skips
//      launch_spectral_prep.
// Every form is tested against the others and the oracle, halted batches
// included (tests/test_gpu_fast_tail.py).
static bool fast_tail(const fasst_ctx *c) {
  if (!c->ftail || c->multi || c->anytb || c->anytwc) return false;
  for (int j = 0; j < c->J; ++j)
    if (c->fw_free[j]) return false;
  return true;
}

// update_mix_matrix (audioModel.py:766-889) on stream s: k_mix (per-bin
// statistics, hat_Rss / hat_Rxs, the 'conv' solves) and k_mix_inst (the
// 'inst' f-mean solve), when some spatial component is free
static int launch_mix(fasst_ctx *c, hipStream_t s) {
  const int J = c->J;
  bool any_free = false;
  for (int j = 0; j < J; ++j) any_free |= c->spat_free[j] != 0;
  if (any_free) {
    MArgs m{};
    m.part = c->epart.p;
    m.Wkf = c->Wkf.p;
    m.hsum = c->hsum.p;
    m.KP = c->KP;
    m.A = c->A.p;
    m.rss = c->rss.p;
    m.rxs = c->rxs.p;
    m.flags = c->flags.p;
    m.halt = c->halt;
    m.F = c->F;
    m.Fp = c->Fp;
    m.J = J;
    m.R = c->R;
    m.es = c->esched;
    m.nacc = c->nacc;
    m.conv_update = c->conv ? 1 : 0;
    m.invT = 1.0 / (double)c->T;
    for (int j = 0; j < J; ++j)
      for (int r = c->roff[j]; r < c->roff[j + 1]; ++r) m.jr[r] = j;
    prof_begin(c, KMIX, s);
    {
      const size_t ms = mix_smem(J, c->R, c->KP, c->nacc);
      const int q = (c->nacc + 63) / 64;
      constexpr int QX = (4 * (kMaxJ * (kMaxJ + 1) / 2) + 8 * kMaxJ + 63) / 64;
      if (c->R > 16) {   // (R^2 > 256 hat_Rss entries: 16 per lane; up to ~73 KB of LDS)
        k_mix<QX, (kMaxR * kMaxR + 63) / 64><<<c->F, 64, ms, s>>>(m);
      }
      else if (q <= 2)
        k_mix<2><<<c->F, 64, ms, s>>>(m);
      else if (q <= 4)   // (J <= 8: 4 J (J + 1) / 2 + 8 J <= 208)
        k_mix<4><<<c->F, 64, ms, s>>>(m);
      else
        k_mix<QX><<<c->F, 64, ms, s>>>(m);
    }
    prof_end(c, KMIX, s);
    FASST_LAUNCH_CHECK();
    if (!c->conv) {
      IArgs ia{};
      ia.rss = c->rss.p;
      ia.rxs = c->rxs.p;
      ia.A = c->A.p;
      ia.Pinst = c->Pinst.p;
      ia.flags = c->flags.p;
      ia.halt = c->halt;
      ia.F = c->F;
      ia.Fp = c->Fp;
      ia.R = c->R;
      ia.nu = ia.no = 0;
      for (int j = 0; j < J; ++j)
        for (int r = c->roff[j]; r < c->roff[j + 1]; ++r) {
          if (c->spat_free[j])
            ia.upd[ia.nu++] = r;
          else
            ia.oth[ia.no++] = r;
        }
      prof_begin(c, KMIXI, s);
      k_mix_inst<<<1, 256, 0, s>>>(ia);
      prof_end(c, KMIXI, s);
      FASST_LAUNCH_CHECK();
    }
  }
  return FASST_OK;
}

// the scales and the FB / mixing / FW rescale, after k_fb_update: on the side
// stream beside the TW contraction; ev_scales gates k_tw_update, ev_rows the
// iteration's end
static int launch_tail_side(fasst_ctx *c) {
  const RArgs r = renorm_args(c);
  hipStream_t side = c->aux;
  FASST_HIP(hipEventRecord(c->ev_tail, c->stream));
  FASST_HIP(hipStreamWaitEvent(c->aux, c->ev_tail, 0));
  prof_begin(c, KREN, side);
  k_renorm_scales<<<c->J, 1024, 0, side>>>(r);
  FASST_LAUNCH_CHECK();
  FASST_HIP(hipEventRecord(c->ev_scales, c->aux));
  k_renorm_rows<<<dim3(c->nft, c->J), 256, 0, side>>>(r);
  FASST_LAUNCH_CHECK();
  prof_end(c, KREN, side);
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
static int launch_spectral_prep(fasst_ctx *c, bool fork) {
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
static int spectral_update(fasst_ctx *c, double omega, bool tail = false) {
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

// the fused tail's last launch (k_renorm_tail: the loglik and, with prep, the
// next iteration's TW row sums), after the side stream's ev_rows
static int launch_renorm_tail(fasst_ctx *c, double *ll_dev, int iter, bool prep) {
  FASST_HIP(hipStreamWaitEvent(c->stream, c->ev_rows, 0));
  RArgs r = renorm_args(c);
  r.ll_out = ll_dev;
  r.hpart = prep ? c->hpart.p : nullptr;
  r.hsum = c->hsum.p;
  r.J = c->J;
  prof_begin(c, KRTAIL);
  k_renorm_tail<<<1 + (prep ? (c->J * c->KP + 3) / 4 : 0), 256, 0, c->stream>>>(r, iter);
  prof_end(c, KRTAIL);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// One GEM iteration, all launches asynchronous on c->stream.
static int gem_iteration(fasst_ctx *c, const double *psd_dev, double *ll_dev, double omega,
                         int iter) {
  const int J = c->J;
  if (!c->conv) {
    // a free 'conv' component next to other components: the reference's conv
    // solve (audioModel.py:856-857) passes the full hat_Rss[f].T against the
    // free components' right-hand side only, and np.linalg.solve raises
    for (int j = 0; j < J; ++j)
      if ((c->convm >> j & 1u) && c->spat_free[j]) {
        set_error("spatial component %d is 'conv' and free next to other components: the "
                  "reference's mixing solve (audioModel.py:856-857) raises for this structure",
                  j);
        return FASST_ERR_UNSUPPORTED;
      }
  }
  // (FW.TW)^T and the TW row sums depend only on the previous iteration's
  // parameters: forked onto the side stream beside the E-step (unless the
  // previous iteration's fused tail in the same batch formed them)
  const bool prep_ready = c->prep_ready;
  c->prep_ready = 0;
  int st = prep_ready ? FASST_OK : launch_spectral_prep(c, true);
  if (st) return st;
  const bool w_ready = c->w_ready;   // (the previous iteration's fused tail formed W)
  c->w_ready = 0;
  if (!w_ready && (st = launch_w_old(c))) return st;
  st = build_inst_A(c);
  if (st) return st;
  if ((st = launch_estep_phase(c, psd_dev, prep_ready))) return st;
  if (!prep_ready) FASST_HIP(hipStreamWaitEvent(c->stream, c->ev_join, 0));  // hsum, FWHt below
  const bool ft = fast_tail(c);
  if (!ft && (st = launch_loglik(c, ll_dev))) return st;   // (fused tail: summed by k_renorm_tail)
  // mixing update (update_mix_matrix, :766-889).  (On the side stream beside
  // the TW contraction instead, after the FB update: k_mix stretched to 0.18
  // ms and took 23 us from the TW contraction and 14 us from the FB
  // contraction for the 30 us it left the critical path; profiles/r6_ab_mix_side.txt)
  if ((st = launch_mix(c, c->stream))) return st;
  if ((st = spectral_update(c, omega, ft))) return st;
  if (!ft) return launch_renorm(c, iter);
  const bool prep = c->ftail >= 2 && c->KP <= 64;   // (spectral_update's k_tw_update formed FWHt)
  if ((st = launch_renorm_tail(c, ll_dev, iter, prep))) return st;
  std::swap(c->Wkf.p, c->Wkf_next.p);
  c->w_ready = 1;
  c->prep_ready = prep;
  return FASST_OK;
}

}  // namespace fasst

using namespace fasst;

// ============================================================================ C ABI
extern "C" {

const char *fasst_last_error(void) { return fasst::g_err.c_str(); }

int fasst_abi_version(void) { return FASST_ABI_VERSION; }

int fasst_estep_partition(int nbt, int Q, int nb, long long *lo, int *first, int *nseg,
                          int *max_slots) {
  if (nbt < 1 || Q < 1 || nb < 1 || (long long)nbt * Q >= (1ll << 30) || nb > (long long)nbt * Q) {
    set_error("fasst_estep_partition: need 1 <= nb <= nbt Q < 2^30 (nbt=%d Q=%d nb=%d)", nbt, Q, nb);
    return FASST_ERR_SHAPE;
  }
  const long long U = (long long)nbt * Q;
  if (lo)
    for (int b = 0; b <= nb; ++b) lo[b] = es_lo(b, U, nb);
  for (int bt = 0; bt < nbt; ++bt) {
    if (first) first[bt] = es_first(bt, Q, nbt, nb);
    if (nseg) nseg[bt] = es_nseg(bt, Q, nbt, nb);
  }
  if (max_slots) *max_slots = es_max_slots(nbt, Q, nb);
  return FASST_OK;
}

int fasst_device_count(int *n) {
  FASST_HIP(hipGetDeviceCount(n));
  return FASST_OK;
}

int fasst_create(int device, int F, int T, fasst_ctx **out) {
  if (!out || F < 1 || T < 1) {
    set_error("fasst_create: bad arguments F=%d T=%d", F, T);
    return FASST_ERR_SHAPE;
  }
  int ndev = 0;
  FASST_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) {
    set_error("fasst_create: device %d not present (%d visible)", device, ndev);
    return FASST_ERR_DEVICE;
  }
  DeviceGuard g(device);
  fasst_ctx *c = new fasst_ctx();
  c->device = device;
  c->F = F;
  c->T = T;
  c->Fp = round_up(F, kTile);
  c->Tp = round_up(T, kTile);
  c->nft = c->Fp / kTile;
  c->ntt = c->Tp / kTile;
  if (const char *v = getenv("FASST_FAST_TAIL")) c->ftail = atoi(v);
  if (const char *v = getenv("FASST_ESTEP_IMG"))
    c->eimg = !strcmp(v, "cx") ? 1 : (!strcmp(v, "tw") ? 2 : (!strcmp(v, "0") ? 0 : 3));
  int st = FASST_OK;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_scales, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_rows, hipEventDisableTiming) != hipSuccess) {
    set_error("hipStreamCreate / hipEventCreate failed");
    st = FASST_ERR_DEVICE;
  }
  if (!st) st = c->cx.alloc((size_t)4 * c->Tp * c->Fp);
  if (!st && hipHostMalloc((void **)&c->h_flags, kNFlags * sizeof(int)) != hipSuccess)
    st = FASST_ERR_OOM;
  if (!st && hipHostMalloc((void **)&c->h_ll, 64 * sizeof(double)) != hipSuccess) st = FASST_ERR_OOM;
  if (st) {
    fasst_destroy(c);
    return st;
  }
  *out = c;
  return FASST_OK;
}

int fasst_configure_types(fasst_ctx *c, int J, const int *rank, const int *K,
                          const int *mix_conv) {
  if (!c || !rank || !K || !mix_conv) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  return configure_model(c, J, rank, K, mix_conv);
}

int fasst_configure(fasst_ctx *c, int J, const int *rank, const int *K, int mix_conv) {
  if (!c || !rank || !K) return FASST_ERR_SHAPE;
  if (J < 1 || J > kMaxJ) return configure_model(c, J, rank, K, nullptr);
  int types[kMaxJ];
  for (int j = 0; j < J; ++j) types[j] = mix_conv ? 1 : 0;
  DeviceGuard g(c->device);
  return configure_model(c, J, rank, K, types);
}

int fasst_destroy(fasst_ctx *c) {
  if (!c) return FASST_OK;
  {
    DeviceGuard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    sf_release(c);
    if (c->h_flags) (void)hipHostFree(c->h_flags);
    if (c->h_ll) (void)hipHostFree(c->h_ll);
    c->cx.release();
    c->cxp.release();
    c->twp.release();
    c->X.release();
    c->FB.release();
    c->FW.release();
    c->TW.release();
    c->Wkf.release();
    c->Wkf_new.release();
    c->Wfk_new.release();
    c->FWHt.release();
    c->hatW.release();
    c->A.release();
    c->Pinst.release();
    c->epart.release();
    c->llpart.release();
    c->bnum.release();
    c->tnum.release();
    c->tden.release();
    c->psd.release();
    c->ll.release();
    c->rss.release();
    c->rxs.release();
    c->flags.release();
    c->hsum.release();
    c->rscal.release();
    c->rpmax.release();
    c->rpe.release();
    c->rtpart.release();
    c->rpmax2.release();
    c->rtpart2.release();
    c->hpart.release();
    c->vgen.release();
    c->npgen.release();
    c->lgen.release();
    c->Wkf_next.release();
    c->mplanes.release();
    c->bden.release();
    for (int i = 0; i < fasst_ctx::kNK; ++i) {
      for (int q = 0; q < fasst_ctx::kProfRing; ++q) {
        if (c->ev0[i][q]) (void)hipEventDestroy(c->ev0[i][q]);
        if (c->ev1[i][q]) (void)hipEventDestroy(c->ev1[i][q]);
      }
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
    if (c->ev_scales) (void)hipEventDestroy(c->ev_scales);
    if (c->ev_rows) (void)hipEventDestroy(c->ev_rows);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  delete c;
  return FASST_OK;
}

static int need_model(fasst_ctx *c, int j) {
  if (!c || !c->configured) {
    set_error("context not configured");
    return FASST_ERR_SHAPE;
  }
  if (j < 0 || j >= c->J) {
    set_error("component %d out of range (J=%d)", j, c->J);
    return FASST_ERR_SHAPE;
  }
  return FASST_OK;
}

int fasst_set_spatial(fasst_ctx *c, int j, const double *params, int free_) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  c->spat_free[j] = free_ ? 1 : 0;
  const int r0 = c->roff[j], nr = c->rank[j];
  const double2 *p = reinterpret_cast<const double2 *>(params);
  if (c->convm >> j & 1u) {
    // params [r][C][F] -> A[r][c][f] (row pitch Fp)
    FASST_TRY(c->A.at((size_t)2 * r0 * c->Fp, (size_t)2 * nr * c->Fp)
                  .put_rows(p, (size_t)nr * 2, c->F, c->F, c->Fp, c->stream));
  } else {
    // params [C][r] -> Pinst[r][c]
    std::vector<double2> tmp((size_t)nr * 2);
    for (int r = 0; r < nr; ++r)
      for (int ch = 0; ch < 2; ++ch) tmp[(size_t)r * 2 + ch] = p[(size_t)ch * nr + r];
    FASST_TRY(c->Pinst.at(2 * r0, tmp.size()).put(tmp.data(), tmp.size(), c->stream));
  }
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_get_spatial(fasst_ctx *c, int j, double *params) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  const int r0 = c->roff[j], nr = c->rank[j];
  double2 *p = reinterpret_cast<double2 *>(params);
  if (c->convm >> j & 1u) {
    FASST_TRY(c->A.at((size_t)2 * r0 * c->Fp, (size_t)2 * nr * c->Fp)
                  .get_rows(p, (size_t)nr * 2, c->F, c->F, c->Fp, c->stream));
    FASST_HIP(hipStreamSynchronize(c->stream));
  } else {
    std::vector<double2> tmp((size_t)nr * 2);
    FASST_TRY(c->Pinst.at(2 * r0, tmp.size()).get(tmp.data(), tmp.size(), c->stream));
    FASST_HIP(hipStreamSynchronize(c->stream));
    for (int r = 0; r < nr; ++r)
      for (int ch = 0; ch < 2; ++ch) p[(size_t)ch * nr + r] = tmp[(size_t)r * 2 + ch];
  }
  return FASST_OK;
}

int fasst_set_fw_prior(fasst_ctx *c, int j, int fw_free) {
  int st = need_model(c, j);
  if (st) return st;

  c->fw_free[j] = fw_free ? 1 : 0;
  if (c->nblk[j] == 1) c->bfw[j][0] = c->fw_free[j];
  return FASST_OK;
}

int fasst_set_blocks(fasst_ctx *c, int j, int nblk, const int *kb, const int *fb_free,
                     const int *fw_free, const int *tw_free) {
  int st = need_model(c, j);
  if (st) return st;
  if (nblk < 1 || nblk > kMaxBlk || !kb || !fb_free || !fw_free || !tw_free) {
    set_error("source %d: %d spectral components (1..%d on the HIP path)", j, nblk, kMaxBlk);
    return nblk > kMaxBlk ? FASST_ERR_UNSUPPORTED : FASST_ERR_SHAPE;
  }
  if (kb[0] != 0 || kb[nblk] != c->K[j]) {
    set_error("source %d: component blocks must cover its %d columns", j, c->K[j]);
    return FASST_ERR_SHAPE;
  }
  for (int b = 0; b < nblk; ++b)
    if (kb[b + 1] <= kb[b]) {
      set_error("source %d: empty or unordered component block %d", j, b);
      return FASST_ERR_SHAPE;
    }
  int nslot = 0, maxblk = 0;
  for (int i = 0; i < c->J; ++i) {
    const int n = i == j ? nblk : c->nblk[i];
    nslot += n;
    maxblk = std::max(maxblk, n);
  }
  if (nslot > kMaxSlot) {
    set_error("%d spectral components in all (max %d on the HIP path)", nslot, kMaxSlot);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(c->device);
  if (maxblk > 1) {
    const size_t plane = (size_t)c->J * c->Tp * c->Fp;
    if (c->mplanes.n < 5 * plane && (st = c->mplanes.alloc(5 * plane))) return st;
    const size_t nb = (size_t)c->nchunk_b * c->J * c->Fp * c->KP;
    if (c->bden.n < nb && (st = c->bden.alloc(nb))) return st;
  }
  bool same = c->nblk[j] == nblk;
  for (int b = 0; same && b <= nblk; ++b) same = c->kb[j][b] == kb[b];
  c->nblk[j] = nblk;
  if (nblk > 1 && c->twc[j]) {   // a discrete-state TW needs the source's only component
    c->twc[j] = c->twc_free[j] = c->anytwc = 0;
    for (int i = 0; i < c->J; ++i) c->anytwc |= c->twc[i] != 0;
  }
  for (int b = 0; b <= nblk; ++b) c->kb[j][b] = kb[b];
  bool fbf = false, twf = false, fwf = false;
  for (int b = 0; b < nblk; ++b) {
    c->bfb[j][b] = fb_free[b] ? 1 : 0;
    c->bfw[j][b] = fw_free[b] ? 1 : 0;
    c->btw[j][b] = tw_free[b] ? 1 : 0;
    fbf |= c->bfb[j][b] != 0;
    fwf |= c->bfw[j][b] != 0;
    twf |= c->btw[j][b] != 0;
  }
  c->fb_free[j] = fbf;
  c->fw_free[j] = fwf;
  c->tw_free[j] = twf;
  c->soff[0] = 0;
  for (int i = 0; i < c->J; ++i) c->soff[i + 1] = c->soff[i] + c->nblk[i];
  c->nslot = nslot;
  c->maxblk = maxblk;
  if (!same)   // the blocks moved: their time blobs go (an unchanged layout,
               // e.g. the per-iteration re-upload, keeps them and their buffers)
    for (int b = 0; b < kMaxBlk; ++b) {
      c->tb[j][b].release();
      c->tbl[j][b] = c->btb[j][b] = 0;
    }
  update_multi(c);
  return FASST_OK;
}

int fasst_set_corr(fasst_ctx *c, double lambda, int nseq, const int *seq_j, const int *seq_b) {
  int st = need_model(c, 0);
  if (st) return st;
  if (!(lambda >= 0.0) || (lambda > 0.0 && (nseq < 1 || nseq > kMaxSlot || !seq_j || !seq_b))) {
    set_error("fasst_set_corr: lambda %g with %d components", lambda, nseq);
    return FASST_ERR_SHAPE;
  }
  if (lambda > 0.0) {
    int seen[kMaxJ][kMaxBlk] = {{0}};
    for (int q = 0; q < nseq; ++q) {
      const int j = seq_j[q], b = seq_b[q];
      if (j < 0 || j >= c->J || b < 0 || b >= c->nblk[j] || seen[j][b]++) {
        set_error("fasst_set_corr: bad component (%d, %d) at position %d", j, b, q);
        return FASST_ERR_SHAPE;
      }
      c->seq_j[q] = j;
      c->seq_b[q] = b;
    }
    if (nseq != c->nslot) {
      set_error("fasst_set_corr: %d components given, the model has %d", nseq, c->nslot);
      return FASST_ERR_SHAPE;
    }
    DeviceGuard g(c->device);
    const size_t plane = (size_t)c->J * c->Tp * c->Fp;
    if (c->mplanes.n < 5 * plane && (st = c->mplanes.alloc(5 * plane))) return st;
    const size_t nb = (size_t)c->nchunk_b * c->J * c->Fp * c->KP;
    if (c->bden.n < nb && (st = c->bden.alloc(nb))) return st;
  }
  c->lambda = lambda;
  c->nseq = lambda > 0.0 ? nseq : 0;
  update_multi(c);
  return FASST_OK;
}

int fasst_set_tb(fasst_ctx *c, int j, int b, int L, const double *TW, const double *TB,
                 int tb_free) {
  int st = need_model(c, j);
  if (st) return st;
  if (b < 0 || b >= c->nblk[j] || L < 0 || L > kMaxTB || (L > 0 && (!TW || !TB))) {
    set_error("fasst_set_tb: source %d component %d with %d time blobs (1..%d)", j, b, L, kMaxTB);
    return L > kMaxTB ? FASST_ERR_UNSUPPORTED : FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  if (L == 0) {
    c->tb[j][b].release();
    c->tbl[j][b] = c->btb[j][b] = 0;
    update_multi(c);
    return FASST_OK;
  }
  const int kbw = c->kb[j][b + 1] - c->kb[j][b];
  const TBLayout o = tb_layout(kbw, L, c->Tp);
  const size_t plane = (size_t)c->J * c->Tp * c->Fp;
  if (c->mplanes.n < 6 * plane && (st = c->mplanes.alloc(6 * plane))) return st;
  const size_t nb = (size_t)c->nchunk_b * c->J * c->Fp * c->KP;
  if (c->bden.n < nb && (st = c->bden.alloc(nb))) return st;
  // a buffer large enough is reused (no hipMalloc / device-wide sync on the
  // per-iteration re-upload); either way it is zero-filled: TB's padding
  // frames stay 0
  if (c->tb[j][b].n < o.n) {
    if ((st = c->tb[j][b].alloc(o.n))) return st;
  } else {
    FASST_TRY(c->tb[j][b].zero(o.n, c->stream));
  }
  FASST_TRY(c->tb[j][b].at(o.tws).put(TW, (size_t)kbw * L, c->stream));
  FASST_TRY(c->tb[j][b].at(o.tb).put_rows(TB, L, c->T, c->T, c->Tp, c->stream));
  c->tbl[j][b] = L;
  c->btb[j][b] = tb_free ? 1 : 0;
  if (c->twc[j]) {   // time blobs and a discrete-state TW exclude each other (:1736-1742)
    c->twc[j] = c->twc_free[j] = c->anytwc = 0;
    for (int i = 0; i < c->J; ++i) c->anytwc |= c->twc[i] != 0;
  }
  update_multi(c);
  c->halt = nullptr;
  TBArgs a = tb_args(c, b, j, 0, 1.0);   // H = TW TB into the block's rows
  if ((st = launch_tb_h(c, a))) return st;
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_get_tb(fasst_ctx *c, int j, int b, double *TW, double *TB) {
  int st = need_model(c, j);
  if (st) return st;
  if (b < 0 || b >= c->nblk[j] || c->tbl[j][b] == 0) {
    set_error("fasst_get_tb: source %d component %d has no time blobs", j, b);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  const int kbw = c->kb[j][b + 1] - c->kb[j][b], L = c->tbl[j][b];
  const TBLayout o = tb_layout(kbw, L, c->Tp);
  if (TW)
    FASST_TRY(c->tb[j][b].at(o.tws).get(TW, (size_t)kbw * L, c->stream));
  if (TB) FASST_TRY(c->tb[j][b].at(o.tb).get_rows(TB, L, c->T, c->T, c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_set_spectral(fasst_ctx *c, int j, const double *FB, const double *FW, const double *TW,
                       int fb_free, int tw_free) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  const int K = c->K[j], KP = c->KP;
  c->fb_free[j] = fb_free ? 1 : 0;
  c->tw_free[j] = tw_free ? 1 : 0;
  if (c->nblk[j] == 1) {
    c->bfb[j][0] = c->fb_free[j];
    c->btw[j][0] = c->tw_free[j];
  }
  // source j's rows of the padded images FB [Fp][KP], FW [KP][KP], TW [KP][Tp]
  const DSpan<double> fb = c->FB.at((size_t)j * c->Fp * KP, (size_t)c->Fp * KP),
                      fw = c->FW.at((size_t)j * KP * KP, (size_t)KP * KP),
                      tw = c->TW.at((size_t)j * KP * c->Tp, (size_t)KP * c->Tp);
  FASST_TRY(fw.zero(fw.n, c->stream));
  FASST_TRY(fb.put_rows(FB, c->F, K, K, KP, c->stream));
  FASST_TRY(fw.put_rows(FW, K, K, K, KP, c->stream));
  FASST_TRY(tw.put_rows(TW, K, c->T, c->T, c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_get_spectral(fasst_ctx *c, int j, double *FB, double *FW, double *TW) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  const int K = c->K[j], KP = c->KP;
  if (FB)
    FASST_TRY(c->FB.at((size_t)j * c->Fp * KP, (size_t)c->Fp * KP)
                  .get_rows(FB, c->F, K, K, KP, c->stream));
  if (FW)
    FASST_TRY(c->FW.at((size_t)j * KP * KP, (size_t)KP * KP).get_rows(FW, K, K, K, KP, c->stream));
  if (TW)
    FASST_TRY(c->TW.at((size_t)j * KP * c->Tp, (size_t)KP * c->Tp)
                  .get_rows(TW, K, c->T, c->T, c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_spectral_update(fasst_ctx *c, const double *hat_W, double omega) {
  int st = need_model(c, 0);
  if (st) return st;
  if (!hat_W) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const size_t n = (size_t)c->J * c->F * c->T;
  DBuf<double> dh;
  if ((st = dh.alloc_uninit(n))) return st;
  FASST_TRY(dh.put(hat_W, n, c->stream));
  FASST_TRY(c->flags.zero(kNFlags, c->stream));
  c->halt = nullptr;
  if ((st = launch_spectral_prep(c, false)) || (st = launch_w_old(c))) return st;
  FASST_TRY(c->hatW.zero((size_t)c->J * c->Tp * c->Fp, c->stream));
  k_rho_from_hatw<<<dim3((c->F + 63) / 64, (c->T + 3) / 4, c->J), 256, 0, c->stream>>>(
      dh.p, c->Wkf.p, c->TW.p, c->hatW.p, c->F, c->T, c->Fp, c->Tp, c->KP);
  FASST_LAUNCH_CHECK();
  if ((st = spectral_update(c, omega))) return st;
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_renormalize(fasst_ctx *c, int *restart_mask) {
  int st = need_model(c, 0);
  if (st) return st;
  DeviceGuard g(c->device);
  FASST_TRY(c->flags.zero(kNFlags, c->stream));
  c->halt = nullptr;
  st = launch_renorm(c, 0);
  if (st) return st;
  FASST_TRY(c->flags.get(c->h_flags, kNFlags, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  int mask = 0;
  for (int sl = 0; sl < c->nslot; ++sl)
    if (c->h_flags[1 + sl]) mask |= 1 << sl;
  if (restart_mask) *restart_mask = mask;
  return FASST_OK;
}

int fasst_run(fasst_ctx *c, int n_iter, const double *psd, double omega, double *logliks,
              int *restart_mask, int *iters_done) {
  int st = need_model(c, 0);
  if (st) return st;
  if (n_iter < 0 || (n_iter > 0 && (!psd || !logliks))) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  if (iters_done) *iters_done = 0;
  if (restart_mask) *restart_mask = 0;
  if (n_iter == 0) return FASST_OK;
  if (c->psd_cap < n_iter) {
    if ((st = c->psd.alloc((size_t)n_iter * c->Fp))) return st;
    c->psd_cap = n_iter;
  }
  if (c->ll_cap < n_iter) {
    if ((st = c->ll.alloc(n_iter))) return st;
    c->ll_cap = n_iter;
  }
  FASST_TRY(c->psd.zero((size_t)n_iter * c->Fp, c->stream));
  FASST_TRY(c->psd.at(0).put_rows(psd, n_iter, c->F, c->F, c->Fp, c->stream));
  FASST_TRY(c->flags.zero(kNFlags, c->stream));
  // Without profiling the whole batch is enqueued at once: a flag raised in
  // iteration i halts every later kernel on the device (HALT_GUARD), and the
  // host reads the flags once at the end.  Profiling keeps one sync per
  // iteration so the per-kernel events can be folded.
  c->halt = c->flags.p + kFlagHalt;
  c->w_ready = c->prep_ready = 0;
  const int sync_every = c->prof ? fasst_ctx::kProfRing : n_iter;
  int done = 0;
  for (int it = 0; it < n_iter; ++it) {
    c->pslot = it % fasst_ctx::kProfRing;
    st = gem_iteration(c, c->psd.p + (size_t)it * c->Fp, c->ll.p + it, omega, it);
    if (st) {
      c->halt = nullptr;
      return st;
    }
    if ((it + 1) % sync_every && it + 1 < n_iter) continue;
    FASST_TRY(c->flags.get(c->h_flags, kNFlags, c->stream));
    FASST_HIP(hipStreamSynchronize(c->stream));
    prof_collect(c);
    done = it + 1;
    if (c->h_flags[kFlagHalt] || c->h_flags[0]) break;
  }
  c->halt = nullptr;
  // a halted batch skipped its later iterations' kernels while the host still
  // swapped the fused tail's W buffers: rebuild W = FB.FW from the parameters
  if (c->w_ready && (c->h_flags[kFlagHalt] || c->h_flags[0])) {
    if ((st = launch_w_old(c))) return st;
    FASST_HIP(hipStreamSynchronize(c->stream));
  }
  c->w_ready = c->prep_ready = 0;
  if (c->h_flags[0]) {
    set_error("Singular Matrix");
    return FASST_ERR_SINGULAR;
  }
  int mask = 0;
  for (int sl = 0; sl < c->nslot; ++sl)
    if (c->h_flags[1 + sl]) mask |= 1 << sl;
  if (mask) done = c->h_flags[kFlagIter] + 1;
  if (iters_done) *iters_done = done;
  FASST_TRY(c->ll.get(logliks, done));
  if (mask) {
    if (restart_mask) *restart_mask = mask;
    return FASST_TW_RESTART;
  }
  return FASST_OK;
}

int fasst_set_profiling(fasst_ctx *c, int on) {
  if (!c) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  if (on && !c->ev0[0][0])
    for (int i = 0; i < fasst_ctx::kNK; ++i)
      for (int q = 0; q < fasst_ctx::kProfRing; ++q) {
        FASST_HIP(hipEventCreate(&c->ev0[i][q]));
        FASST_HIP(hipEventCreate(&c->ev1[i][q]));
      }
  c->prof = on ? 1 : 0;
  c->pslot = 0;
  for (int i = 0; i < fasst_ctx::kNK; ++i) {
    c->prof_ms[i] = 0.0;
    c->prof_cnt[i] = 0;
    for (int q = 0; q < fasst_ctx::kProfRing; ++q) c->used[i][q] = 0;
  }
  return FASST_OK;
}

int fasst_kernel_times(fasst_ctx *c, double *avg_ms, long *counts, int nk) {
  if (!c || !avg_ms) return FASST_ERR_SHAPE;
  for (int i = 0; i < nk && i < fasst_ctx::kNK; ++i) {
    avg_ms[i] = c->prof_cnt[i] ? c->prof_ms[i] / (double)c->prof_cnt[i] : 0.0;
    if (counts) counts[i] = c->prof_cnt[i];
  }
  return fasst_ctx::kNK;
}

const char *fasst_kernel_name(int i) {
  return (i >= 0 && i < fasst_ctx::kNK) ? kKernelNames[i] : "";
}

}  // extern "C"
