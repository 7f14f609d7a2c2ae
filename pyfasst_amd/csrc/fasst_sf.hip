// Two-factor (source / filter) spectral components on the device: the "planar"
// GEM path.  V_j = prod_i P_{j,i}, P_{j,i} = (FB_i.FW_i).TW_i, every power an
// F x T plane (comp_spat_comp_power, audioModel.py:430-498; the multi-factor
// branches of update_spectral_components :1469-1727 and renormalize_parameters
// :1980-2040).  Kept beside the single-factor kernels of fasst_em_*.hip: a model
// without a two-factor component never reaches this file.
//
// Per GEM iteration (sf_iteration):
//   powers    W = FB.FW, P = W.TW on the FP64 MFMA GEMM (k_gemm, 16x16x4),
//             V_j by k_sf_prod
//   E-step    k_suff_stat on the resident planes (rank r reads plane vmap[r])
//   mixing    k_mix_solve_inst / k_mix_solve_conv, hat_W_j = mean_r hat_Ws
//   spectral  per source, per factor: `other` once (k_sf_other), then per free
//             matrix k_sf_ratio (other / V and hat_W other / V^2 from the resident
//             planes, nothing else written), the contraction on the MFMA GEMM
//             (split-K slabs summed in fixed order) and k_sf_update
//   renorm    k_sf_energy per source, k_sf_renorm per factor (the energy handed
//             from factor to factor as the reference does)
// Every reduction has a fixed order: two runs are bit-equal.
//
// Between iterations, for a model with sparsity lengths (fasst_sf_run_sparse,
// fasst_sf_reweigh): reweigh_sparsity_constraint (:2981-3014) on factor 0's
// TW, k_sf_bary then k_sf_sparsify per component.
#include "fasst_sf.h"
#include "fasst_cqt_dev.h"
#include "fasst_fft.h"
#include "../../include/fasst_cqt.h"
#include "fasst_gemm.h"

#include <algorithm>
#include <cmath>

namespace fasst {

enum { KSF_GEMM = fasst_ctx::kSfSlot0, KSF_PROD, KSF_RATIO, KSF_UPDATE, KSF_RENORM, KSF_WIENER, KSF_OTHER,
       KSF_HATW, KSF_ENERGY, KSF_BARY, KSF_SPARSIFY, KSFW_SCALE, KSFW_DGEMM2, KSFW_UPDATE, KSFW_RENORM };
static_assert(KSFW_RENORM == fasst_ctx::kNK - 1, "one profiling slot per kernel of this file");
static inline void sf_count(fasst_ctx *c, int id) {
  if (c->prof) c->prof_cnt[id] += 1;
}

constexpr size_t kSfGridCap = 16384;  // blocks of this file's element-wise launches

// V = P0 (one factor) or P0 P1
__global__ void k_sf_prod(const double *__restrict__ P0, const double *__restrict__ P1,
                          double *__restrict__ V, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    V[i] = P1 ? P0[i] * P1[i] : P0[i];
}

// other = max(prod of the other factors, eps); a one-factor component: its own
// power, Po = that plane either way
__global__ void k_sf_other(const double *__restrict__ Po, double *__restrict__ other, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    other[i] = fmax(Po[i], kEps);
}

// Vj = max(Ps Po, eps) (Po == nullptr: one factor): rd = other (1 / Vj),
// rn = hat_W / Vj^2 other  (audioModel.py:1544-1573, lambdaCorr == 0)
__global__ void k_sf_ratio(const double *__restrict__ Ps, const double *__restrict__ Po,
                           const double *__restrict__ other, const double *__restrict__ hatW,
                           double *__restrict__ rn, double *__restrict__ rd, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double v = fmax(Po ? Ps[i] * Po[i] : Ps[i], kEps), o = other[i];
    rd[i] = o * (1.0 / v);
    rn[i] = hatW[i] / (v * v) * o;
  }
}

// P[r][c] *= (num / max(den, eps))^omega; tr: num / den are stored [cols][rows]
__global__ void k_sf_update(double *__restrict__ P, int rows, int cols, const double *__restrict__ num,
                            const double *__restrict__ den, int tr, double omega) {
  const size_t n = (size_t)rows * cols;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t q = tr ? (i % cols) * (size_t)rows + i / cols : i;
    const double g = num[q] / fmax(den[q], kEps);
    P[i] *= omega == 1.0 ? g : pow(g, omega);
  }
}

// hat_W_j = mean over the ranks of source j of hat_Ws (audioModel.py:414-416)
__global__ void k_sf_hatw(const double *__restrict__ ws, double *__restrict__ hatW, int r0, int nr,
                          size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int r = 0; r < nr; ++r) s += ws[(size_t)(r0 + r) * n + i];
    hatW[i] = s / (double)nr;
  }
}

// renormalize_parameters, the spatial half (:1993-1999), one block per source:
// energy = mean |params|^2 ('inst': the C x r matrix, bin 0 of its constant
// rows; 'conv': r x C x F), params /= sqrt(energy)
__global__ __launch_bounds__(256) void k_sf_energy(double2 *__restrict__ mix, int F, const int *__restrict__ roff,
                                                   const int *__restrict__ conv, double *__restrict__ energy) {
  __shared__ double s_red[256];
  const int j = blockIdx.x, r0 = roff[j], r1 = roff[j + 1], cv = conv[j];
  const int nf = cv ? F : 1;
  const size_t n = (size_t)(r1 - r0) * 2 * nf;
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += 256) {
    const double2 z = mix[(size_t)r0 * 2 * F + (i / nf) * F + i % nf];
    s += z.x * z.x + z.y * z.y;
  }
  const double e = block_sum(s, s_red) / (double)n;
  const double q = sqrt(e);
  for (size_t i = threadIdx.x; i < (size_t)(r1 - r0) * 2 * F; i += 256) {
    double2 z = mix[(size_t)r0 * 2 * F + i];
    z.x /= q;
    z.y /= q;
    mix[(size_t)r0 * 2 * F + i] = z;
  }
  if (threadIdx.x == 0) energy[j] = e;
}

// renormalize_parameters of one factor (:2003-2036), one block: FB *= energy;
// column max of FB -> FW; column mean of FW -> TW; sum(TW) < eps: restart flag
// (the host redraws and finishes); else TW /= mean(TW) unless the last factor.
// The reference reuses one variable down the factors: *energy is the spatial
// energy for factor 0 and the previous factor's mean(TW) (*ge_out of its
// launch) after that.  A previous factor that needs a restart (*prev_flag)
// leaves this one to the host, which alone knows the redrawn mean.
// scal: max(Kb, Kw) doubles of scratch
__global__ __launch_bounds__(256) void k_sf_renorm(double *__restrict__ FB, double *__restrict__ FW,
                                                   double *__restrict__ TW, int F, int Kb, int Kw, int T,
                                                   const double *__restrict__ energy, int last,
                                                   double *__restrict__ scal, int *__restrict__ flag,
                                                   const int *__restrict__ prev_flag,
                                                   double *__restrict__ ge_out) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x;
  if (prev_flag && *prev_flag) return;
  const double e = *energy;
  for (int k = tid; k < Kb; k += 256) {
    double m = -INFINITY;
    for (int f = 0; f < F; ++f) {
      const double v = FB[(size_t)f * Kb + k] * e;
      FB[(size_t)f * Kb + k] = v;
      m = fmax(m, v);
    }
    if (m == 0.0) m = 1.0;
    for (int f = 0; f < F; ++f) FB[(size_t)f * Kb + k] /= m;
    scal[k] = m;
  }
  __syncthreads();
  for (int i = tid; i < Kb * Kw; i += 256) FW[i] *= scal[i / Kw];
  __syncthreads();
  for (int k = tid; k < Kw; k += 256) {   // (scal's column maxima were consumed above)
    double s = 0.0;
    for (int b = 0; b < Kb; ++b) s += FW[(size_t)b * Kw + k];
    double w2 = s / (double)Kb;
    if (w2 == 0.0) w2 = 1.0;
    for (int b = 0; b < Kb; ++b) FW[(size_t)b * Kw + k] /= w2;
    scal[k] = w2;
  }
  __syncthreads();
  const size_t n = (size_t)Kw * T;
  double s = 0.0;
  for (size_t i = tid; i < n; i += 256) {
    const double v = TW[i] * scal[i / T];
    TW[i] = v;
    s += v;
  }
  const double tot = block_sum(s, s_red);
  const int dead = tot < kEps ? 1 : 0;
  const double ge = tot / (double)n;
  if (tid == 0) {
    *flag = dead;
    *ge_out = ge;
  }
  if (dead || last) return;
  for (size_t i = tid; i < n; i += 256) TW[i] /= ge;
}

// ------------------------------------------------------------ wide factors
// A factor with Kb > kSfWideK, FB and FW fixed and FW diagonal (the F0 comb
// dictionary of multiChanSourceF0Filter: FW starts as the identity, and the
// renormalisation below, like the reference's, turns it into another diagonal
// matrix at its first pass, so "identity" cannot be what the arm relies on).
// W = FB.FW is then a column scaling, formed exactly by k_sfw_scale in both
// layouts k_dgemm2 wants as its k-major operand; P = W.TW and [num | den] =
// W^T [rn | rd] run on k_dgemm2, which has no split-K: one fixed summation
// order per output.  The renormalisation is the reference's (:2003-2036) as
// k_sf_renorm states it, spread over the chip: the launches below in stream
// order, each leaving the factor alone after a dead predecessor.

// W[f][k] = FB[f][k] FW[k][k] and WT = W^T, through a 32 x 32 LDS tile
__global__ __launch_bounds__(256) void k_sfw_scale(const double *__restrict__ FB, const double *__restrict__ FW,
                                                   double *__restrict__ W, double *__restrict__ WT, int F,
                                                   int Kb, int ldw, int ldwt) {
  __shared__ double tile[32][33];
  const int k0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int f = f0 + r, k = k0 + tx;
    double v = 0.0;
    if (f < F && k < Kb) {
      v = FB[(size_t)f * Kb + k] * FW[(size_t)k * Kb + k];
      W[(size_t)f * ldw + k] = v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, f = f0 + tx;
    if (k < Kb && f < F) WT[(size_t)k * ldwt + f] = tile[tx][r];
  }
}

// k_sf_ratio writing rnd [F][2 T] = [rn | rd], the B operand of one product
__global__ void k_sfw_ratio(const double *__restrict__ Ps, const double *__restrict__ Po,
                            const double *__restrict__ other, const double *__restrict__ hatW,
                            double *__restrict__ rnd, int T, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double v = fmax(Po ? Ps[i] * Po[i] : Ps[i], kEps), o = other[i];
    const size_t q = i + (i / T) * (size_t)T;
    rnd[q + T] = o * (1.0 / v);
    rnd[q] = hatW[i] / (v * v) * o;
  }
}

// TW[k][t] *= (num / max(den, eps))^omega from cnd [Kb][2 T] = [num | den]
__global__ void k_sfw_update(double *__restrict__ TW, const double *__restrict__ cnd, int T, size_t n,
                             double omega) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t q = i + (i / T) * (size_t)T;
    const double g = cnd[q] / fmax(cnd[q + T], kEps);
    TW[i] *= omega == 1.0 ? g : pow(g, omega);
  }
}

struct SfwRenArgs {
  double *FB, *FW, *TW;
  int F, Kb, T, last;
  const double *energy;
  double *cmax, *m, *w2, *part;   // [G][Kb], [Kb], [Kb], [gridDim of k_sfw_twscale]
  int *flag;
  const int *prev_flag;
  double *ge_out;
};

// block (x, y): the maximum of FB energy over rows [kSfWideRows y, + kSfWideRows)
// of columns 256 x + tid (a maximum does not depend on its order)
__global__ __launch_bounds__(256) void k_sfw_colmax(const SfwRenArgs a) {
  if (a.prev_flag && *a.prev_flag) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.Kb) return;
  const double e = *a.energy;
  const int f1 = min(a.F, ((int)blockIdx.y + 1) * kSfWideRows);
  double m = -INFINITY;
  for (int f = blockIdx.y * kSfWideRows; f < f1; ++f) m = fmax(m, a.FB[(size_t)f * a.Kb + k] * e);
  a.cmax[(size_t)blockIdx.y * a.Kb + k] = m;
}

// column k: m = max of its G partials (0 -> 1); FW[k][k] *= m; the mean of a
// column of a diagonal FW is FW[k][k] / Kb = w2 (0 -> 1); FW[k][k] /= w2
__global__ __launch_bounds__(256) void k_sfw_colfin(const SfwRenArgs a, int G) {
  if (a.prev_flag && *a.prev_flag) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.Kb) return;
  double m = -INFINITY;
  for (int g = 0; g < G; ++g) m = fmax(m, a.cmax[(size_t)g * a.Kb + k]);
  if (m == 0.0) m = 1.0;
  a.m[k] = m;
  const double d = a.FW[(size_t)k * a.Kb + k] * m;
  double w2 = d / (double)a.Kb;
  if (w2 == 0.0) w2 = 1.0;
  a.FW[(size_t)k * a.Kb + k] = d / w2;
  a.w2[k] = w2;
}

// FB[f][k] = FB[f][k] energy / m[k]
__global__ void k_sfw_fbapply(const SfwRenArgs a) {
  if (a.prev_flag && *a.prev_flag) return;
  const double e = *a.energy;
  const size_t n = (size_t)a.F * a.Kb;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    a.FB[i] = a.FB[i] * e / a.m[i % a.Kb];
}

// TW[k][t] *= w2[k]; part[block] = this block's sum of the scaled TW (a
// thread's elements in ascending order, then the tree of block_sum)
__global__ __launch_bounds__(256) void k_sfw_twscale(const SfwRenArgs a) {
  __shared__ double s_red[256];
  if (a.prev_flag && *a.prev_flag) return;
  const size_t n = (size_t)a.Kb * a.T;
  double s = 0.0;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double v = a.TW[i] * a.w2[i / a.T];
    a.TW[i] = v;
    s += v;
  }
  const double tot = block_sum(s, s_red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

// one thread: the partials in index order -> the restart flag and mean(TW)
__global__ void k_sfw_twfin(const SfwRenArgs a, int nb) {
  if (a.prev_flag && *a.prev_flag) return;
  if (blockIdx.x || threadIdx.x) return;
  double tot = 0.0;
  for (int b = 0; b < nb; ++b) tot += a.part[b];
  *a.flag = tot < kEps ? 1 : 0;
  *a.ge_out = tot / (double)((size_t)a.Kb * a.T);
}

// TW /= mean(TW), unless it is dead or the component's last factor
__global__ void k_sfw_twdiv(const SfwRenArgs a) {
  if ((a.prev_flag && *a.prev_flag) || *a.flag) return;
  const double ge = *a.ge_out;
  const size_t n = (size_t)a.Kb * a.T;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    a.TW[i] /= ge;
}

// reweigh_sparsity_constraint (audioModel.py:2981-3014) on one TW [K][T], K > 2,
// in two launches: a frame's median window holds the barycentres of up to 2 L
// neighbouring frames, and in one in-place launch another block could have
// multiplied those columns of TW before they were read.
//
// mu[t] = sum_{k<K-1} k (K-1-k)^2 TW[k,t] / sum_{k<K-1} (K-1-k)^2 max(TW[k,t], eps):
// one thread per frame, the rows in ascending order (loads coalesce over t)
constexpr int kBaryBlock = 64;
__global__ __launch_bounds__(kBaryBlock) void k_sf_bary(const double *__restrict__ TW, int K, int T,
                                                        double *__restrict__ mu) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * kBaryBlock + threadIdx.x;
  if (t >= T) return;
  const double *p = TW + t;
  double num = 0.0, den = 0.0;
#pragma unroll 8
  for (int k = 0; k < K - 1; ++k) {
    const double v = p[(size_t)k * T];
    const double d = (double)(K - 1 - k), w = d * d;
    num += (double)k * w * v;
    den += w * fmax(v, kEps);
  }
  mu[t] = num / den;
}

// TW[k,t] *= m[k] / max_k m[k], m[k] = exp(-0.5 (k - med(mu)[t])^2 / sigma), the
// last row's m replaced by the maximum (no division where the maximum is not
// > 0).  Block (x, y): frames [256 x, 256 x + 256), rows [rows y, rows y + rows);
// every block takes the median of its frames itself (medianFilter's windows,
// median_at; mu staged in LDS over the chunk and its halo when that fits).
// The maximum over k = 0 .. K-1 needs no pass over the rows: subtraction,
// square, division and exp are monotone in |k - med| in floating point too, so
// it is m at the row nearest to med, the larger of its two integer neighbours
constexpr int kSpChunk = 256;

struct SfSpArgs {
  double *TW;
  const double *mu;
  int K, T, L, rows;
  double sigma;
};

__device__ __forceinline__ double sp_mask(double k, double med, double sigma) {
#pragma clang fp contract(off)
  const double d = k - med;
  return exp(-0.5 * (d * d) / sigma);
}

template <bool kStaged>
__global__ __launch_bounds__(kSpChunk) void k_sf_sparsify(const SfSpArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double sm[];  // [kSpChunk + 2 L] if staged
  const int c0 = blockIdx.x * kSpChunk;
  // the samples any window of this chunk can hold: [s_lo, s_hi), s_hi <= T - 1
  const int s_lo = max(c0 - a.L, 0);
  const int s_hi = (int)min((long)c0 + kSpChunk - 1 + a.L, (long)a.T - 1);
  if (kStaged) {
    for (int i = s_lo + (int)threadIdx.x; i < s_hi; i += kSpChunk) sm[i - s_lo] = a.mu[i];
    __syncthreads();
  }
  const double *src = kStaged ? sm - s_lo : a.mu;
  const int t = c0 + threadIdx.x;
  if (t >= a.T) return;
  const double med = median_at(src, a.mu[t], t, a.L, a.T);
  const double last = (double)(a.K - 1);
  double top = med;   // a NaN track: a NaN mask, as np.max gives
  if (med == med) {
    const double kf = fmin(fmax(floor(med), 0.0), last);
    top = fmax(sp_mask(kf, med, a.sigma), sp_mask(fmin(kf + 1.0, last), med, a.sigma));
  }
  const bool norm = top > 0.0;
  const int k0 = blockIdx.y * a.rows, k1 = min(k0 + a.rows, a.K);
  double *p = a.TW + t;
  for (int k = k0; k < k1; ++k) {
    double w = k == a.K - 1 ? top : sp_mask((double)k, med, a.sigma);
    if (norm) w /= top;
    p[(size_t)k * a.T] *= w;
  }
}

// Per-bin Wiener images from the V_j planes (compute_sigma_comp_2d :1327-1372,
// compute_inv_sigma_mix_2d :1374-1394, compute_Wiener_gain_2d :1396-1467):
// source n sums the spatial components j with src_of[j] == n.  X [2][Tp][Fp]
// frame-major; S[(n 2 + c) splane + f sf + t st]
struct SfWArgs {
  const double *V;       // [J][F][T]
  const double2 *mix;    // [R][2][F]
  const double *psd;
  const double2 *X;
  double2 *S;
  int F, T, Fp, Tp, J, nsrc;
  int roff[kMaxJ + 1], src_of[kMaxJ];
  size_t splane, sf, st;
};

__global__ __launch_bounds__(256) void k_sf_wiener(const SfWArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
  if (t >= a.T) return;
  const size_t FT = (size_t)a.F * a.T, i = (size_t)f * a.T + t;
  double c0[kMaxJ], c1[kMaxJ], cr[kMaxJ], ci[kMaxJ];
  for (int j = 0; j < a.J; ++j) {
    double r0 = 0.0, r1 = 0.0, orr = 0.0, oi = 0.0;
    for (int r = a.roff[j]; r < a.roff[j + 1]; ++r) {
      const double2 a0 = a.mix[((size_t)r * 2 + 0) * a.F + f], a1 = a.mix[((size_t)r * 2 + 1) * a.F + f];
      r0 += a0.x * a0.x + a0.y * a0.y;
      r1 += a1.x * a1.x + a1.y * a1.y;
      orr += a0.x * a1.x + a0.y * a1.y;
      oi += a0.y * a1.x - a0.x * a1.y;
    }
    const double v = a.V[(size_t)j * FT + i];
    c0[j] = r0 * v;
    c1[j] = r1 * v;
    cr[j] = orr * v;
    ci[j] = oi * v;
  }
  double d0 = 0.0, d1 = 0.0, orr = 0.0, oi = 0.0;
  for (int n = 0; n < a.nsrc; ++n)
    for (int j = 0; j < a.J; ++j)
      if (a.src_of[j] == n) {
        d0 += c0[j];
        d1 += c1[j];
        orr += cr[j];
        oi += ci[j];
      }
  const double p = a.psd[f];
  d0 += p;
  d1 += p;
  double det = d0 * d1 - (orr * orr + oi * oi);
  const double dg = det + kEps;
  det = (dg > 0.0 ? 1.0 : (dg < 0.0 ? -1.0 : 0.0)) * fmax(fabs(det), kEps);
  const double i0 = d1 / det, i1 = d0 / det, ior = -orr / det, ioi = -oi / det;
  const double2 x0 = a.X[(size_t)t * a.Fp + f], x1 = a.X[((size_t)a.Tp + t) * a.Fp + f];
  for (int n = 0; n < a.nsrc; ++n) {
    double s0 = 0.0, s1 = 0.0, sr = 0.0, si = 0.0;
    for (int j = 0; j < a.J; ++j)
      if (a.src_of[j] == n) {
        s0 += c0[j];
        s1 += c1[j];
        sr += cr[j];
        si += ci[j];
      }
    // so conj(iso)
    const double wr = sr * ior + si * ioi, wi = si * ior - sr * ioi;
    const double g00r = wr + s0 * i0, g00i = wi, g11r = wr + s1 * i1, g11i = -wi;
    const double g01r = s0 * ior + sr * i1, g01i = s0 * ioi + si * i1;
    const double g10r = sr * i0 + s1 * ior, g10i = -si * i0 - s1 * ioi;
    const double2 y0 = make_double2(g00r * x0.x - g00i * x0.y + g01r * x1.x - g01i * x1.y,
                                    g00r * x0.y + g00i * x0.x + g01r * x1.y + g01i * x1.x);
    const double2 y1 = make_double2(g10r * x0.x - g10i * x0.y + g11r * x1.x - g11i * x1.y,
                                    g10r * x0.y + g10i * x0.x + g11r * x1.y + g11i * x1.x);
    a.S[(size_t)(2 * n) * a.splane + f * a.sf + t * a.st] = y0;
    a.S[(size_t)(2 * n + 1) * a.splane + f * a.sf + t * a.st] = y1;
  }
}

// ------------------------------------------------------------------ host side
void sf_release(fasst_ctx *c) {
  if (!c || !c->sf) return;
  DeviceGuard g(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c->sf;
  c->sf = nullptr;
}

static int need_sf(fasst_ctx *c, int j, int i = 0) {
  if (!c || !c->sf) {
    set_error("no two-factor model configured (fasst_sf_configure)");
    return FASST_ERR_SHAPE;
  }
  if (j < 0 || j >= c->sf->J || i < 0 || i >= c->sf->nfac[j]) {
    set_error("component %d factor %d out of range", j, i);
    return FASST_ERR_SHAPE;
  }
  return FASST_OK;
}

// C = A.B on the MFMA GEMM (row-major, dense)
static int sf_mm(fasst_ctx *c, const double *A, const double *B, double *C, int M, int N, int K) {
  const double *Bs[1] = {B};
  double *Cs[1] = {C};
  sf_count(c, KSF_GEMM);
  return gemm<false, false, 1>(c->stream, A, K, Bs, N, Cs, N, M, N, K, c->sf->work.p);
}

// W = FB.FW (unless only TW moved: w == false), P = W.TW of factor (j, i)
static int sf_power(fasst_ctx *c, int j, int i, bool w = true) {
  SfFactor &x = c->sf->fac[j][i];
  int st;
  if (x.wide) {   // the column scaling, then P = WT^T TW on k_dgemm2
    if (w) {
      sf_count(c, KSFW_SCALE);
      k_sfw_scale<<<dim3((x.Kb + 31) / 32, (c->F + 31) / 32), 256, 0, c->stream>>>(x.fb, x.fw, x.W.p, x.WT.p, c->F,
                                                                                 x.Kb, x.ldw, x.ldwt);
      FASST_LAUNCH_CHECK();
    }
    sf_count(c, KSFW_DGEMM2);
    return dgemm2(c->stream, c->F, c->T, x.Kb, x.WT.p, x.ldwt, x.tw, c->T, x.P.p, c->T);
  }
  if (w && (st = sf_mm(c, x.fb, x.fw, x.W.p, c->F, x.Kw, x.Kb))) return st;
  return sf_mm(c, x.W.p, x.tw, x.P.p, c->F, c->T, x.Kw);
}

static int sf_source_power(fasst_ctx *c, int j) {
  fasst_sf_model *m = c->sf;
  const size_t FT = (size_t)c->F * c->T;
  sf_count(c, KSF_PROD);
  k_sf_prod<<<egrid(FT, kSfGridCap), 256, 0, c->stream>>>(m->fac[j][0].P.p, m->nfac[j] > 1 ? m->fac[j][1].P.p : nullptr,
                                                m->V.p + (size_t)j * FT, FT);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

static int sf_all_powers(fasst_ctx *c) {
  int st;
  for (int j = 0; j < c->sf->J; ++j) {
    for (int i = 0; i < c->sf->nfac[j]; ++i)
      if ((st = sf_power(c, j, i))) return st;
    if ((st = sf_source_power(c, j))) return st;
  }
  return FASST_OK;
}

static int sf_ratio(fasst_ctx *c, int j, int i) {
  fasst_sf_model *m = c->sf;
  const size_t FT = (size_t)c->F * c->T;
  sf_count(c, KSF_RATIO);
  k_sf_ratio<<<egrid(FT, kSfGridCap), 256, 0, c->stream>>>(m->fac[j][i].P.p, m->nfac[j] > 1 ? m->fac[j][1 - i].P.p : nullptr,
                                                 m->other.p, m->hatW.p + (size_t)j * FT, m->rn.p, m->rd.p, FT);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

static int sf_apply(fasst_ctx *c, double *P, int rows, int cols, const double *num, const double *den,
                    int tr, double omega) {
  sf_count(c, KSF_UPDATE);
  k_sf_update<<<egrid((size_t)rows * cols, kSfGridCap), 256, 0, c->stream>>>(P, rows, cols, num, den, tr, omega);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// update_spectral_components of source j (audioModel.py:1509-1727, lambdaCorr
// == 0, TB empty): factors in order, FB then FW then TW
static int sf_spectral_update(fasst_ctx *c, int j, double omega) {
  fasst_sf_model *m = c->sf;
  const int F = c->F, T = c->T;
  const size_t FT = (size_t)F * T;
  int st;
  // a matrix shared with another source may have moved since the iteration's
  // powers were formed; without one they stand
  if (m->shared[j])
    for (int i = 0; i < m->nfac[j]; ++i)
      if ((st = sf_power(c, j, i))) return st;
  for (int i = 0; i < m->nfac[j]; ++i) {
    SfFactor &x = m->fac[j][i];
    const int Kb = x.Kb, Kw = x.Kw;
    // the power is refreshed after a step only when a later step of this
    // source reads it (the next iteration and the separation form their own)
    const bool more = i < m->nfac[j] - 1;
    // `other`, once per factor, from the powers as they stand
    const double *Po = m->nfac[j] > 1 ? m->fac[j][1 - i].P.p : x.P.p;
    sf_count(c, KSF_OTHER);
    k_sf_other<<<egrid(FT, kSfGridCap), 256, 0, c->stream>>>(Po, m->other.p, FT);
    FASST_LAUNCH_CHECK();
    const double *RB[2] = {m->rn.p, m->rd.p};
    if (x.fb_free) {
      if ((st = sf_ratio(c, j, i))) return st;
      // (FW.TW) [Kb][T]; num^T [Kb][F] = (FW.TW) rn^T, den^T likewise
      if ((st = sf_mm(c, x.fw, x.tw, m->fwh.p, Kb, T, Kw))) return st;
      double *Cs[2] = {m->cn.p, m->cd.p};
      sf_count(c, KSF_GEMM);
      if ((st = gemm<false, true, 2>(c->stream, m->fwh.p, T, RB, T, Cs, F, Kb, F, T, m->work.p))) return st;
      if ((st = sf_apply(c, x.fb, F, Kb, m->cn.p, m->cd.p, 1, omega))) return st;
      if ((more || x.fw_free || x.tw_free) && (st = sf_power(c, j, i))) return st;
    }
    if (x.fw_free) {
      if ((st = sf_ratio(c, j, i))) return st;
      // X^T [Kw][F] = TW r^T, then num^T [Kw][Kb] = X^T FB
      double *Xs[2] = {m->xn.p, m->xd.p};
      sf_count(c, KSF_GEMM);
      if ((st = gemm<false, true, 2>(c->stream, x.tw, T, RB, T, Xs, F, Kw, F, T, m->work.p))) return st;
      if ((st = sf_mm(c, m->xn.p, x.fb, m->cn.p, Kw, Kb, F))) return st;
      if ((st = sf_mm(c, m->xd.p, x.fb, m->cd.p, Kw, Kb, F))) return st;
      if ((st = sf_apply(c, x.fw, Kb, Kw, m->cn.p, m->cd.p, 1, omega))) return st;
      if ((more || x.tw_free) && (st = sf_power(c, j, i))) return st;
    }
    if (x.tw_free && x.wide) {
      // [num | den] [Kb][2 T] = W^T [rn | rd]: one product, W read once
      sf_count(c, KSF_RATIO);
      k_sfw_ratio<<<egrid(FT, kSfGridCap), 256, 0, c->stream>>>(x.P.p, m->nfac[j] > 1 ? m->fac[j][1 - i].P.p : nullptr,
                                                      m->other.p, m->hatW.p + (size_t)j * FT, m->rnd.p, T, FT);
      FASST_LAUNCH_CHECK();
      sf_count(c, KSFW_DGEMM2);
      if ((st = dgemm2(c->stream, Kb, 2 * T, F, x.W.p, x.ldw, m->rnd.p, 2 * T, m->cnd.p, 2 * T))) return st;
      sf_count(c, KSFW_UPDATE);
      k_sfw_update<<<egrid((size_t)Kb * T, kSfGridCap), 256, 0, c->stream>>>(x.tw, m->cnd.p, T, (size_t)Kb * T, omega);
      FASST_LAUNCH_CHECK();
      if (more && (st = sf_power(c, j, i, false))) return st;
    } else if (x.tw_free) {
      if ((st = sf_ratio(c, j, i))) return st;
      // num [Kw][T] = W^T rn, den = W^T rd
      double *Cs[2] = {m->cn.p, m->cd.p};
      sf_count(c, KSF_GEMM);
      if ((st = gemm<true, false, 2>(c->stream, x.W.p, Kw, RB, T, Cs, T, Kw, T, F, m->work.p))) return st;
      if ((st = sf_apply(c, x.tw, Kw, T, m->cn.p, m->cd.p, 0, omega))) return st;
      if (more && (st = sf_power(c, j, i, false))) return st;
    }
  }
  return FASST_OK;
}

static int sf_renormalize(fasst_ctx *c) {
  fasst_sf_model *m = c->sf;
  sf_count(c, KSF_ENERGY);
  k_sf_energy<<<m->J, 256, 0, c->stream>>>(m->mix.p, c->F, m->droff.p, m->dconv.p, m->energy.p);
  FASST_LAUNCH_CHECK();
  for (int j = 0; j < m->J; ++j)
    for (int i = 0; i < m->nfac[j]; ++i) {
      SfFactor &x = m->fac[j][i];
      int *flag = m->flags.p + 1 + 2 * j + i;
      if (x.wide) {
        SfwRenArgs a;
        a.FB = x.fb;
        a.FW = x.fw;
        a.TW = x.tw;
        a.F = c->F;
        a.Kb = x.Kb;
        a.T = c->T;
        a.last = i == m->nfac[j] - 1;
        a.energy = m->energy.p + (i ? kMaxJ + j : j);
        a.cmax = m->wcmax.p;
        a.m = m->wm.p;
        a.w2 = m->ww2.p;
        a.part = m->wpart.p;
        a.flag = flag;
        a.prev_flag = i ? flag - 1 : nullptr;
        a.ge_out = m->energy.p + kMaxJ + j;
        const int G = (c->F + kSfWideRows - 1) / kSfWideRows, kg = (x.Kb + 255) / 256;
        const size_t n = (size_t)x.Kb * c->T;
        const int nb = (int)std::min<size_t>((n + 255) / 256, kSfWidePart);
        k_sfw_colmax<<<dim3(kg, G), 256, 0, c->stream>>>(a);
        FASST_LAUNCH_CHECK();
        k_sfw_colfin<<<kg, 256, 0, c->stream>>>(a, G);
        FASST_LAUNCH_CHECK();
        k_sfw_fbapply<<<egrid((size_t)c->F * x.Kb, kSfGridCap), 256, 0, c->stream>>>(a);
        FASST_LAUNCH_CHECK();
        k_sfw_twscale<<<nb, 256, 0, c->stream>>>(a);
        FASST_LAUNCH_CHECK();
        k_sfw_twfin<<<1, 64, 0, c->stream>>>(a, nb);
        FASST_LAUNCH_CHECK();
        if (c->prof) c->prof_cnt[KSFW_RENORM] += 5;
        if (!a.last) {
          sf_count(c, KSFW_RENORM);
          k_sfw_twdiv<<<egrid(n, kSfGridCap), 256, 0, c->stream>>>(a);
          FASST_LAUNCH_CHECK();
        }
        continue;
      }
      sf_count(c, KSF_RENORM);
      k_sf_renorm<<<1, 256, 0, c->stream>>>(x.fb, x.fw, x.tw, c->F, x.Kb, x.Kw, c->T,
                                            m->energy.p + (i ? kMaxJ + j : j), i == m->nfac[j] - 1,
                                            m->scal.p, flag, i ? flag - 1 : nullptr, m->energy.p + kMaxJ + j);
      FASST_LAUNCH_CHECK();
    }
  return FASST_OK;
}

static int sf_iteration(fasst_ctx *c, const double *dpsd, double *dll, double omega, int nconv) {
  fasst_sf_model *m = c->sf;
  const size_t FT = (size_t)c->F * c->T;
  int st;
  if ((st = sf_all_powers(c))) return st;
  int vmap[kStepMaxR];
  for (int j = 0; j < m->J; ++j)
    for (int r = m->roff[j]; r < m->roff[j + 1]; ++r) vmap[r] = j;
  if ((st = suff_stat_device(c, c->stream, m->R, m->V.p, vmap, m->mix.p, dpsd, m->rxx.p, m->rxs.p, m->rss.p,
                             m->ws.p, m->llb.p, dll)))
    return st;
  if ((st = mix_solve_device(c->stream, c->F, m->R, m->rss.p, m->rxs.p, m->mix.p, m->kind.p, nconv,
                             m->flags.p)))
    return st;
  for (int j = 0; j < m->J; ++j) {
    sf_count(c, KSF_HATW);
    k_sf_hatw<<<egrid(FT, kSfGridCap), 256, 0, c->stream>>>(m->ws.p, m->hatW.p + (size_t)j * FT, m->roff[j], m->rank[j],
                                                  FT);
    FASST_LAUNCH_CHECK();
  }
  for (int j = 0; j < m->J; ++j)
    if ((st = sf_spectral_update(c, j, omega))) return st;
  return sf_renormalize(c);
}

static int sf_flags_mask(fasst_ctx *c, int *mask) {
  fasst_sf_model *m = c->sf;
  int h[1 + 2 * kMaxJ];
  FASST_TRY(m->flags.get(h, 1 + 2 * kMaxJ, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  if (h[0]) {
    set_error("Singular Matrix");
    return FASST_ERR_SINGULAR;
  }
  *mask = 0;
  for (int j = 0; j < m->J; ++j)
    for (int i = 0; i < m->nfac[j]; ++i)
      if (h[1 + 2 * j + i]) *mask = (int)((unsigned)*mask | (1u << (2 * j + i)));
  return FASST_OK;
}

// the two reweighting kernels carry device time as well as a launch count
// while profiling is on: an event pair and a host wait per launch
static int sf_tick(fasst_ctx *c, int id) {
  if (c->prof) FASST_HIP(hipEventRecord(c->ev0[id][0], c->stream));
  return FASST_OK;
}
static int sf_tock(fasst_ctx *c, int id) {
  if (!c->prof) return FASST_OK;
  float ms = 0.f;
  int st = elapsed_ms(c->ev0[id][0], c->ev1[id][0], c->stream, &ms);
  if (st) return st;
  c->prof_ms[id] += ms;
  c->prof_cnt[id] += 1;
  return FASST_OK;
}

// reweigh_sparsity_constraint (audioModel.py:2987-3014): the components in
// order, each on the TW its factor 0 uses, so a TW shared by two components is
// multiplied twice, as the reference's in-place loop does
static int sf_reweigh(fasst_ctx *c, double sigma) {
  fasst_sf_model *m = c->sf;
  const int T = c->T;
  int st;
  for (int j = 0; j < m->J; ++j) {
    const int K = m->fac[j][0].Kw;
    if (!m->sparsity[j] || K <= 2) continue;
    if ((st = sf_tick(c, KSF_BARY))) return st;
    k_sf_bary<<<(T + kBaryBlock - 1) / kBaryBlock, kBaryBlock, 0, c->stream>>>(m->fac[j][0].tw, K, T, m->mu.p);
    FASST_LAUNCH_CHECK();
    if ((st = sf_tock(c, KSF_BARY))) return st;
    SfSpArgs a;
    a.TW = m->fac[j][0].tw;
    a.mu = m->mu.p;
    a.K = K;
    a.T = T;
    a.L = std::min(m->sparsity[j], T);   // the same windows, and t + L stays an int
    a.sigma = sigma;
    // row slabs: about 1024 blocks in all, no slab under 8 rows
    const int nchunks = (T + kSpChunk - 1) / kSpChunk;
    const int want = std::max(1, 1024 / nchunks);
    a.rows = std::max(8, (K + want - 1) / want);
    const dim3 grid(nchunks, (K + a.rows - 1) / a.rows);
    if ((st = sf_tick(c, KSF_SPARSIFY))) return st;
    if ((long)kSpChunk + 2L * a.L <= kMedLdsSpan)
      k_sf_sparsify<true><<<grid, kSpChunk, (kSpChunk + 2 * (size_t)a.L) * sizeof(double), c->stream>>>(a);
    else
      k_sf_sparsify<false><<<grid, kSpChunk, 0, c->stream>>>(a);
    FASST_LAUNCH_CHECK();
    if ((st = sf_tock(c, KSF_SPARSIFY))) return st;
  }
  return FASST_OK;
}

// the mask's width: the maximum over the rows is taken where it must lie for
// sigma > 0 (k_sf_sparsify)
static int sf_check_sigma(const double *sigma, int n) {
  for (int i = 0; i < n; ++i)
    if (!(sigma[i] > 0.0)) {
      set_error("reweigh_sparsity_constraint: sigma[%d] = %g is not > 0", i, sigma[i]);
      return FASST_ERR_SHAPE;
    }
  return FASST_OK;
}

static int sf_launch_wiener(fasst_ctx *c, const double *dpsd, int nsrc, const int *src_of, double2 *dS,
                            size_t splane, size_t sf, size_t st_) {
  fasst_sf_model *m = c->sf;
  SfWArgs a;
  a.V = m->V.p;
  a.mix = m->mix.p;
  a.psd = dpsd;
  a.X = c->X.p;
  a.S = dS;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.Tp = c->Tp;
  a.J = m->J;
  a.nsrc = nsrc;
  for (int j = 0; j <= kMaxJ; ++j) a.roff[j] = j <= m->J ? m->roff[j] : m->roff[m->J];
  for (int j = 0; j < kMaxJ; ++j) a.src_of[j] = j < m->J ? src_of[j] : -1;
  a.splane = splane;
  a.sf = sf;
  a.st = st_;
  sf_count(c, KSF_WIENER);
  k_sf_wiener<<<dim3((c->T + 255) / 256, c->F), 256, 0, c->stream>>>(a);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

static int sf_check_sources(fasst_ctx *c, int nsrc, const int *src_of) {
  if (nsrc < 1 || nsrc > kMaxJ || !src_of) {
    set_error("separation sources: %d outside 1..%d", nsrc, kMaxJ);
    return FASST_ERR_SHAPE;
  }
  for (int j = 0; j < c->sf->J; ++j)
    if (src_of[j] < -1 || src_of[j] >= nsrc) {
      set_error("separation sources: component %d in source %d of %d", j, src_of[j], nsrc);
      return FASST_ERR_SHAPE;
    }
  return FASST_OK;
}

// The image producer of the two-factor model's separation calls: the Wiener
// images of the nsrc sources in p.S, queued on c->stream; frame-major [Tp][Fp]
// planes (zero in the padding) for a device sink, else the caller's dense
// [F][T] order.  The caller keeps p until the stream has drained.
struct SfPlanes {
  DBuf<double> dpsd;
  DBuf<double2> S;
};

static int sf_planes(fasst_ctx *c, const double *psd, int nsrc, const int *src_of, bool frame_major,
                     SfPlanes &p) {
  const size_t splane = frame_major ? (size_t)c->Tp * c->Fp : (size_t)c->F * c->T;
  int st;
  if ((st = frame_major ? p.S.alloc(nsrc * 2 * splane) : p.S.alloc_uninit(nsrc * 2 * splane)) ||
      (st = p.dpsd.upload(psd, c->F, c->stream)) || (st = sf_all_powers(c)))
    return st;
  return frame_major ? sf_launch_wiener(c, p.dpsd.p, nsrc, src_of, p.S.p, splane, 1, (size_t)c->Fp)
                     : sf_launch_wiener(c, p.dpsd.p, nsrc, src_of, p.S.p, splane, (size_t)c->T, 1);
}

}  // namespace fasst

using namespace fasst;

extern "C" {

int fasst_sf_configure(fasst_ctx *c, int J, const int *rank, const int *mix_conv, const int *nfac,
                       const int *Kb, const int *Kw, const int *priors, const int *alias) {
  if (!c || !rank || !mix_conv || !nfac || !Kb || !Kw || !priors || !alias) return FASST_ERR_SHAPE;
  if (J < 1 || J > kMaxJ) {
    set_error("J=%d outside the HIP path (1..%d sources)", J, kMaxJ);
    return FASST_ERR_UNSUPPORTED;
  }
  int R = 0;
  for (int j = 0; j < J; ++j) {
    if (rank[j] < 1 || nfac[j] < 1 || nfac[j] > kSfMaxFac) {
      set_error("component %d: rank %d, %d factors (1..%d)", j, rank[j], nfac[j], kSfMaxFac);
      return FASST_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < nfac[j]; ++i)
      if (Kb[2 * j + i] < 1 || Kw[2 * j + i] < 1) {
        set_error("component %d factor %d: Kb %d, Kw %d", j, i, Kb[2 * j + i], Kw[2 * j + i]);
        return FASST_ERR_SHAPE;
      }
    R += rank[j];
  }
  if (R > kStepMaxR) {
    set_error("total spatial rank %d above the explicit-V E-step's %d", R, kStepMaxR);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(c->device);
  sf_release(c);
  fasst_sf_model *m = new fasst_sf_model();
  c->sf = m;
  m->J = J;
  m->R = R;
  const int F = c->F, T = c->T;
  const size_t FT = (size_t)F * T;
  size_t ncd = 1, nx = 1, nfwh = 1, nwork = 1, nscal = 1, nwide = 0;
  int kind[kStepMaxR];
  for (int j = 0; j < J; ++j) {
    m->rank[j] = rank[j];
    m->roff[j + 1] = m->roff[j] + rank[j];
    m->conv[j] = mix_conv[j] ? 1 : 0;
    m->nfac[j] = nfac[j];
    for (int r = m->roff[j]; r < m->roff[j + 1]; ++r) kind[r] = 0;
  }
  int st = FASST_OK;
  for (int j = 0; j < J && !st; ++j)
    for (int i = 0; i < nfac[j] && !st; ++i) {
      SfFactor &x = m->fac[j][i];
      const int kb = Kb[2 * j + i], kw = Kw[2 * j + i];
      x.Kb = kb;
      x.Kw = kw;
      x.fb_free = priors[(2 * j + i) * 3 + 0];
      x.fw_free = priors[(2 * j + i) * 3 + 1];
      x.tw_free = priors[(2 * j + i) * 3 + 2];
      // a matrix shared with an earlier factor (one NumPy array in several
      // factor dicts, updated in place by the reference) shares its buffer
      const int *al = alias + (2 * j + i) * 3;
      const SfFactor *o[3];
      for (int q = 0; q < 3; ++q) {
        o[q] = nullptr;
        if (al[q] < 0) continue;
        const int oj = al[q] / 2, oi = al[q] % 2;
        if (al[q] >= 2 * j + i || oj >= J || oi >= nfac[oj]) {
          set_error("component %d factor %d: shared matrix index %d", j, i, al[q]);
          st = FASST_ERR_SHAPE;
          break;
        }
        o[q] = &m->fac[oj][oi];
        m->shared[j] = m->shared[oj] = 1;
      }
      if (st) break;
      if ((o[0] && (o[0]->Kb != kb)) || (o[1] && (o[1]->Kb != kb || o[1]->Kw != kw)) ||
          (o[2] && o[2]->Kw != kw)) {
        set_error("component %d factor %d: shared matrices of different shapes", j, i);
        st = FASST_ERR_SHAPE;
        break;
      }
      // a wide candidate: whether it is wide is known once its FW is uploaded
      x.cand = kb > kSfWideK && kw == kb && !x.fb_free && !x.fw_free;
      x.ldw = kw + (x.cand ? kw & 1 : 0);
      x.ldwt = F + (F & 1);
      if ((!o[0] && (st = x.FB.alloc((size_t)F * kb))) || (!o[1] && (st = x.FW.alloc((size_t)kb * kw))) ||
          (!o[2] && (st = x.TW.alloc((size_t)kw * T))) || (st = x.W.alloc((size_t)F * x.ldw)) ||
          (x.cand && (st = x.WT.alloc((size_t)kb * x.ldwt))) || (st = x.P.alloc(FT)))
        break;
      if (x.cand) nwide = std::max(nwide, (size_t)kb);
      x.fb = o[0] ? o[0]->fb : x.FB.p;
      x.fw = o[1] ? o[1]->fw : x.FW.p;
      x.tw = o[2] ? o[2]->tw : x.TW.p;
      ncd = std::max({ncd, (size_t)kb * F, (size_t)kw * T, (size_t)kw * kb});
      nx = std::max(nx, (size_t)kw * F);
      nfwh = std::max(nfwh, (size_t)kb * T);
      nscal = std::max({nscal, (size_t)kb, (size_t)kw});
      nwork = std::max({nwork, gemm_workspace(F, kw, kb, 1), gemm_workspace(F, T, kw, 1),
                        gemm_workspace(kb, T, kw, 1), gemm_workspace(kb, F, T, 2),
                        gemm_workspace(kw, F, T, 2), gemm_workspace(kw, kb, F, 1),
                        gemm_workspace(kw, T, F, 2)});
    }
  if (!st) {
    (st = m->V.alloc((size_t)J * FT)) || (st = m->ws.alloc((size_t)R * FT)) ||
        (st = m->hatW.alloc((size_t)J * FT)) || (st = m->other.alloc(FT)) || (st = m->rn.alloc(FT)) ||
        (st = m->rd.alloc(FT)) || (st = m->mix.alloc((size_t)R * 2 * F)) ||
        (st = m->rss.alloc((size_t)F * R * R)) || (st = m->rxs.alloc((size_t)F * 2 * R)) ||
        (st = m->rxx.alloc((size_t)3 * F)) || (st = m->llb.alloc(F)) || (st = m->energy.alloc(2 * kMaxJ)) || (st = m->droff.alloc(kMaxJ + 1)) ||
        (st = m->dconv.alloc(kMaxJ)) ||
        (st = m->scal.alloc(nscal)) || (st = m->kind.alloc(kStepMaxR)) ||
        (st = m->flags.alloc(1 + 2 * kMaxJ)) || (st = m->cn.alloc(ncd)) || (st = m->cd.alloc(ncd)) ||
        (st = m->xn.alloc(nx)) || (st = m->xd.alloc(nx)) || (st = m->fwh.alloc(nfwh)) ||
        (st = m->work.alloc(nwork));
  }
  if (!st && nwide) {
    (st = m->rnd.alloc(2 * FT)) || (st = m->cnd.alloc(nwide * 2 * T)) ||
        (st = m->wcmax.alloc((size_t)((F + kSfWideRows - 1) / kSfWideRows) * nwide)) ||
        (st = m->wm.alloc(nwide)) || (st = m->ww2.alloc(nwide)) || (st = m->wpart.alloc(kSfWidePart));
  }
  if (st) {
    sf_release(c);
    return st;
  }
  if ((st = m->kind.put(kind, R)) || (st = m->droff.put(m->roff, J + 1))) return st;
  return m->dconv.put(m->conv, J);
}

int fasst_sf_set_spatial(fasst_ctx *c, int j, const double *params, int free_) {
  int st = need_sf(c, j);
  if (st) return st;
  if (!params) return FASST_ERR_SHAPE;
  fasst_sf_model *m = c->sf;
  DeviceGuard g(c->device);
  const int F = c->F, r0 = m->roff[j], nr = m->rank[j];
  std::vector<double2> h((size_t)nr * 2 * F);
  const double2 *p = (const double2 *)params;
  if (m->conv[j]) {
    std::copy(p, p + h.size(), h.begin());
  } else {   // the C x r matrix on every bin
    for (int r = 0; r < nr; ++r)
      for (int ch = 0; ch < 2; ++ch)
        for (int f = 0; f < F; ++f) h[((size_t)r * 2 + ch) * F + f] = p[ch * nr + r];
  }
  m->spat_free[j] = free_ ? 1 : 0;
  std::vector<int> kind(nr, free_ ? (m->conv[j] ? 2 : 1) : 0);
  FASST_TRY(m->mix.at((size_t)r0 * 2 * F, h.size()).put(h.data(), h.size()));
  return m->kind.at(r0, nr).put(kind.data(), nr);
}

int fasst_sf_get_spatial(fasst_ctx *c, int j, double *params) {
  int st = need_sf(c, j);
  if (st) return st;
  if (!params) return FASST_ERR_SHAPE;
  fasst_sf_model *m = c->sf;
  DeviceGuard g(c->device);
  const int F = c->F, r0 = m->roff[j], nr = m->rank[j];
  std::vector<double2> h((size_t)nr * 2 * F);
  FASST_HIP(hipStreamSynchronize(c->stream));
  FASST_TRY(m->mix.at((size_t)r0 * 2 * F, h.size()).get(h.data(), h.size()));
  double2 *p = (double2 *)params;
  if (m->conv[j]) {
    std::copy(h.begin(), h.end(), p);
  } else {
    for (int r = 0; r < nr; ++r)
      for (int ch = 0; ch < 2; ++ch) p[ch * nr + r] = h[((size_t)r * 2 + ch) * F];
  }
  return FASST_OK;
}

int fasst_set_factors(fasst_ctx *c, int j, int i, const double *FB, const double *FW, const double *TW) {
  int st = need_sf(c, j, i);
  if (st) return st;
  if (!FB || !FW || !TW) return FASST_ERR_SHAPE;
  SfFactor &x = c->sf->fac[j][i];
  DeviceGuard g(c->device);
  FASST_HIP(hipStreamSynchronize(c->stream));
  // x.fb / x.fw / x.tw may be another factor's buffers, of these shapes (fasst_sf_configure)
  const DSpan<double> fb{x.fb, (size_t)c->F * x.Kb}, fw{x.fw, (size_t)x.Kb * x.Kw},
      tw{x.tw, (size_t)x.Kw * c->T};
  FASST_TRY(fb.put(FB, fb.n));
  FASST_TRY(fw.put(FW, fw.n));
  FASST_TRY(tw.put(TW, tw.n));
  if (x.cand) {   // wide: every entry finite and nothing off the diagonal
    bool diag = true;
    for (int b = 0; b < x.Kb && diag; ++b)
      for (int k = 0; k < x.Kw; ++k) {
        const double v = FW[(size_t)b * x.Kw + k];
        if (!std::isfinite(v) || (b != k && v != 0.0)) {
          diag = false;
          break;
        }
      }
    // (every candidate reading this FW buffer: the upload replaced theirs too)
    fasst_sf_model *m = c->sf;
    for (int oj = 0; oj < m->J; ++oj)
      for (int oi = 0; oi < m->nfac[oj]; ++oi)
        if (m->fac[oj][oi].cand && m->fac[oj][oi].fw == x.fw) m->fac[oj][oi].wide = diag ? 1 : 0;
  }
  return FASST_OK;
}

int fasst_get_factors(fasst_ctx *c, int j, int i, double *FB, double *FW, double *TW) {
  int st = need_sf(c, j, i);
  if (st) return st;
  SfFactor &x = c->sf->fac[j][i];
  DeviceGuard g(c->device);
  FASST_HIP(hipStreamSynchronize(c->stream));
  const DSpan<double> fb{x.fb, (size_t)c->F * x.Kb}, fw{x.fw, (size_t)x.Kb * x.Kw},
      tw{x.tw, (size_t)x.Kw * c->T};
  if (FB) FASST_TRY(fb.get(FB, fb.n));
  if (FW) FASST_TRY(fw.get(FW, fw.n));
  if (TW) FASST_TRY(tw.get(TW, tw.n));
  return FASST_OK;
}

int fasst_sf_renormalize(fasst_ctx *c, int *restart_mask) {
  int st = need_sf(c, 0);
  if (st) return st;
  DeviceGuard g(c->device);
  FASST_TRY(c->sf->flags.zero(1 + 2 * kMaxJ, c->stream));
  if ((st = sf_renormalize(c))) return st;
  int mask = 0;
  if ((st = sf_flags_mask(c, &mask))) return st;
  if (restart_mask) *restart_mask = mask;
  return FASST_OK;
}

// fasst_sf_run (sigma == nullptr) and fasst_sf_run_sparse
static int sf_run(fasst_ctx *c, int n_iter, const double *psd, double omega, const double *sigma,
                  double *logliks, int *restart_mask, int *iters_done) {
  int st = need_sf(c, 0);
  if (st) return st;
  if (n_iter < 0 || (n_iter > 0 && (!psd || !logliks))) return FASST_ERR_SHAPE;
  if (!c->cx_ready) {
    set_error("fasst_sf_run: no observation resident (upload Cx first)");
    return FASST_ERR_SHAPE;
  }
  if (sigma && (st = sf_check_sigma(sigma, n_iter))) return st;
  fasst_sf_model *m = c->sf;
  DeviceGuard g(c->device);
  if (iters_done) *iters_done = 0;
  if (restart_mask) *restart_mask = 0;
  if (n_iter == 0) return FASST_OK;
  if (m->psd_cap < n_iter) {
    FASST_HIP(hipStreamSynchronize(c->stream));
    if ((st = m->psd.alloc((size_t)n_iter * c->F)) || (st = m->ll.alloc(n_iter))) return st;
    m->psd_cap = n_iter;
  }
  FASST_TRY(m->psd.put(psd, (size_t)n_iter * c->F, c->stream));
  FASST_TRY(m->flags.zero(1 + 2 * kMaxJ, c->stream));
  int nconv = 0;
  for (int j = 0; j < m->J; ++j)
    if (m->conv[j] && m->spat_free[j]) nconv += m->rank[j];
  if (nconv && nconv != m->R) {
    set_error("update_mix_matrix: a free 'conv' component next to other components");
    return FASST_ERR_SHAPE;
  }
  int done = 0, mask = 0;
  for (int it = 0; it < n_iter; ++it) {
    if ((st = sf_iteration(c, m->psd.p + (size_t)it * c->F, m->ll.p + it, omega, nconv))) return st;
    if ((st = sf_flags_mask(c, &mask))) return st;
    done = it + 1;
    if (mask) break;
    // (a dead TW is redrawn inside the reference's GEM_iteration, before its
    // reweigh: that iteration's reweigh is the caller's, after the redraw)
    if (sigma && (st = sf_reweigh(c, sigma[it]))) return st;
  }
  if (iters_done) *iters_done = done;
  FASST_TRY(m->ll.get(logliks, done));
  if (mask) {
    if (restart_mask) *restart_mask = mask;
    return FASST_TW_RESTART;
  }
  return FASST_OK;
}

int fasst_sf_run(fasst_ctx *c, int n_iter, const double *psd, double omega, double *logliks,
                 int *restart_mask, int *iters_done) {
  return sf_run(c, n_iter, psd, omega, nullptr, logliks, restart_mask, iters_done);
}

int fasst_sf_run_sparse(fasst_ctx *c, int n_iter, const double *psd, double omega, const double *sigma,
                        double *logliks, int *restart_mask, int *iters_done) {
  if (n_iter > 0 && !sigma) return FASST_ERR_SHAPE;
  return sf_run(c, n_iter, psd, omega, n_iter > 0 ? sigma : nullptr, logliks, restart_mask, iters_done);
}

int fasst_sf_set_sparsity(fasst_ctx *c, const int *length) {
  int st = need_sf(c, 0);
  if (st) return st;
  if (!length) return FASST_ERR_SHAPE;
  fasst_sf_model *m = c->sf;
  bool any = false;
  for (int j = 0; j < m->J; ++j) {
    if (length[j] < 0) {
      set_error("fasst_sf_set_sparsity: component %d has length %d < 0", j, length[j]);
      return FASST_ERR_SHAPE;
    }
    any |= length[j] > 0;
  }
  DeviceGuard g(c->device);
  if (any && !m->mu.p) {
    FASST_HIP(hipStreamSynchronize(c->stream));
    if ((st = m->mu.alloc(c->T))) return st;
  }
  for (int j = 0; j < m->J; ++j) m->sparsity[j] = length[j];
  return FASST_OK;
}

int fasst_sf_reweigh(fasst_ctx *c, double sigma) {
  int st = need_sf(c, 0);
  if (st) return st;
  if ((st = sf_check_sigma(&sigma, 1))) return st;
  DeviceGuard g(c->device);
  return sf_reweigh(c, sigma);
}

int fasst_sf_wiener_images(fasst_ctx *c, const double *psd, int nsrc, const int *src_of, double *S) {
  int st = need_sf(c, 0);
  if (st) return st;
  if (!psd || !S) return FASST_ERR_SHAPE;
  if ((st = sf_check_sources(c, nsrc, src_of)) || (st = need_stft_model(c, "fasst_sf_wiener_images")))
    return st;
  DeviceGuard g(c->device);
  SfPlanes p;
  if ((st = sf_planes(c, psd, nsrc, src_of, false, p))) return st;
  // the kernel wrote the host layout through its strides: no transpose
  FASST_TRY(p.S.get(S, p.S.n, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_sf_separate_waveforms(fasst_ctx *c, const double *psd, int nsrc, const int *src_of,
                                const double *window, const double *analysis_window, int wlen,
                                int nfft, int hop, double *y) {
  int st = need_sf(c, 0);
  if (st) return st;
  if (!psd || !window || !y) return FASST_ERR_SHAPE;
  if ((st = sf_check_sources(c, nsrc, src_of)) ||
      (st = need_stft_model(c, "fasst_sf_separate_waveforms", nfft)))
    return st;
  DeviceGuard g(c->device);
  IstftSink sink;
  SfPlanes p;
  if ((st = sink.init(c->stream, window, analysis_window, wlen, nfft, hop, c->T)) ||
      (st = sf_planes(c, psd, nsrc, src_of, true, p)))
    return st;
  return images_to_waveforms(sink, p.S.p, (size_t)c->Tp * c->Fp, c->Fp, 2 * nsrc, y);
}

// fasst_sf_separate_waveforms for a model on a CQT / MinQT (include/fasst_cqt.h):
// the 2 nsrc images stay in HBM and go through one batched inverse chain
int fasst_sf_separate_waveforms_cqt(fasst_ctx *c, cqt_ctx *q, const double *psd, int nsrc,
                                    const int *src_of, long L, double *y) {
  int st = need_sf(c, 0);
  if (st) return st;
  if (!q || !psd || !y) return FASST_ERR_SHAPE;
  if ((st = sf_check_sources(c, nsrc, src_of)) ||
      (st = cqt_match_model(q, L, c->device, c->F, c->T, "fasst_sf_separate_waveforms_cqt")) ||
      (st = need_stft_model(c, "fasst_sf_separate_waveforms_cqt")))
    return st;
  DeviceGuard g(c->device);
  SfPlanes p;
  if ((st = sf_planes(c, psd, nsrc, src_of, true, p))) return st;
  CqtImages im;
  im.S = p.S.p;
  im.plane = (size_t)c->Tp * c->Fp;
  im.ld = c->Fp;
  return cqt_inverse_batch(q, c->stream, im, 2 * nsrc, L, y);
}

}  // extern "C"
