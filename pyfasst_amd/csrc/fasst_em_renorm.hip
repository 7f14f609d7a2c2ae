// The renormalisation phase of the GEM iteration (renormalize_parameters,
// audioModel.py:1980-2040), in its two forms:
//   unfused  k_renorm_stats / _apply / _final, then k_tb_renorm for the
//            components with time blobs (launch_renorm; fasst_renormalize)
//   fused    the stage-1 statistics come from k_fb_update / k_tw_update of the
//            spectral unit; k_renorm_scales / _rows on the side stream beside
//            the TW contraction (launch_renorm_side), k_renorm_tail at the
//            iteration's end (launch_renorm_tail)
// Interface: fasst_em.h.

#include "fasst_em.h"
#include "fasst_device.h"

namespace fasst {

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

int launch_renorm(fasst_ctx *c, int iter) {
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
    if (int st = launch_tb_refresh(c, iter)) return st;   // H = TWs TB (k_tb_h, the spectral unit's)
  }
  prof_end(c, KREN);
  return FASST_OK;
}

// the fused tail's scales and the FB / mixing / FW rescale, after k_fb_update,
// on the side stream beside the TW contraction (launch_tail_side of the
// spectral unit forks and joins it); ev_scales gates k_tw_update
int launch_renorm_side(fasst_ctx *c, hipStream_t side) {
  const RArgs r = renorm_args(c);
  prof_begin(c, KREN, side);
  k_renorm_scales<<<c->J, 1024, 0, side>>>(r);
  FASST_LAUNCH_CHECK();
  FASST_HIP(hipEventRecord(c->ev_scales, c->aux));
  k_renorm_rows<<<dim3(c->nft, c->J), 256, 0, side>>>(r);
  FASST_LAUNCH_CHECK();
  prof_end(c, KREN, side);
  return FASST_OK;
}

// the fused tail's last launch (k_renorm_tail: the loglik and, with prep, the
// next iteration's TW row sums), after the side stream's ev_rows
int launch_renorm_tail(fasst_ctx *c, double *ll_dev, int iter, bool prep) {
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

}  // namespace fasst
