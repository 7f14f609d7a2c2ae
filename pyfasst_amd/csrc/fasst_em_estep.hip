// The E-step of the GEM iteration (compute_suff_stat, audioModel.py:580-764):
// the operand images, the many-source k_egen_* kernels and k_loglik with
// their launches, and the phase's entry points.  The single-pass k_estep_mx
// (J <= 8) is in fasst_em_estep_mx.h and its instantiations in one unit per
// source count, fasst_em_estep_j1.hip .. _j8.hip, reached through
// estep_mx_j<J> (the switches on J below); this unit names none of them.
//
// E-step restructuring (exact algebra, verified to 1e-15 against the
// reference): with S = Sigma_x^-1, N = S Cx S - S and P = Cx S (2x2 per
// (f,t)), the reference's R x R pair loop (:698-731) is
//   hat_Rss[f][r1,r2] = a_r1^H (sum_t V_j1 V_j2 N) a_r2 / T + d_r1r2 mean_t V_r1
//   hat_Rxs[f][c,r]   = sum_c' (sum_t V_j P)[c,c'] A_r,c' / T
//   hat_Ws[r](f,t)    = | V_j^2 a_r^H N a_r + V_j |
// because the mixing a_r is constant over t.  The t-reductions shrink from
// R^2 complex products per (f,t) to J(J+1)/2 x 4 + 9J real FMAs.
#include "fasst_em_estep_mx.h"

namespace fasst {

// ------------------------------------------- E-step operand images (J <= 8)
// k_estep_mx's lane (fl = lane & 15, tq = lane >> 4) of the wave on the
// 16 x 16 tile (bin tile bt, frame tile tt) holds point i at (f = 16 bt + fl,
// t = 16 tt + tq + 4 i).  The images store what each of its load instructions
// needs as one contiguous KB, 16 bytes per lane.
//
// Cx image: record (bt, tt) = 8 pieces of 64 double2 at img + (bt ntt + tt)
// 512; piece 2 i + h, lane l: (cx00, cx11) (h = 0) or (cxr, cxi) (h = 1) of
// the lane's point i, padding included.  The records of one bin tile are
// consecutive in tt.  Built once per observation (cx_image below).
__global__ __launch_bounds__(256) void k_cx_image(const double *__restrict__ cx,
                                                  double2 *__restrict__ img, int Fp, int ntt,
                                                  size_t plane) {
  const int tt = blockIdx.x, bt = blockIdx.y;
  double2 *rec = img + ((size_t)bt * ntt + tt) * 512;
  for (int e = threadIdx.x; e < 512; e += 256) {
    const int piece = e >> 6, lane = e & 63, i = piece >> 1, fl = lane & 15, tq = lane >> 4;
    const double *p = cx + (size_t)(16 * tt + tq + 4 * i) * Fp + 16 * bt + fl;
    rec[e] = piece & 1 ? make_double2(p[2 * plane], p[3 * plane]) : make_double2(p[0], p[plane]);
  }
}

// the TW image from the planes: wherever TW was written without it (an
// upload, the unfused tail, the first iteration of a batch)
__global__ __launch_bounds__(256) void k_tw_image(const double *__restrict__ TW,
                                                  double2 *__restrict__ img, int J, int KP, int Tp) {
  const int tt = blockIdx.x, j = blockIdx.y;
  const double *tw = TW + (size_t)j * KP * Tp + 16 * tt;
  for (int e = threadIdx.x; e < (KP / 8) * 64; e += 256)
    tw_image_store(img, tt, j, J, KP, e, [&](int k, int fl) { return tw[(size_t)k * Tp + fl]; });
}

// ---------------------------------------------------------------- E-step, J > 8
// More than 8 sources (up to kMaxJ): the statistics no longer fit the
// single-pass kernel's registers (J (J + 1) / 2 pair and 8 J cross sums per
// bin), so the E-step runs in two passes over a scratch copy of its point
// quantities.  k_egen_point: one wave per 16 x 16 (bin, frame) tile, V_j on
// 16x16x4 MFMA (the k_estep_mx / k_wiener tile), then per point Sigma_x, its
// guarded inverse, the loglik term, P = Cx S, N = S Cx S - S and rho, with V_j,
// N and P written to frame-major scratch planes.  k_egen_stats: one block per
// (16-bin tile, frame chunk) sums the pair statistics V_j1 V_j2 N_c and the
// cross statistics V_j P_c over its frames (tiles staged in LDS) into the
// k_estep_mx partial layout, so k_mix reads it unchanged.
struct GArgs {
  double *V;     // [J][Tp][Fp]
  double *NP;    // [12][Tp][Fp]: N0..N3, P0..P7
  double *lw;    // [ntt][nft] per-wave loglik partials
  int J;
};

// V_j of the tile: per source, its NKS TW / W operand pairs in chunks of CH,
// every chunk's loads issued one chunk ahead of its MFMAs (two static register
// buffers; the unrolled (source, chunk) sequence fixes which), so a wave waits
// one memory round trip per chunk instead of one per MFMA.  The loads are
// unconditional (a chunk past source J - 1 re-reads its last), so every path
// reaches each wait with the same loads outstanding.
template <int NKS>
__global__ __launch_bounds__(64) void k_egen_point(const EArgs a, const GArgs g) {
  HALT_GUARD(a.halt);
  constexpr int CH = NKS < 8 ? NKS : 8, NCH = NKS / CH, NST = kMaxJ * NCH;
  const int lane = threadIdx.x, fl = lane & 15, tq = lane >> 4;
  const int tt = blockIdx.x, ft = blockIdx.y, t0 = tt * 16, f0 = ft * 16, f = f0 + fl;
  const int J = g.J;
  __shared__ double s_c[kMaxJ][4][16];   // Sigma_x coefficients of the tile's bins
  __shared__ double s_irk[kMaxJ];
  double ta[2][CH], wa[2][CH];
  auto load = [&](int buf, int st) {
    const int j = min(st / NCH, J - 1), s0 = (st % NCH) * CH;
    const double *tw = a.TW + ((size_t)j * a.KP + tq + 4 * s0) * a.Tp + t0 + fl;
    const double *wk = a.Wkf + ((size_t)j * a.KP + tq + 4 * s0) * a.Fp + f;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      ta[buf][u] = tw[(size_t)(4 * u) * a.Tp];
      wa[buf][u] = wk[(size_t)(4 * u) * a.Fp];
    }
  };
  load(0, 0);
  // lane (fl, tq): the coefficients of sources tq, tq + 4, ... of bin fl
  for (int j = tq; j < J; j += 4) {
    double al = 0, be = 0, gr = 0, gi = 0;
    for (int r = a.roff[j]; r < a.roff[j + 1]; ++r) {
      const double2 a0 = a.A[(size_t)(2 * r) * a.Fp + f];
      const double2 a1 = a.A[(size_t)(2 * r + 1) * a.Fp + f];
      al += a0.x * a0.x + a0.y * a0.y;
      be += a1.x * a1.x + a1.y * a1.y;
      gr += a0.x * a1.x + a0.y * a1.y;
      gi += a0.y * a1.x - a0.x * a1.y;
    }
    s_c[j][0][fl] = al;
    s_c[j][1][fl] = be;
    s_c[j][2][fl] = gr;
    s_c[j][3][fl] = gi;
  }
  if (lane < J) s_irk[lane] = 1.0 / (double)(a.roff[lane + 1] - a.roff[lane]);
  d4 v[kMaxJ];
#pragma unroll
  for (int j = 0; j < kMaxJ; ++j) v[j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const int j = st / NCH, cur = st & 1;
    if (j >= J) break;   // (wave-uniform)
    if (st + 1 < NST) load(cur ^ 1, st + 1);
    asm volatile("" ::: "memory");   // (keeps the prefetch here, not sunk past the next break)
#pragma unroll
    for (int u = 0; u < CH; ++u) v[j] = mfma4(ta[cur][u], wa[cur][u], v[j]);
  }
  __syncthreads();
  const size_t plane = (size_t)a.Tp * a.Fp;
  const double psd = a.psd[f];
  double ll = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = t0 + tq + 4 * i;
    const size_t o = (size_t)t * a.Fp + f;
    const double x00 = a.cx00[o], x11 = a.cx11[o], xr = a.cxr[o], xi = a.cxi[o];
    double d0 = psd, d1 = psd, ore = 0.0, oim = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxJ; ++j)
      if (j < J) {
        d0 += s_c[j][0][fl] * v[j][i];
        d1 += s_c[j][1][fl] * v[j][i];
        ore += s_c[j][2][fl] * v[j][i];
        oim += s_c[j][3][fl] * v[j][i];
      }
    // inv_herm_mat_2d (signalTools.py:177-194)
    double det = d0 * d1 - (ore * ore + oim * oim);
    const double dg = det + kEps;
    det = (dg > 0.0 ? 1.0 : (dg < 0.0 ? -1.0 : 0.0)) * fmax(fabs(det), kEps);
    const double rdet = rcp_nr(det);
    const double i0 = d1 * rdet, i1 = d0 * rdet, ior = -ore * rdet, ioi = -oim * rdet;
    if (f < a.F && t < a.T) ll += log(det * M_PI) + (i0 * x00 + i1 * x11 + 2.0 * (ior * xr + ioi * xi));
    double P[8], N[4];
    P[0] = x00 * i0 + xr * ior + xi * ioi;
    P[1] = xi * ior - xr * ioi;
    P[2] = x00 * ior + xr * i1;
    P[3] = x00 * ioi + xi * i1;
    P[4] = xr * i0 + x11 * ior;
    P[5] = -xi * i0 - x11 * ioi;
    P[6] = xr * ior + xi * ioi + x11 * i1;
    P[7] = xr * ioi - xi * ior;
    N[0] = P[0] * i0 + (P[4] * ior - P[5] * ioi) - i0;
    N[1] = (P[2] * ior + P[3] * ioi) + P[6] * i1 - i1;
    N[2] = P[0] * ior + P[1] * ioi + P[4] * i1 - ior;
    N[3] = P[0] * ioi - P[1] * ior - P[5] * i1 - ioi;
#pragma unroll
    for (int c = 0; c < 4; ++c) g.NP[c * plane + o] = N[c];
#pragma unroll
    for (int c = 0; c < 8; ++c) g.NP[(4 + c) * plane + o] = P[c];
#pragma unroll
    for (int j = 0; j < kMaxJ; ++j)
      if (j < J) {
        const double Vj = v[j][i];
        g.V[j * plane + o] = Vj;
        // rho = |V^2 q + V| / max(V, eps) = |V q + 1| min(V / eps, 1), q the
        // rank-merged quadratic form (as k_estep_mx)
        const double q = ((s_c[j][0][fl] * N[0] + s_c[j][1][fl] * N[1]) +
                          2.0 * (s_c[j][2][fl] * N[2] + s_c[j][3][fl] * N[3])) * s_irk[j];
        a.hatW[j * plane + o] = fabs(fma(Vj, q, 1.0)) * fmin(Vj * (1.0 / kEps), 1.0);
      }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) ll += __shfl_xor(ll, m, 64);
  if (lane == 0) g.lw[(size_t)tt * a.nft + ft] = ll;
}

// The statistics as 16x16x4 FP64 MFMAs per bin, frames as the k dimension:
// with A[m = j1][k = t] = V_j1(t) and B[k = t][n = j2] = V_j2(t) N_c(t),
// D[j1][j2] accumulates the pair sums of component c for all (j1, j2) at
// once (the j1 > j2 half is discarded), and B[k = t][n = c] = P_c(t) gives
// the cross sums D[j][c].  Lane (fl, tq) supplies the A and B operands of
// row/column fl and frame tq from one LDS read of V_fl(t).  Block = 8 waves
// on one (16-bin tile, frame chunk); wave wv owns bins 2 wv, 2 wv + 1 (five
// 16x16 accumulators each).  A frame tile's J + 12 planes are staged point-
// major in LDS ([16 frames][16 bins][RS], RS = (J + 12) | 1 so the 16 rows a
// wave reads land on distinct banks), the next tile's values already in
// flight in registers while the current one is summed.  (Was VALU pair FMAs
// over the same staged tile at 5.48 ms for J = 16 at C3's size;
// profiles/r6_struct_J16K32_sum.txt.)
constexpr int kEgsThreads = 512;
constexpr int kEgsRows = (kMaxJ + 12) | 1;
__global__ __launch_bounds__(kEgsThreads) void k_egen_stats(const EArgs a, const GArgs g) {
  HALT_GUARD(a.halt);
  const int J = g.J, NP = J * (J + 1) / 2, NACC = 4 * NP + 8 * J;
  const int tid = threadIdx.x, lane = tid & 63, fl = lane & 15, tq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ft = blockIdx.x, f0 = ft * 16, y = blockIdx.y;
  const int nr = J + 12, RS = nr | 1;
  extern __shared__ __attribute__((aligned(16))) double s_t[];   // [16 frames][16 bins][RS]
  d4 acc[2][5];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int c = 0; c < 5; ++c) acc[bi][c] = d4{0.0, 0.0, 0.0, 0.0};
  const size_t plane = (size_t)a.Tp * a.Fp;
  const int tb = a.tbase + y * a.tpc, te = min(tb + a.tpc, a.ntt);
  // staging: thread tid carries point e = tid & 255 of rows r = 2 k + (tid >> 8)
  // (wave-uniform: each row's plane is a scalar base, the point a 32-bit offset)
  const int e = tid & 255, rh = __builtin_amdgcn_readfirstlane(tid >> 8), etl = e >> 4, efl = e & 15;
  constexpr int kPre = (kMaxJ + 12 + 1) / 2;
  double pre[2][kPre];   // two tiles in flight
  // Loads and stores unconditional (rows past nr repeat the last; a tile
  // past the chunk re-reads its last and is never staged), so every path
  // reaches the loop head with the same two batches outstanding and the
  // older one is waited for alone.
  auto load = [&](double(&p)[kPre], int tt) {
    const unsigned o = (unsigned)((min(tt, te - 1) * 16 + etl) * a.Fp + f0 + efl);
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      const int r = min(2 * k + rh, nr - 1);
      const double *base = r < J ? g.V + r * plane : g.NP + (r - J) * plane;
      p[k] = __builtin_nontemporal_load(base + o);
    }
  };
  auto stage = [&](const double(&p)[kPre]) {
    __syncthreads();   // (the previous tile's reads)
#pragma unroll
    for (int k = 0; k < kPre; ++k) s_t[e * RS + min(2 * k + rh, nr - 1)] = p[k];
    __syncthreads();
  };
  // MFMA operands: lane (fl, tq) reads V_fl (fl < J), N_0..3 and P_fl (fl <
  // 8) of its point; out-of-range lanes read a valid slot and select zero
  const int vcol = min(fl, J - 1), xcol = J + 4 + (fl & 7);
  const bool vok = fl < J, xok = fl < 8;
  auto sum_tile = [&]() {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int b = 2 * wv + bi;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double *pt = s_t + ((4 * q + tq) * 16 + b) * RS;   // point (frame 4 q + tq, bin b)
        const double vr = pt[vcol], pr = pt[xcol];
        const double n0 = pt[J], n1 = pt[J + 1], n2 = pt[J + 2], n3 = pt[J + 3];
        const double v = vok ? vr : 0.0, px = xok ? pr : 0.0;
        acc[bi][0] = mfma4(v, v * n0, acc[bi][0]);
        acc[bi][1] = mfma4(v, v * n1, acc[bi][1]);
        acc[bi][2] = mfma4(v, v * n2, acc[bi][2]);
        acc[bi][3] = mfma4(v, v * n3, acc[bi][3]);
        acc[bi][4] = mfma4(v, px, acc[bi][4]);
      }
    }
  };
  if (tb < te) {
    load(pre[0], tb);
    load(pre[1], tb + 1);
    for (int tt = tb; tt < te; tt += 2) {
      stage(pre[0]);
      load(pre[0], tt + 2);
      sum_tile();
      if (tt + 1 < te) {   // (block-uniform)
        stage(pre[1]);
        sum_tile();
      }
      load(pre[1], tt + 3);
    }
  }
  // lane (fl, tq), register i: D[tq + 4 i][fl]
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    double *out = a.part + ((size_t)(a.ybase + y) * a.Fp + f0 + 2 * wv + bi) * NACC;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j1 = tq + 4 * i, j2 = fl;
      if (j1 <= j2 && j2 < J) {
        const int p = j1 * J - j1 * (j1 - 1) / 2 + j2 - j1;   // canonical index of (j1, j2)
#pragma unroll
        for (int c = 0; c < 4; ++c) out[4 * p + c] = acc[bi][c][i];
      }
      if (j1 < J && fl < 8) out[4 * NP + 8 * j1 + fl] = acc[bi][4][i];
    }
  }
  if (tid == 0) {   // the chunk's loglik, its tiles in order
    double l = 0.0;
    for (int tt = tb; tt < te; ++tt) l += g.lw[(size_t)tt * a.nft + ft];
    a.llpart[(a.ybase + y) * a.nft + ft] = l;
  }
}

// Fused many-source E-step (J > 8, KP <= 32): k_egen_point's point pass and
// k_egen_stats' statistics in one block per (16-bin tile, frame chunk), V, N
// and P never leaving the LDS slab (the two-pass form writes and re-reads
// 28 planes, 4.6 GB at J = 16 and C3's size, and its point pass is bound by
// those writes; profiles/r6_ab_egen_point.txt).  Per frame tile, three phases
// between barriers:
//   V      wave wv forms V of sources 2 wv, 2 wv + 1 on 16x16x4 MFMA (its W
//          operands held in registers for the chunk, the next tile's TW
//          operands loaded while the current tile is summed) into the slab;
//   point  thread pair (2 e, 2 e + 1) owns point e: Sigma_x summed over the
//          even / odd sources and combined across the pair, then both form
//          the guarded inverse, P and N (the pair's halves write N and P to
//          the slab) and rho of their own sources to global;
//   stats  as k_egen_stats, from the slab.
template <int NKS>
__global__ __launch_bounds__(kEgsThreads) void k_egen_fused(const EArgs a, const GArgs g) {
  HALT_GUARD(a.halt);
  const int J = g.J, NP = J * (J + 1) / 2, NACC = 4 * NP + 8 * J;
  const int tid = threadIdx.x, lane = tid & 63, fl = lane & 15, tq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ft = blockIdx.x, f0 = ft * 16, y = blockIdx.y;
  const int nr = J + 12, RS = nr | 1;
  const int tb = a.tbase + y * a.tpc, te = min(tb + a.tpc, a.ntt);
  const size_t plane = (size_t)a.Tp * a.Fp;
  extern __shared__ __attribute__((aligned(16))) double s_t[];   // [256 points][RS], then W
  double *s_w = s_t + 256 * RS;           // [J][KP][16 bins]: the tile's W operands
  // Sigma_x coefficients per (source, component, bin), the source stride 80
  // doubles (= 16 mod 32 banks) so a half-wave's 16 bins x even / odd
  // sources fall on 32 distinct banks
  __shared__ double s_cfb[kMaxJ][80];
  auto cf = [&](int b, int j, int c) -> double & { return s_cfb[j][16 * c + b]; };
  __shared__ double s_irk[kMaxJ];
  __shared__ double s_ll[kEgsThreads / 64];
  if (tid < 16 * J) {
    const int j = tid >> 4, b = tid & 15, f = f0 + b;
    double al = 0, be = 0, gr = 0, gi = 0;
    for (int r = a.roff[j]; r < a.roff[j + 1]; ++r) {
      const double2 a0 = a.A[(size_t)(2 * r) * a.Fp + f];
      const double2 a1 = a.A[(size_t)(2 * r + 1) * a.Fp + f];
      al += a0.x * a0.x + a0.y * a0.y;
      be += a1.x * a1.x + a1.y * a1.y;
      gr += a0.x * a1.x + a0.y * a1.y;
      gi += a0.y * a1.x - a0.x * a1.y;
    }
    cf(b, j, 0) = al;
    cf(b, j, 1) = be;
    cf(b, j, 2) = gr;
    cf(b, j, 3) = gi;
  }
  if (tid < J) s_irk[tid] = 1.0 / (double)(a.roff[tid + 1] - a.roff[tid]);
  constexpr int KP = 4 * NKS;
  for (int idx = tid; idx < J * KP * 16; idx += kEgsThreads)
    s_w[idx] = a.Wkf[(size_t)(idx >> 4) * a.Fp + f0 + (idx & 15)];
  // V phase: sources ja, ja + 1 of this wave (clamped operands past J - 1)
  const int ja = 2 * wv, jA = min(ja, J - 1), jB = min(ja + 1, J - 1);
  const double *wA = s_w + (jA * KP + tq) * 16 + fl, *wB = s_w + (jB * KP + tq) * 16 + fl;
  double tr[2][NKS];
  auto load_tw = [&](int tt) {
    const int t = min(tt, te - 1) * 16 + fl;
    const double *tA = a.TW + ((size_t)jA * a.KP + tq) * a.Tp + t;
    const double *tB = a.TW + ((size_t)jB * a.KP + tq) * a.Tp + t;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      tr[0][s] = tA[(size_t)(4 * s) * a.Tp];
      tr[1][s] = tB[(size_t)(4 * s) * a.Tp];
    }
  };
  // point phase: point e = (frame tl, bin b), half h (even / odd sources)
  const int e = tid >> 1, h = tid & 1, tl = e >> 4, b = e & 15, f = f0 + b;
  const double psd = a.psd[f];
  double cx[4];
  auto load_cx = [&](int tt) {
    const size_t o = (size_t)(min(tt, te - 1) * 16 + tl) * a.Fp + f;
    cx[0] = a.cx00[o];
    cx[1] = a.cx11[o];
    cx[2] = a.cxr[o];
    cx[3] = a.cxi[o];
  };
  // statistics phase: v_mfma_f64_4x4x4_4b with block = bin (lane = 16 X +
  // 4 b + Y: A[m=Y][k=X], B[k=X][n=Y], D[m=X][n=Y] of block b), k = frame.
  // Wave wv owns bin quad bq = wv / 2 (bins 4 bq + b) and half hf = wv % 2:
  // the pair blocks (j1 block jb1 <= j2 block jb2, 4 sources each) of
  // components 2 hf, 2 hf + 1 and the cross blocks of sources 8 hf .. 8 hf + 7
  // -- 24 one-double accumulators, upper-triangle blocks only (40% fewer
  // matrix cycles than all 16 x 16 pairs on 16x16x4)
  const int X = lane >> 4, Yl = lane & 3, bq = wv >> 1, hf = wv & 1;
  const int sbin = 4 * bq + ((lane >> 2) & 3);
  double accp[10][2], accx[2][2];
#pragma unroll
  for (int pb = 0; pb < 10; ++pb) accp[pb][0] = accp[pb][1] = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u) accx[u][0] = accx[u][1] = 0.0;
  double ll = 0.0;
  if (tb < te) {
    load_tw(tb);
    load_cx(tb);
  }
  for (int tt = tb; tt < te; ++tt) {
    __syncthreads();   // (the slab's previous readers; at the first tile, s_cf)
    {
      d4 vA = d4{0.0, 0.0, 0.0, 0.0}, vB = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < NKS; ++s) {
        vA = mfma4(tr[0][s], wA[64 * s], vA);
        vB = mfma4(tr[1][s], wB[64 * s], vB);
      }
      load_tw(tt + 1);
      if (ja < J)   // (wave-uniform)
#pragma unroll
        for (int i = 0; i < 4; ++i) s_t[((tq + 4 * i) * 16 + fl) * RS + ja] = vA[i];
      if (ja + 1 < J)
#pragma unroll
        for (int i = 0; i < 4; ++i) s_t[((tq + 4 * i) * 16 + fl) * RS + ja + 1] = vB[i];
    }
    __syncthreads();
    {
      double *pt = s_t + e * RS;
      double d0 = 0.0, d1 = 0.0, ore = 0.0, oim = 0.0, vk[kMaxJ / 2];
#pragma unroll
      for (int m = 0; m < kMaxJ / 2; ++m) {
        const int j = 2 * m + h, jc = min(j, J - 1);
        vk[m] = pt[jc];   // (kept for rho below)
        const double vj = j < J ? vk[m] : 0.0;
        d0 = fma(cf(b, jc, 0), vj, d0);
        d1 = fma(cf(b, jc, 1), vj, d1);
        ore = fma(cf(b, jc, 2), vj, ore);
        oim = fma(cf(b, jc, 3), vj, oim);
      }
      d0 = psd + (d0 + __shfl_xor(d0, 1, 64));
      d1 = psd + (d1 + __shfl_xor(d1, 1, 64));
      ore += __shfl_xor(ore, 1, 64);
      oim += __shfl_xor(oim, 1, 64);
      const double x00 = cx[0], x11 = cx[1], xr = cx[2], xi = cx[3];
      load_cx(tt + 1);
      // inv_herm_mat_2d (signalTools.py:177-194)
      double det = d0 * d1 - (ore * ore + oim * oim);
      const double dg = det + kEps;
      det = (dg > 0.0 ? 1.0 : (dg < 0.0 ? -1.0 : 0.0)) * fmax(fabs(det), kEps);
      const double rdet = rcp_nr(det);
      const double i0 = d1 * rdet, i1 = d0 * rdet, ior = -ore * rdet, ioi = -oim * rdet;
      const int t = tt * 16 + tl;
      if (h == 0 && f < a.F && t < a.T)
        ll += log(det * M_PI) + (i0 * x00 + i1 * x11 + 2.0 * (ior * xr + ioi * xi));
      double P[8], N[4];
      P[0] = x00 * i0 + xr * ior + xi * ioi;
      P[1] = xi * ior - xr * ioi;
      P[2] = x00 * ior + xr * i1;
      P[3] = x00 * ioi + xi * i1;
      P[4] = xr * i0 + x11 * ior;
      P[5] = -xi * i0 - x11 * ioi;
      P[6] = xr * ior + xi * ioi + x11 * i1;
      P[7] = xr * ioi - xi * ior;
      N[0] = P[0] * i0 + (P[4] * ior - P[5] * ioi) - i0;
      N[1] = (P[2] * ior + P[3] * ioi) + P[6] * i1 - i1;
      N[2] = P[0] * ior + P[1] * ioi + P[4] * i1 - ior;
      N[3] = P[0] * ioi - P[1] * ior - P[5] * i1 - ioi;
      if (h == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) pt[J + c] = N[c];
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) pt[J + 4 + c] = P[c];
      }
      const size_t o = (size_t)t * a.Fp + f;
      // (sources past J - 1 clamp to J - 1 and store the very value its
      // owner stores -- both halves hold bit-identical N -- so the stores
      // need no lane-divergent branch)
#pragma unroll
      for (int m = 0; m < kMaxJ / 2; ++m) {
        const int j = min(2 * m + h, J - 1);
        // rho = |V q + 1| min(V / eps, 1), q the rank-merged quadratic form
        const double q = ((cf(b, j, 0) * N[0] + cf(b, j, 1) * N[1]) +
                          2.0 * (cf(b, j, 2) * N[2] + cf(b, j, 3) * N[3])) * s_irk[j];
        const double vj = vk[m];   // (= pt[j]: the same clamped source)
        __builtin_nontemporal_store(fabs(fma(vj, q, 1.0)) * fmin(vj * (1.0 / kEps), 1.0),
                                    a.hatW + j * plane + o);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const double *pt = s_t + ((4 * g + X) * 16 + sbin) * RS;   // point (frame 4 g + X, bin sbin)
      double va[4], bn[4][2], px[2];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const int jj = 4 * jb + Yl;
        const double v = pt[min(jj, J - 1)];
        va[jb] = jj < J ? v : 0.0;
      }
      const double nc0 = pt[J + 2 * hf], nc1 = pt[J + 2 * hf + 1];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        bn[jb][0] = va[jb] * nc0;
        bn[jb][1] = va[jb] * nc1;
      }
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) px[cb] = pt[J + 4 + 4 * cb + Yl];
      // (the ten blocks spelled out: constant register indices)
#define EGF_PB(pb, j1b, j2b)                                              \
  if (4 * (j2b) < J) {   /* (wave-uniform) */                             \
    accp[pb][0] = mfma44(va[j1b], bn[j2b][0], accp[pb][0]);              \
    accp[pb][1] = mfma44(va[j1b], bn[j2b][1], accp[pb][1]);              \
  }
      EGF_PB(0, 0, 0) EGF_PB(1, 0, 1) EGF_PB(2, 0, 2) EGF_PB(3, 0, 3) EGF_PB(4, 1, 1)
      EGF_PB(5, 1, 2) EGF_PB(6, 1, 3) EGF_PB(7, 2, 2) EGF_PB(8, 2, 3) EGF_PB(9, 3, 3)
#undef EGF_PB
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (4 * (2 * hf + u) >= J) continue;   // (wave-uniform)
        // (its own LDS read: selecting va[2 hf + u] became a scratch access)
        const int jj = 4 * (2 * hf + u) + Yl;
        const double vr = pt[min(jj, J - 1)], vs = jj < J ? vr : 0.0;
        accx[u][0] = mfma44(vs, px[0], accx[u][0]);
        accx[u][1] = mfma44(vs, px[1], accx[u][1]);
      }
    }
  }
  // lane (X, b, Y) holds D[X][Y] of its bin: pair (4 jb1 + X, 4 jb2 + Y),
  // cross (source 4 jb + X, component 4 cb + Y)
  {
    double *out = a.part + ((size_t)(a.ybase + y) * a.Fp + f0 + sbin) * NACC;
#pragma unroll
    for (int pb = 0; pb < 10; ++pb) {
      const int jb1 = pb < 4 ? 0 : pb < 7 ? 1 : pb < 9 ? 2 : 3;
      const int jb2 = pb < 4 ? pb : pb < 7 ? pb - 3 : pb < 9 ? pb - 5 : 3;
      const int j1 = 4 * jb1 + X, j2 = 4 * jb2 + Yl;
      if (j1 <= j2 && j2 < J) {
        const int p = j1 * J - j1 * (j1 - 1) / 2 + j2 - j1;   // canonical index of (j1, j2)
        out[4 * p + 2 * hf] = accp[pb][0];
        out[4 * p + 2 * hf + 1] = accp[pb][1];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = 4 * (2 * hf + u) + X;
      if (j < J) {
        out[4 * NP + 8 * j + Yl] = accx[u][0];
        out[4 * NP + 8 * j + 4 + Yl] = accx[u][1];
      }
    }
  }
  // the chunk's loglik: lanes in order within a wave, then waves in order
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) ll += __shfl_xor(ll, m, 64);
  if (lane == 0) s_ll[wv] = ll;
  __syncthreads();
  if (tid == 0) {
    double l = 0.0;
    for (int w = 0; w < kEgsThreads / 64; ++w) l += s_ll[w];
    a.llpart[(a.ybase + y) * a.nft + ft] = l;
  }
}

__global__ void k_loglik(const double *__restrict__ llpart, const ESched es, double *__restrict__ out,
                         double inv_FT, const int *halt) {
  HALT_GUARD(halt);
  __shared__ double s[256];
  const double x = ll_partial_sum(llpart, es);
  s[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = -(s[0] * inv_FT);
}

// ---------------------------------------------------------------- host side
static EArgs e_args(const fasst_ctx *c, const double *psd_dev) {
  EArgs e{};
  const size_t plane = (size_t)c->Tp * c->Fp;
  e.cx00 = c->cx.p;
  e.cx11 = c->cx.p + plane;
  e.cxr = c->cx.p + 2 * plane;
  e.cxi = c->cx.p + 3 * plane;
  e.TW = c->TW.p;
  e.cxp = c->cxp.p;
  e.twp = c->twp.p;
  e.nttp = c->ntt;
  e.Wkf = c->Wkf.p;
  e.A = c->A.p;
  e.psd = psd_dev;
  e.hatW = c->hatW.p;
  e.halt = c->halt;
  e.part = c->epart.p;
  e.llpart = c->llpart.p;
  e.F = c->F;
  e.T = c->T;
  e.Fp = c->Fp;
  e.Tp = c->Tp;
  e.KP = c->KP;
  e.R = c->R;
  e.ntt = c->ntt;
  e.tpc = c->tpc_e;
  e.nft = c->nft;
  e.es = c->esched;
  for (int j = 0; j <= kMaxJ; ++j) e.roff[j] = j <= c->J ? c->roff[j] : c->R;
  return e;
}

// does the model's single-pass E-step read the Cx / the TW image (the
// context's FASST_ESTEP_IMG choice; the TW image on the preload path only)
// (J = 7 at K = 128 keeps the planes: with the 16-byte loads that one
// instantiation, already at the whole register file, spills 12 bytes per lane)
bool estep_cxi(const fasst_ctx *c) {
  return c->J <= 8 && (c->eimg & 1) && !(c->J == 7 && c->KP == 128);
}
bool estep_twi(const fasst_ctx *c) {
  return c->J <= 4 && (c->eimg & 2) && c->J * (c->KP / 4) <= 32;
}

// estep_mx_j<J> is instantiated by fasst_em_estep_j<J>.hip and nowhere else
// (a k_estep_mx instantiation named here too would be a second host stub)
extern template int estep_mx_j<1>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<2>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<3>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<4>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<5>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<6>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<7>(const fasst_ctx *, const EArgs *, int);
extern template int estep_mx_j<8>(const fasst_ctx *, const EArgs *, int);

static int estep_mx(const fasst_ctx *c, const EArgs *e, int ny) {
  switch (c->J) {
    case 1: return estep_mx_j<1>(c, e, ny);
    case 2: return estep_mx_j<2>(c, e, ny);
    case 3: return estep_mx_j<3>(c, e, ny);
    case 4: return estep_mx_j<4>(c, e, ny);
    case 5: return estep_mx_j<5>(c, e, ny);
    case 6: return estep_mx_j<6>(c, e, ny);
    case 7: return estep_mx_j<7>(c, e, ny);
    default: return estep_mx_j<8>(c, e, ny);
  }
}

// The operand images of the coming k_estep_mx launch (fasst_ctx.h): the Cx
// image rebuilt if an observation was written since it was packed, the TW
// image packed from TW unless the previous iteration's fused k_tw_update
// wrote it (tw_fresh: gem_iteration's prep_ready, which every batch start and
// every path around the fused tail clears)
static int estep_images(fasst_ctx *c, bool tw_fresh) {
  if (estep_cxi(c) && !(c->cxp_valid && c->cxp.p)) {
    const size_t n = (size_t)c->nft * c->ntt * 512;
    if (c->cxp.n != n)
      if (int st = c->cxp.alloc_uninit(n)) return st;
    k_cx_image<<<dim3(c->ntt, c->nft), 256, 0, c->stream>>>(c->cx.p, c->cxp.p, c->Fp, c->ntt,
                                                            (size_t)c->Tp * c->Fp);
    FASST_LAUNCH_CHECK();
    c->cxp_valid = true;
  }
  if (estep_twi(c)) {
    const size_t n = (size_t)c->ntt * c->J * (c->KP / 8) * 64;
    if (c->twp.n != n) {
      if (int st = c->twp.alloc_uninit(n)) return st;
      tw_fresh = false;
    }
    if (!tw_fresh) {
      k_tw_image<<<dim3(c->ntt, c->J), 256, 0, c->stream>>>(c->TW.p, c->twp.p, c->J, c->KP, c->Tp);
      FASST_LAUNCH_CHECK();
    }
  }
  return FASST_OK;
}

static void launch_estep(fasst_ctx *c, const EArgs &e, int ny) {
  prof_begin(c, KESTEP);
  estep_mx(c, &e, ny);
  prof_end(c, KESTEP);
}

// resident E-step blocks per CU
int estep_occupancy(const fasst_ctx *c) { return estep_mx(c, nullptr, 0); }

int estep_lds_limits() {
  struct L {
    const void *f;
    size_t bytes;
  };
  const L lim[] = {
      {(const void *)k_egen_stats, (size_t)kEgsRows * 256 * sizeof(double)},
      {(const void *)k_egen_fused<4>, (size_t)(kEgsRows * 256 + kMaxJ * 16 * 16) * sizeof(double)},
      {(const void *)k_egen_fused<8>, (size_t)(kEgsRows * 256 + kMaxJ * 32 * 16) * sizeof(double)},
  };
  for (const L &l : lim)
    if (hipFuncSetAttribute(l.f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes) != hipSuccess) {
      set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", l.bytes);
      return FASST_ERR_DEVICE;
    }
  return FASST_OK;
}

int launch_estep_phase(fasst_ctx *c, const double *psd_dev, bool tw_fresh) {
  const int J = c->J;
  const EArgs e = e_args(c, psd_dev);
  if (J > 8 && c->KP <= 32) {   // the fused many-source E-step
    GArgs gg{};
    gg.J = J;
    const size_t lds = (size_t)(((J + 12) | 1) * 256 + J * c->KP * 16) * sizeof(double);   // (ceiling: estep_lds_limits)
    prof_begin(c, KESTEP);
    if (c->KP == 16)
      k_egen_fused<4><<<dim3(c->nft, c->nchunk_e), kEgsThreads, lds, c->stream>>>(e, gg);
    else
      k_egen_fused<8><<<dim3(c->nft, c->nchunk_e), kEgsThreads, lds, c->stream>>>(e, gg);
    prof_end(c, KESTEP);
  } else if (J > 8) {   // the two-pass E-step (k_egen_point / k_egen_stats)
    GArgs gg{};
    gg.V = c->vgen.p;
    gg.NP = c->npgen.p;
    gg.lw = c->lgen.p;
    gg.J = J;
    prof_begin(c, KESTEP);
    if (c->KP == 64)   // (this path has KP > 32: the fused branch above took the rest)
      k_egen_point<16><<<dim3(c->ntt, c->nft), 64, 0, c->stream>>>(e, gg);
    else
      k_egen_point<32><<<dim3(c->ntt, c->nft), 64, 0, c->stream>>>(e, gg);
    const size_t lds = (size_t)((J + 12) | 1) * 256 * sizeof(double);   // (ceiling: estep_lds_limits)
    k_egen_stats<<<dim3(c->nft, c->nchunk_e), kEgsThreads, lds, c->stream>>>(e, gg);
    prof_end(c, KESTEP);
  } else {
    if (int st = estep_images(c, tw_fresh)) return st;
    launch_estep(c, e_args(c, psd_dev), c->nchunk_e);
  }
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

int launch_loglik(fasst_ctx *c, double *ll_dev) {
  prof_begin(c, KLL);
  k_loglik<<<1, 256, 0, c->stream>>>(c->llpart.p, c->esched, ll_dev,
                                     1.0 / ((double)c->F * (double)c->T), c->halt);
  prof_end(c, KLL);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

}  // namespace fasst
