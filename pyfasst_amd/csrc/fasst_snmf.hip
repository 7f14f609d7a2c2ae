// Stereo accompaniment IS-NMF on MI355X (gfx950), FP64: the reference's
// SIMM.stereo_NMF (SeparateLeadStereo/SIMM/SIMM.py:945-1104).
//
//   SX_R ~ WM diag(betaR^2) HM,  SX_L ~ WM diag(betaL^2) HM,  betaL = 1 - betaR
//
// One iteration is three steps (HM, WM with its column renormalisation, beta),
// each against the model left by the step before.  No F x N array but the two
// data planes lives on the device: every step is one launch of k_snmf_con,
// which forms hat_R and hat_L of a 16 x 16 tile on the FP64 MFMA from WM,
// beta^2 and HM, turns them into the ratios P_c = SX_c / max(hat_c^2, eps),
// Q_c = 1 / max(hat_c, eps) in registers, and feeds them straight back into
// the MFMA as the next product's operand (the accumulator-as-operand layout
// of 16x16x4, as fasst_nmf.hip).  One pass over SX_R / SX_L serves both
// channels' numerator and denominator.
//
// k_snmf_con is written once over a "kept" and a "contracted" index:
//   HM step   kept = frame, contracted = bin:   num[n][r] = sum_f P[f][n] W[f][r] b2_c[r]
//   WM step   kept = bin, contracted = frame:   num[f][r] = sum_n P[f][n] H[n][r] b2_c[r]
//   beta step kept = frame, contracted = bin, the channels apart and without
//             b2: T_c[n][r] = sum_f P_c[f][n] W[f][r], then the per-tile
//             reduction sum_n T_c[n][r] H[n][r] (no R x N intermediate).
// Parameters live component-minor and zero-padded: W [Fa][Rp], Ht [Na][Rp]
// (HM frame-major), Fa / Na / Rp the sizes rounded up to 16.  Pad components
// carry W = H = beta^2 = 0 and so add nothing to hat; pad bins and frames are
// masked out of the ratios, so nothing of the padding reaches a reduction.
//
// Register layout of a tile (lane = fl + 16 tq):
//   hat product   A[i = fl][k = tq]: contracted index c0 + 4 (fl & 3) + (fl >> 2),
//                 component NKS tq + s at step s (a lane's operand run is NKS
//                 consecutive doubles of one row);
//                 B[k = tq][j = fl]: kept index k0 + fl, same component, times b2_c;
//                 D register m (row tq + 4 m, column fl) is therefore hat at
//                 (contracted c0 + 4 tq + m, kept k0 + fl): a lane's four data
//                 values are consecutive in the contracted index.
//   contraction   A = the ratio of register m (i = fl kept, k = tq <-> contracted
//                 c0 + 4 tq + m), B[k = tq][j = fl] = the contracted operand's
//                 row c0 + 4 tq + m at component 16 oc + fl; D register m' is
//                 (kept k0 + tq + 4 m', component 16 oc + fl).
// Every wave owns a run of contracted tiles and writes its own partial; the
// consumers sum the partials in index order, so a run is reproducible bit for
// bit.
#include "fasst_device.h"

#include <algorithm>
#include <vector>

#include "../../include/fasst_simm.h"

namespace fasst {

constexpr double kSnmfEps = 1e-20;  // SIMM.py:951
constexpr int kSnmfMaxR = 128;
constexpr int kSnmfH = 0, kSnmfW = 1, kSnmfB = 2;

// the loop-invariant kept operand of the hat products: row k0 + fl of keptOp
// times betaR^2 / betaL^2 (b2: [2][Rp])
template <int NKC>
__device__ __forceinline__ void snmf_kept(const double *__restrict__ keptOp,
                                          const double *__restrict__ b2, int k0, int fl, int tq,
                                          double (&bk)[2][4 * NKC]) {
  constexpr int Rp = 16 * NKC, NKS = 4 * NKC;
  const double *kr = keptOp + (size_t)(k0 + fl) * Rp + NKS * tq;
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const double v = kr[s];
    bk[0][s] = v * b2[NKS * tq + s];
    bk[1][s] = v * b2[Rp + NKS * tq + s];
  }
}

// hat_R, hat_L of one tile (clamped at eps): two accumulation chains per channel
template <int NKC>
__device__ __forceinline__ void snmf_hat(const double (&a)[4 * NKC], const double (&bk)[2][4 * NKC],
                                         d4 &hR, d4 &hL) {
  constexpr int NKS = 4 * NKC;
  d4 r0 = d4{0.0, 0.0, 0.0, 0.0}, r1 = r0, l0 = r0, l1 = r0;
#pragma unroll
  for (int s = 0; s < NKS; s += 2) {
    r0 = mfma4(a[s], bk[0][s], r0);
    l0 = mfma4(a[s], bk[1][s], l0);
    r1 = mfma4(a[s + 1], bk[0][s + 1], r1);
    l1 = mfma4(a[s + 1], bk[1][s + 1], l1);
  }
  hR = r0 + r1;
  hL = l0 + l1;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    hR[m] = fmax(hR[m], kSnmfEps);
    hL[m] = fmax(hL[m], kSnmfEps);
  }
}

// A workgroup owns the 16 kept indices k0 .. k0 + 15 and, per wave, tpc
// contracted tiles; grid.y splits the contracted range further, grid.z the
// output components into slabs of NOC tiles (Rp > 64: the accumulators of all
// eight tiles do not fit the register file next to the hat operands).
// part: kSnmfH / kSnmfW  [chunk][num, den][nKa][Rp], chunk = 4 blockIdx.y + wave
//       kSnmfB           [blockIdx.x][chunk][numR, denR, numL, denL][Rp]
template <int NKC, int NOC, int MODE>
__global__ __launch_bounds__(256) void k_snmf_con(const double *__restrict__ keptOp,
                                                  const double *__restrict__ conOp,
                                                  const double *__restrict__ b2,
                                                  const double *__restrict__ DR,
                                                  const double *__restrict__ DL, int F, int N,
                                                  int tpc, double *__restrict__ part) {
  constexpr int Rp = 16 * NKC, NKS = 4 * NKC;
  constexpr bool DT = MODE == kSnmfW;  // data rows run along the kept index
  constexpr int NA = MODE == kSnmfB ? 4 : 2;
  constexpr bool PF = NKC <= 4;  // prefetch the next tile where the registers allow
  const int nKept = DT ? F : N, nCon = DT ? N : F;
  const int lane = threadIdx.x & 63, fl = lane & 15, tq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = blockIdx.x * 16, oc0 = blockIdx.z * NOC;
  const int nct = (nCon + 15) / 16;
  const int chunk = blockIdx.y * 4 + wv;
  const int ctb = min(chunk * tpc, nct), cte = min(ctb + tpc, nct);

  double bk[2][NKS];
  snmf_kept<NKC>(keptOp, b2, k0, fl, tq, bk);
  double bo[2][NOC];  // beta^2 of this lane's output components
#pragma unroll
  for (int kc = 0; kc < NOC; ++kc) {
    const int oc = min(oc0 + kc, NKC - 1);
    bo[0][kc] = b2[16 * oc + fl];
    bo[1][kc] = b2[Rp + 16 * oc + fl];
  }
  (void)bo;  // the beta step contracts without them
  d4 acc[NA][NOC];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int kc = 0; kc < NOC; ++kc) acc[a][kc] = d4{0.0, 0.0, 0.0, 0.0};

  const int kept = k0 + fl, cperm = 4 * (fl & 3) + (fl >> 2);
  const bool kv = kept < nKept;
  double a[NKS], xr[4], xl[4];
  auto load = [&](int ct, double (&av)[NKS], double (&r)[4], double (&l)[4]) {
    const int c0 = ct * 16;
    const double *ar = conOp + (size_t)(c0 + cperm) * Rp + NKS * tq;
#pragma unroll
    for (int s = 0; s < NKS; ++s) av[s] = ar[s];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int con = c0 + 4 * tq + m;
      const bool ok = kv && con < nCon;
      const size_t o = DT ? (size_t)kept * N + con : (size_t)con * N + kept;
      r[m] = ok ? DR[o] : 0.0;
      l[m] = ok ? DL[o] : 0.0;
    }
  };
  if (ctb < cte) load(ctb, a, xr, xl);
  for (int ct = ctb; ct < cte; ++ct) {
    const int c0 = ct * 16;
    double an[NKS], xrn[4], xln[4];
    if (PF && ct + 1 < cte) load(ct + 1, an, xrn, xln);
    d4 hR, hL;
    snmf_hat<NKC>(a, bk, hR, hL);
    double pR[4], qR[4], pL[4], qL[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      // pad bins / frames: x = 0 gives p = 0, q is masked
      const bool ok = kv && c0 + 4 * tq + m < nCon;
      const double r = hR[m], l = hL[m];
      pR[m] = xr[m] * rcp_nr(fmax(r * r, kSnmfEps));
      pL[m] = xl[m] * rcp_nr(fmax(l * l, kSnmfEps));
      qR[m] = ok ? rcp_nr(r) : 0.0;
      qL[m] = ok ? rcp_nr(l) : 0.0;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double *cr = conOp + (size_t)(c0 + 4 * tq + m) * Rp + fl;
#pragma unroll
      for (int kc = 0; kc < NOC; ++kc) {
        if (oc0 + kc >= NKC) continue;  // wave-uniform: the last slab's tail
        const double w = cr[16 * (oc0 + kc)];
        if constexpr (MODE == kSnmfB) {
          acc[0][kc] = mfma4(pR[m], w, acc[0][kc]);
          acc[1][kc] = mfma4(qR[m], w, acc[1][kc]);
          acc[2][kc] = mfma4(pL[m], w, acc[2][kc]);
          acc[3][kc] = mfma4(qL[m], w, acc[3][kc]);
        } else {
          const double wR = w * bo[0][kc], wL = w * bo[1][kc];
          acc[0][kc] = mfma4(pR[m], wR, acc[0][kc]);
          acc[1][kc] = mfma4(qR[m], wR, acc[1][kc]);
          acc[0][kc] = mfma4(pL[m], wL, acc[0][kc]);
          acc[1][kc] = mfma4(qL[m], wL, acc[1][kc]);
        }
      }
    }
    if (PF && ct + 1 < cte) {
#pragma unroll
      for (int s = 0; s < NKS; ++s) a[s] = an[s];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        xr[m] = xrn[m];
        xl[m] = xln[m];
      }
    } else if (!PF && ct + 1 < cte) {
      load(ct + 1, a, xr, xl);
    }
  }

  if constexpr (MODE == kSnmfB) {
    // sum_n T_c[n][r] HM[r][n] over the tile's 16 frames (rows tq + 4 m of the
    // lane's column; pad frames hold T = 0 and Ht = 0), lanes tq = 1..3 folded
    // into tq = 0 in a fixed order
    double *pb = part + ((size_t)blockIdx.x * (4 * gridDim.y) + chunk) * 4 * Rp;
#pragma unroll
    for (int kc = 0; kc < NOC; ++kc) {
      if (oc0 + kc >= NKC) continue;
      const int comp = 16 * (oc0 + kc) + fl;
      double h[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) h[m] = keptOp[(size_t)(k0 + tq + 4 * m) * Rp + comp];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const d4 v = acc[q][kc];
        double t = ((v[0] * h[0] + v[1] * h[1]) + v[2] * h[2]) + v[3] * h[3];
        t += __shfl_xor(t, 16);
        t += __shfl_xor(t, 32);
        if (tq == 0) pb[q * Rp + comp] = t;
      }
    }
  } else {
    const size_t nKa = (size_t)((nKept + 15) / 16) * 16;
    double *pn = part + (size_t)chunk * 2 * nKa * Rp;
#pragma unroll
    for (int kc = 0; kc < NOC; ++kc) {
      if (oc0 + kc >= NKC) continue;
      const int comp = 16 * (oc0 + kc) + fl;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const size_t o = (size_t)(k0 + tq + 4 * m) * Rp + comp;
        pn[o] = acc[0][kc][m];
        pn[nKa * Rp + o] = acc[1][kc][m];
      }
    }
  }
}

// ISDistortion(SX_R, hat_R) and ISDistortion(SX_L, hat_L) (SIMM.py:34-44), a
// partial pair per wave: perr [wave][2].  Geometry of the HM step.
template <int NKC>
__global__ __launch_bounds__(256) void k_snmf_err(const double *__restrict__ Ht,
                                                  const double *__restrict__ W,
                                                  const double *__restrict__ b2,
                                                  const double *__restrict__ DR,
                                                  const double *__restrict__ DL, int F, int N,
                                                  int tpc, double *__restrict__ perr) {
  constexpr int Rp = 16 * NKC, NKS = 4 * NKC;
  const int lane = threadIdx.x & 63, fl = lane & 15, tq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = blockIdx.x * 16, nct = (F + 15) / 16;
  const int chunk = blockIdx.y * 4 + wv;
  const int ctb = min(chunk * tpc, nct), cte = min(ctb + tpc, nct);
  double bk[2][NKS];
  snmf_kept<NKC>(Ht, b2, k0, fl, tq, bk);
  const int n = k0 + fl, cperm = 4 * (fl & 3) + (fl >> 2);
  double eR = 0.0, eL = 0.0;
  for (int ct = ctb; ct < cte; ++ct) {
    const int c0 = ct * 16;
    double a[NKS];
    const double *ar = W + (size_t)(c0 + cperm) * Rp + NKS * tq;
#pragma unroll
    for (int s = 0; s < NKS; ++s) a[s] = ar[s];
    d4 hR, hL;
    snmf_hat<NKC>(a, bk, hR, hL);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int f = c0 + 4 * tq + m;
      if (n < N && f < F) {
        const double r = DR[(size_t)f * N + n] / hR[m], l = DL[(size_t)f * N + n] / hL[m];
        eR += -log(r) + r - 1.0;
        eL += -log(l) + l - 1.0;
      }
    }
  }
  // lanes folded in a fixed (butterfly) order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    eR += __shfl_xor(eR, o);
    eL += __shfl_xor(eL, o);
  }
  if (lane == 0) {
    const size_t w = (size_t)blockIdx.x * (4 * gridDim.y) + chunk;
    perr[2 * w] = eR;
    perr[2 * w + 1] = eL;
  }
}

// out[0] = sum of the R partials + sum of the L partials, one workgroup
__global__ __launch_bounds__(256) void k_snmf_err_sum(const double *__restrict__ perr, int nw,
                                                      double *__restrict__ out) {
  __shared__ double s_r[256], s_l[256];
  double r = 0.0, l = 0.0;
  for (int i = threadIdx.x; i < nw; i += 256) {
    r += perr[2 * i];
    l += perr[2 * i + 1];
  }
  s_r[threadIdx.x] = r;
  s_l[threadIdx.x] = l;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      s_r[threadIdx.x] += s_r[threadIdx.x + w];
      s_l[threadIdx.x] += s_l[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s_r[0] + s_l[0];
}

// HM *= (num / max(den, eps)) ** omega (SIMM.py:1021-1031) on the frame-major
// Ht, the chunk partials summed in index order
__global__ void k_snmf_h_upd(double *__restrict__ Ht, const double *__restrict__ part, int nchunk,
                             int N, int R, int Rp, double omega) {
  const size_t slab = (size_t)((N + 15) / 16) * 16 * Rp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)N * Rp;
       i += (size_t)gridDim.x * blockDim.x) {
    if ((int)(i % Rp) >= R) continue;
    double n = 0.0, d = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      n += part[(size_t)c * 2 * slab + i];
      d += part[(size_t)c * 2 * slab + slab + i];
    }
    Ht[i] *= pow_omega(n / fmax(d, kSnmfEps), omega);
  }
}

// WM *= (num / den) ** omega, the denominator unclamped (SIMM.py:1045-1055);
// sumWM = WM.sum(0), columns with sumWM > 0 divided by it (:1057-1059).  One
// workgroup per component: the column sum is a fixed-order tree.
__global__ __launch_bounds__(256) void k_snmf_w_upd(double *__restrict__ W,
                                                    const double *__restrict__ part, int nchunk,
                                                    int F, int Rp, double omega,
                                                    double *__restrict__ s_out) {
  __shared__ double s_red[256];
  const int r = blockIdx.x;
  const size_t slab = (size_t)((F + 15) / 16) * 16 * Rp;
  double acc = 0.0;
  for (int f = threadIdx.x; f < F; f += 256) {
    const size_t i = (size_t)f * Rp + r;
    double n = 0.0, d = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      n += part[(size_t)c * 2 * slab + i];
      d += part[(size_t)c * 2 * slab + slab + i];
    }
    const double w = W[i] * pow_omega(n / d, omega);
    W[i] = w;
    acc += w;
  }
  s_red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
    __syncthreads();
  }
  const double s = s_red[0];
  if (s > 0)
    for (int f = threadIdx.x; f < F; f += 256) W[(size_t)f * Rp + r] /= s;
  if (threadIdx.x == 0) s_out[r] = s;
}

// HM rows times sumWM, unconditionally (SIMM.py:1060)
__global__ void k_snmf_hscale(double *__restrict__ Ht, const double *__restrict__ s, int N, int R,
                              int Rp) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)N * Rp;
       i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i % Rp);
    if (r < R) Ht[i] *= s[r];
  }
}

// beta step (SIMM.py:1075-1090) from the nblk tile partials [blk][4][Rp]; one
// workgroup per component.  beta: [2][Rp] (R, L), b2 their squares.
__global__ __launch_bounds__(256) void k_snmf_beta(const double *__restrict__ part, int nblk,
                                                   int Rp, double bexp, double *__restrict__ beta,
                                                   double *__restrict__ b2) {
  __shared__ double s_red[4][256];
  const int r = blockIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += part[((size_t)b * 4 + q) * Rp + r];
#pragma unroll
  for (int q = 0; q < 4; ++q) s_red[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w)
#pragma unroll
      for (int q = 0; q < 4; ++q) s_red[q][threadIdx.x] += s_red[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double bR = fmax(beta[r] * pow(s_red[0][0] / s_red[1][0], bexp), kSnmfEps);
    const double bL = fmax(beta[Rp + r] * pow(s_red[2][0] / s_red[3][0], bexp), kSnmfEps);
    bR = bR / fmax(bR + bL, kSnmfEps);
    const double nL = 1.0 - bR;
    beta[r] = bR;
    beta[Rp + r] = nL;
    b2[r] = bR * bR;
    b2[Rp + r] = nL * nL;
  }
}

}  // namespace fasst

using namespace fasst;

struct snmf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int F = 0, N = 0, R = 0, Rp = 0, Fa = 0, Na = 0;
  // contraction geometry: grid.y and contracted tiles per wave, per kept axis
  int ng_h = 1, tpc_h = 1, ng_w = 1, tpc_w = 1;
  DBuf<double> SXR, SXL, W, Ht, beta, b2, s, part, bpart, perr, err;
};

namespace {

constexpr int kSnmfBlocks = 512;  // two workgroups per CU

// split nct contracted tiles over 4 waves x ng workgroups so that about
// kSnmfBlocks workgroups run, each wave keeping a few tiles
void snmf_geom(int nkept_tiles, int nct, int &ng, int &tpc) {
  int g = std::max(1, std::min(kSnmfBlocks / std::max(nkept_tiles, 1), (nct + 15) / 16));
  tpc = (nct + 4 * g - 1) / (4 * g);
  ng = ((nct + tpc - 1) / tpc + 3) / 4;
}

template <int NKC, int NOC>
int snmf_launch(snmf_ctx *c, int mode) {
  const int nz = (NKC + NOC - 1) / NOC;
  const int nft = c->Fa / 16, ntt = c->Na / 16;
  if (mode == kSnmfH)
    k_snmf_con<NKC, NOC, kSnmfH><<<dim3(ntt, c->ng_h, nz), 256, 0, c->stream>>>(
        c->Ht.p, c->W.p, c->b2.p, c->SXR.p, c->SXL.p, c->F, c->N, c->tpc_h, c->part.p);
  else if (mode == kSnmfW)
    k_snmf_con<NKC, NOC, kSnmfW><<<dim3(nft, c->ng_w, nz), 256, 0, c->stream>>>(
        c->W.p, c->Ht.p, c->b2.p, c->SXR.p, c->SXL.p, c->F, c->N, c->tpc_w, c->part.p);
  else if (mode == kSnmfB)
    k_snmf_con<NKC, NOC, kSnmfB><<<dim3(ntt, c->ng_h, nz), 256, 0, c->stream>>>(
        c->Ht.p, c->W.p, c->b2.p, c->SXR.p, c->SXL.p, c->F, c->N, c->tpc_h, c->bpart.p);
  else
    k_snmf_err<NKC><<<dim3(ntt, c->ng_h), 256, 0, c->stream>>>(
        c->Ht.p, c->W.p, c->b2.p, c->SXR.p, c->SXL.p, c->F, c->N, c->tpc_h, c->perr.p);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// mode: kSnmfH / kSnmfW / kSnmfB, 3 = the error partials
int snmf_dispatch(snmf_ctx *c, int mode) {
  switch (c->Rp / 16) {
    case 1: return snmf_launch<1, 1>(c, mode);
    case 2: return snmf_launch<2, 2>(c, mode);
    case 3: return snmf_launch<3, 3>(c, mode);
    case 4: return snmf_launch<4, 4>(c, mode);
    case 5: return snmf_launch<5, 3>(c, mode);
    case 6: return snmf_launch<6, 3>(c, mode);
    case 7: return snmf_launch<7, 4>(c, mode);
    default: return snmf_launch<8, 4>(c, mode);
  }
}

int snmf_error(snmf_ctx *c, int slot) {
  int st = snmf_dispatch(c, 3);
  if (st) return st;
  const int nw = (c->Na / 16) * 4 * c->ng_h;
  k_snmf_err_sum<<<1, 256, 0, c->stream>>>(c->perr.p, nw, c->err.p + slot);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

}  // namespace

extern "C" {

int snmf_create(int device, int F, int N, int R, snmf_ctx **out) {
  if (!out || F < 1 || N < 1 || R < 1) {
    set_error("snmf_create: bad sizes F=%d N=%d R=%d", F, N, R);
    return FASST_ERR_SHAPE;
  }
  if (R > kSnmfMaxR) {
    set_error("snmf_create: R=%d accompaniment components, the stereo NMF engine holds at most %d",
              R, kSnmfMaxR);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(device);
  snmf_ctx *c = new snmf_ctx();
  c->device = device;
  c->F = F;
  c->N = N;
  c->R = R;
  c->Rp = round_up(R, 16);
  c->Fa = round_up(F, 16);
  c->Na = round_up(N, 16);
  snmf_geom(c->Na / 16, c->Fa / 16, c->ng_h, c->tpc_h);
  snmf_geom(c->Fa / 16, c->Na / 16, c->ng_w, c->tpc_w);
  const size_t FN = (size_t)F * N, Rp = c->Rp;
  const size_t np = std::max((size_t)4 * c->ng_h * 2 * c->Na * Rp, (size_t)4 * c->ng_w * 2 * c->Fa * Rp);
  const size_t nw = (size_t)(c->Na / 16) * 4 * c->ng_h;
  int st = FASST_OK;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) st = FASST_ERR_DEVICE;
  if (!st) st = c->SXR.alloc(FN);
  if (!st) st = c->SXL.alloc(FN);
  if (!st) st = c->W.alloc((size_t)c->Fa * Rp);
  if (!st) st = c->Ht.alloc((size_t)c->Na * Rp);
  if (!st) st = c->beta.alloc(2 * Rp);
  if (!st) st = c->b2.alloc(2 * Rp);
  if (!st) st = c->s.alloc(Rp);
  if (!st) st = c->part.alloc(np);
  if (!st) st = c->bpart.alloc(nw * 4 * Rp);
  if (!st) st = c->perr.alloc(nw * 2);
  if (st) {
    snmf_destroy(c);
    return st;
  }
  *out = c;
  return FASST_OK;
}

int snmf_destroy(snmf_ctx *c) {
  if (!c) return FASST_OK;
  {
    DeviceGuard g(c->device);
    if (c->stream) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipStreamDestroy(c->stream);
    }
  }
  delete c;
  return FASST_OK;
}

int snmf_set_data(snmf_ctx *c, const double *SXR, const double *SXL) {
  if (!c || !SXR || !SXL) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const size_t FN = (size_t)c->F * c->N;
  FASST_TRY(c->SXR.put(SXR, FN, c->stream));
  FASST_TRY(c->SXL.put(SXL, FN, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int snmf_set_params(snmf_ctx *c, const double *WM, const double *HM, const double *betaR) {
  if (!c || !WM || !HM || !betaR) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const int F = c->F, N = c->N, R = c->R, Rp = c->Rp;
  // the padded, component-minor device layouts are packed on the host (the
  // parameters are small next to the data planes)
  std::vector<double> w((size_t)c->Fa * Rp, 0.0), ht((size_t)c->Na * Rp, 0.0), b(2 * Rp, 0.0),
      b2(2 * Rp, 0.0);
  for (int f = 0; f < F; ++f)
    for (int r = 0; r < R; ++r) w[(size_t)f * Rp + r] = WM[(size_t)f * R + r];
  for (int r = 0; r < R; ++r)
    for (int n = 0; n < N; ++n) ht[(size_t)n * Rp + r] = HM[(size_t)r * N + n];
  for (int r = 0; r < R; ++r) {
    b[r] = betaR[r];
    b[Rp + r] = 1.0 - betaR[r];  // SIMM.py:991
    b2[r] = b[r] * b[r];
    b2[Rp + r] = b[Rp + r] * b[Rp + r];
  }
  FASST_TRY(c->W.put(w.data(), w.size(), c->stream));
  FASST_TRY(c->Ht.put(ht.data(), ht.size(), c->stream));
  FASST_TRY(c->beta.put(b.data(), b.size(), c->stream));
  FASST_TRY(c->b2.put(b2.data(), b2.size(), c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int snmf_run(snmf_ctx *c, int n_iter, double omega, double *reco_err) {
  if (!c || n_iter < 0) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const int F = c->F, N = c->N, R = c->R, Rp = c->Rp;
  int st, slot = 0;
  if (reco_err) {
    if ((st = c->err.alloc((size_t)3 * n_iter + 1))) return st;
    if ((st = snmf_error(c, slot++))) return st;
  }
  const int eg = egrid((size_t)N * Rp);
  const int nbp = (c->Na / 16) * 4 * c->ng_h;
  for (int it = 0; it < n_iter; ++it) {
    if ((st = snmf_dispatch(c, kSnmfH))) return st;
    k_snmf_h_upd<<<eg, 256, 0, c->stream>>>(c->Ht.p, c->part.p, 4 * c->ng_h, N, R, Rp, omega);
    FASST_LAUNCH_CHECK();
    if (reco_err && (st = snmf_error(c, slot++))) return st;
    if ((st = snmf_dispatch(c, kSnmfW))) return st;
    k_snmf_w_upd<<<R, 256, 0, c->stream>>>(c->W.p, c->part.p, 4 * c->ng_w, F, Rp, omega, c->s.p);
    k_snmf_hscale<<<eg, 256, 0, c->stream>>>(c->Ht.p, c->s.p, N, R, Rp);
    FASST_LAUNCH_CHECK();
    if (reco_err && (st = snmf_error(c, slot++))) return st;
    if ((st = snmf_dispatch(c, kSnmfB))) return st;
    k_snmf_beta<<<R, 256, 0, c->stream>>>(c->bpart.p, nbp, Rp, omega * .1, c->beta.p, c->b2.p);
    FASST_LAUNCH_CHECK();
    if (reco_err && (st = snmf_error(c, slot++))) return st;
  }
  if (reco_err) FASST_TRY(c->err.get(reco_err, (size_t)3 * n_iter + 1, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int snmf_get_params(snmf_ctx *c, double *WM, double *HM, double *betaR, double *betaL) {
  if (!c) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const int F = c->F, N = c->N, R = c->R, Rp = c->Rp;
  std::vector<double> w((size_t)c->Fa * Rp), ht((size_t)c->Na * Rp), b(2 * Rp);
  FASST_TRY(c->W.get(w.data(), w.size(), c->stream));
  FASST_TRY(c->Ht.get(ht.data(), ht.size(), c->stream));
  FASST_TRY(c->beta.get(b.data(), b.size(), c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  if (WM)
    for (int f = 0; f < F; ++f)
      for (int r = 0; r < R; ++r) WM[(size_t)f * R + r] = w[(size_t)f * Rp + r];
  if (HM)
    for (int r = 0; r < R; ++r)
      for (int n = 0; n < N; ++n) HM[(size_t)r * N + n] = ht[(size_t)n * Rp + r];
  for (int r = 0; r < R; ++r) {
    if (betaR) betaR[r] = b[r];
    if (betaL) betaL[r] = b[Rp + r];
  }
  return FASST_OK;
}

}  // extern "C"
