// The mixing phase of the GEM iteration (update_mix_matrix, audioModel.py
// :766-889; retrieve_subsrc_params :570-574):
//   k_inst_A     per-bin mixing matrix from the 'inst' parameters (build_inst_A,
//                ahead of the E-step)
//   k_mix        one wave per bin: hat_Rss / hat_Rxs from the E-step's
//                sufficient statistics, the 'conv' per-bin solve
//   k_mix_inst   the 'inst' f-mean solve
// Interface: fasst_em.h (build_inst_A: fasst_ctx.h).

#include "fasst_em.h"
#include "fasst_device.h"

namespace fasst {

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

// the dynamic-LDS ceiling of k_mix's R > 16 arm, the one launch_mix may pass
// the 64 KB default with: raised once per model configuration to the most
// mix_smem asks for
int mix_lds_limits() {
  constexpr int nacc = 4 * (kMaxJ * (kMaxJ + 1) / 2) + 8 * kMaxJ;
  const size_t bytes = mix_smem(kMaxJ, kMaxR, kMaxKP, nacc);
  if (hipFuncSetAttribute((const void *)k_mix<(nacc + 63) / 64, (kMaxR * kMaxR + 63) / 64>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", bytes);
    return FASST_ERR_DEVICE;
  }
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

// update_mix_matrix (audioModel.py:766-889) on stream s: k_mix (per-bin
// statistics, hat_Rss / hat_Rxs, the 'conv' solves) and k_mix_inst (the
// 'inst' f-mean solve), when some spatial component is free
int launch_mix(fasst_ctx *c, hipStream_t s) {
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

}  // namespace fasst
