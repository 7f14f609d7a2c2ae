// Source / filter Itakura-Saito NMF on MI355X (gfx950), FP64.
//
// Restates tools/nmf.py SFNMF_decomp_init (:161-360):
//   SX ~ hat = SF0 * SPHI + Sres,  SF0 = W H, SPHI = WFilt HFilt, Sres = Wres Hres
// One iteration updates W, H, WFilt, HFilt (each behind its switch), then
// Wres and Hres (always).  Every update is
//   X = SX other / max(hat^2, eps), Y = other / max(hat, eps)   (k_sfnmf_ratio)
//   num, den = the contraction of X, Y with the update's partner factor
//   factor *= num / max(den, eps)
// with other = SPHI (W, H), SF0 (WFilt, HFilt), 1 (Wres, Hres); a W-type update
// is followed by its column normalisation (scale moved into the partner H), the
// HFilt update by its per-frame normalisation (sum moved into H BEFORE the zero
// guard, nmf.py:316-319).
//
// The three factor pairs share one code path (SfFactor).  A pair narrower than
// kSfWide runs its product and contractions on gemm<> (fasst_gemm.h), as the
// IS-NMF engine's unfused path does; a wider one (the F0 dictionary, K = 1093)
// on dgemm2, which wants both operands major in the contracted index: it keeps
// transposed copies WT [K][pF] and Ht [N][pK], refreshed when stale, and its
// W-type ratio pass writes the transposed planes [N][X | Y].  Leading
// dimensions are padded to even (16-byte rows for dgemm2's row loads).
//
// A product plane is formed again only after one of its factors was written
// (`valid`); the reference recomputes all three before each update, from the
// same factors, so the values are the same.  All reductions run in a fixed
// order: two runs are bit-equal.
#include "fasst_gemm.h"

#include <algorithm>

#include "../../include/fasst_nmf.h"

namespace fasst {

constexpr double kSfNmfEps = 1e-10;  // tools/nmf.py:22
constexpr int kSfWide = 128;         // components from which a pair runs on dgemm2
enum { kSfOtherPhi = 0, kSfOtherF0 = 1, kSfOtherOne = 2 };

// One pass over F x N: X = SX o / max(hat^2, eps), Y = o / max(hat, eps) with
// hat = SF0 SPHI + Sres (product and sum rounded separately, as NumPy does)
// and o = SPHI, SF0 or 1.  Planes are [F][pN].  TR = false: out[f][n] = X,
// out[f][yoff + n] = Y (row pitch ldo); TR = true: out[n][f], out[n][yoff + f]
// through a 32 x 32 LDS tile.  Block 256 = 32 x 8, four rows per thread.
template <bool TR>
__global__ __launch_bounds__(256) void k_sfnmf_ratio(const double *__restrict__ SX,
                                                     const double *__restrict__ SF0,
                                                     const double *__restrict__ SPHI,
                                                     const double *__restrict__ Sres,
                                                     double *__restrict__ out, int F, int N, int pN,
                                                     int ldo, int yoff, int other) {
  __shared__ double sx[TR ? 32 : 1][33], sy[TR ? 32 : 1][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int n0 = blockIdx.x * 32;
  for (int f0 = blockIdx.y * 32; f0 < F; f0 += gridDim.y * 32) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int fl = ty + 8 * r, f = f0 + fl, n = n0 + tx;
      double x = 0.0, y = 0.0;
      if (f < F && n < N) {
        const size_t i = (size_t)f * pN + n;
        const double a = SF0[i], b = SPHI[i];
        const double hat = __dadd_rn(__dmul_rn(a, b), Sres[i]);
        const double o = other == kSfOtherPhi ? b : (other == kSfOtherF0 ? a : 1.0);
        x = __dmul_rn(SX[i], o) / fmax(__dmul_rn(hat, hat), kSfNmfEps);
        y = o / fmax(hat, kSfNmfEps);
        if constexpr (!TR) {
          out[(size_t)f * ldo + n] = x;
          out[(size_t)f * ldo + yoff + n] = y;
        }
      }
      if constexpr (TR) {
        sx[fl][tx] = x;
        sy[fl][tx] = y;
      }
    }
    if constexpr (TR) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nl = ty + 8 * r, n = n0 + nl, f = f0 + tx;
        if (f < F && n < N) {
          out[(size_t)n * ldo + f] = sx[tx][nl];
          out[(size_t)n * ldo + yoff + f] = sy[tx][nl];
        }
      }
      __syncthreads();
    }
  }
}

// W-type update of one column k per block (nmf.py:244-248, as k_nmf_w):
// W[:, k] *= num / max(den, eps); s = sum(W[:, k]), s == 0 -> 1; W[:, k] /= s;
// s_out[k] = s.  W [F][ldw]; num / den [K][ldn] (component-major).
__global__ __launch_bounds__(256) void k_sfnmf_wcol(double *__restrict__ W, int ldw,
                                                    const double *__restrict__ numT,
                                                    const double *__restrict__ denT, int ldn,
                                                    double *__restrict__ s_out, int F) {
  __shared__ double s_red[256];
  const int k = blockIdx.x;
  double part = 0.0;
  for (int f = threadIdx.x; f < F; f += 256) {
    const size_t o = (size_t)k * ldn + f;
    const double w = W[(size_t)f * ldw + k] * (numT[o] / fmax(denT[o], kSfNmfEps));
    W[(size_t)f * ldw + k] = w;
    part += w;
  }
  s_red[threadIdx.x] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
    __syncthreads();
  }
  double s = s_red[0];
  if (s == 0) s = 1.0;  // sumW[sumW==0] = 1. (nmf.py:247)
  for (int f = threadIdx.x; f < F; f += 256) W[(size_t)f * ldw + k] /= s;
  if (threadIdx.x == 0) s_out[k] = s;
}

// H[k][:] *= s[k]  (H [K][ldh])
__global__ void k_sfnmf_hscale(double *__restrict__ H, int ldh, const double *__restrict__ s,
                               int K, int N) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)K * N;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t k = i / N;
    H[k * ldh + (i - k * N)] *= s[k];
  }
}

// H *= num / max(den, eps)  (H [K][ldh], num / den [K][ldn])
__global__ void k_sfnmf_hupd(double *__restrict__ H, int ldh, const double *__restrict__ num,
                             const double *__restrict__ den, int ldn, int K, int N) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)K * N;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t k = i / N, n = i - k * N;
    H[k * ldh + n] *= num[k * ldn + n] / fmax(den[k * ldn + n], kSfNmfEps);
  }
}

// sumH[n] = sum_k HFilt[k][n], components in index order (nmf.py:316)
__global__ void k_sfnmf_framesum(const double *__restrict__ HF, int ldh, int Kf, int N,
                                 double *__restrict__ sum) {
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < (size_t)N;
       n += (size_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < Kf; ++k) s += HF[(size_t)k * ldh + n];
    sum[n] = s;
  }
}

// nmf.py:317-319: H *= sumH (the raw sum: a frame of all-zero filter
// activations zeroes that frame of H), then sumH[sumH==0] = 1, HFilt /= sumH
__global__ void k_sfnmf_framenorm(double *__restrict__ H, double *__restrict__ HF, int ldh, int K,
                                  int Kf, int N, const double *__restrict__ sum) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)(K + Kf) * N;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / N, n = i - r * N;
    const double s = sum[n];
    if (r < (size_t)K)
      H[r * ldh + n] *= s;
    else
      HF[(r - K) * ldh + n] /= (s == 0 ? 1.0 : s);
  }
}

// out[c][r] = in[r][c] for an R x C matrix (row pitches ldi / ldo), 32 x 32 tiles
__global__ __launch_bounds__(256) void k_sfnmf_transpose(const double *__restrict__ in, int ldi,
                                                         double *__restrict__ out, int ldo, int R,
                                                         int C) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32;
  for (int r0 = blockIdx.y * 32; r0 < R; r0 += gridDim.y * 32) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + ty + 8 * q, c = c0 + tx;
      if (r < R && c < C) tile[ty + 8 * q][tx] = in[(size_t)r * ldi + c];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + ty + 8 * q, r = r0 + tx;
      if (r < R && c < C) out[(size_t)c * ldo + r] = tile[tx][ty + 8 * q];
    }
    __syncthreads();
  }
}

}  // namespace fasst

using namespace fasst;

namespace {

// one factor pair Wf [F][K], Hf [K][N] of the model
struct SfFactor {
  int K = 0, pK = 0;
  bool wide = false;
  DBuf<double> W, H, s;  // [F][pK], [K][pN], column sums [K]
  DBuf<double> WT, Ht;   // wide only: [K][pF], [N][pK]
  bool wt_ok = false, ht_ok = false;
};

}  // namespace

struct sfnmf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int F = 0, N = 0, pF = 0, pN = 0;
  SfFactor fac[3];       // source (W, H), filter (WFilt, HFilt), residual (Wres, Hres)
  DBuf<double> SX;       // [F][pN]
  DBuf<double> P[3];     // SF0, SPHI, Sres, [F][pN]
  bool valid[3] = {false, false, false};
  DBuf<double> xy;       // ratio planes: [F][X | Y] (pitch 2 pN) or [N][X | Y] (2 pF)
  DBuf<double> nd;       // contraction output: num and den, component-major
  DBuf<double> fsum;     // [N]
  DBuf<double> work;     // gemm<> split-K slabs
};

namespace {

dim3 tgrid(int cols, int rows) { return dim3((cols + 31) / 32, std::min((rows + 31) / 32, 65535)); }

int sf_transpose(sfnmf_ctx *c, const double *in, int ldi, double *out, int ldo, int R, int C) {
  k_sfnmf_transpose<<<tgrid(C, R), 256, 0, c->stream>>>(in, ldi, out, ldo, R, C);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// P[i] = Wf Hf, if a factor of it was written since it was last formed
int sf_product(sfnmf_ctx *c, int i) {
  if (c->valid[i]) return FASST_OK;
  SfFactor &f = c->fac[i];
  int st;
  if (f.wide) {
    if (!f.wt_ok) {
      if ((st = sf_transpose(c, f.W.p, f.pK, f.WT.p, c->pF, c->F, f.K))) return st;
      f.wt_ok = true;
    }
    st = dgemm2(c->stream, c->F, c->N, f.K, f.WT.p, c->pF, f.H.p, c->pN, c->P[i].p, c->pN);
  } else {
    // K < kSfWide: gemm_plan never splits this product, so the padded ldc holds
    const double *Bs[1] = {f.H.p};
    double *Cs[1] = {c->P[i].p};
    st = gemm<false, false, 1>(c->stream, f.W.p, f.pK, Bs, c->pN, Cs, c->pN, c->F, c->N, f.K,
                               nullptr);
  }
  if (st) return st;
  c->valid[i] = true;
  return FASST_OK;
}

// the ratio planes of an update of pair i; tr: the transposed form
int sf_ratio(sfnmf_ctx *c, int other, bool tr) {
  int st;
  for (int i = 0; i < 3; ++i)
    if ((st = sf_product(c, i))) return st;
  if (tr)
    k_sfnmf_ratio<true><<<tgrid(c->N, c->F), 256, 0, c->stream>>>(
        c->SX.p, c->P[0].p, c->P[1].p, c->P[2].p, c->xy.p, c->F, c->N, c->pN, 2 * c->pF, c->pF,
        other);
  else
    k_sfnmf_ratio<false><<<tgrid(c->N, c->F), 256, 0, c->stream>>>(
        c->SX.p, c->P[0].p, c->P[1].p, c->P[2].p, c->xy.p, c->F, c->N, c->pN, 2 * c->pN, c->pN,
        other);
  FASST_LAUNCH_CHECK();
  return FASST_OK;
}

// nmf.py:232-249 (W), :270-288 (WFilt), :329-344 (Wres)
int sf_w_update(sfnmf_ctx *c, int i, int other) {
  SfFactor &f = c->fac[i];
  const int F = c->F, N = c->N, K = f.K;
  int st;
  if ((st = sf_ratio(c, other, f.wide))) return st;
  const double *num, *den;
  int ldn;
  if (f.wide) {
    if (!f.ht_ok) {
      if ((st = sf_transpose(c, f.H.p, c->pN, f.Ht.p, f.pK, K, N))) return st;
      f.ht_ok = true;
    }
    // [numT | denT] [K][2 pF] = Ht^T [X^T | Y^T]
    if ((st = dgemm2(c->stream, K, 2 * c->pF, N, f.Ht.p, f.pK, c->xy.p, 2 * c->pF, c->nd.p,
                     2 * c->pF)))
      return st;
    num = c->nd.p;
    den = c->nd.p + c->pF;
    ldn = 2 * c->pF;
  } else {
    const double *Bs[2] = {c->xy.p, c->xy.p + c->pN};
    double *Cs[2] = {c->nd.p, c->nd.p + (size_t)K * F};
    if ((st = gemm<false, true, 2>(c->stream, f.H.p, c->pN, Bs, 2 * c->pN, Cs, F, K, F, N,
                                   c->work.p)))
      return st;
    num = Cs[0];
    den = Cs[1];
    ldn = F;
  }
  k_sfnmf_wcol<<<K, 256, 0, c->stream>>>(f.W.p, f.pK, num, den, ldn, f.s.p, F);
  k_sfnmf_hscale<<<egrid((size_t)K * N), 256, 0, c->stream>>>(f.H.p, c->pN, f.s.p, K, N);
  FASST_LAUNCH_CHECK();
  // the rescaling moves scale between the two factors: still a write
  c->valid[i] = false;
  f.wt_ok = f.ht_ok = false;
  return FASST_OK;
}

// nmf.py:251-263 (H), :294-313 (HFilt), :346-358 (Hres)
int sf_h_update(sfnmf_ctx *c, int i, int other) {
  SfFactor &f = c->fac[i];
  const int F = c->F, N = c->N, K = f.K;
  int st;
  if ((st = sf_ratio(c, other, false))) return st;
  const double *num, *den;
  int ldn;
  if (f.wide) {
    // [num | den] [K][2 pN] = W^T [X | Y]
    if ((st = dgemm2(c->stream, K, 2 * c->pN, F, f.W.p, f.pK, c->xy.p, 2 * c->pN, c->nd.p,
                     2 * c->pN)))
      return st;
    num = c->nd.p;
    den = c->nd.p + c->pN;
    ldn = 2 * c->pN;
  } else {
    const double *Bs[2] = {c->xy.p, c->xy.p + c->pN};
    double *Cs[2] = {c->nd.p, c->nd.p + (size_t)K * N};
    if ((st = gemm<true, false, 2>(c->stream, f.W.p, f.pK, Bs, 2 * c->pN, Cs, N, K, N, F,
                                   c->work.p)))
      return st;
    num = Cs[0];
    den = Cs[1];
    ldn = N;
  }
  k_sfnmf_hupd<<<egrid((size_t)K * N), 256, 0, c->stream>>>(f.H.p, c->pN, num, den, ldn, K, N);
  FASST_LAUNCH_CHECK();
  c->valid[i] = false;
  f.ht_ok = false;
  return FASST_OK;
}

// nmf.py:315-319
int sf_hfilt_norm(sfnmf_ctx *c) {
  SfFactor &s = c->fac[0], &f = c->fac[1];
  k_sfnmf_framesum<<<egrid(c->N), 256, 0, c->stream>>>(f.H.p, c->pN, f.K, c->N, c->fsum.p);
  k_sfnmf_framenorm<<<egrid((size_t)(s.K + f.K) * c->N), 256, 0, c->stream>>>(
      s.H.p, f.H.p, c->pN, s.K, f.K, c->N, c->fsum.p);
  FASST_LAUNCH_CHECK();
  c->valid[0] = c->valid[1] = false;
  s.ht_ok = f.ht_ok = false;
  return FASST_OK;
}

int sf_iteration(sfnmf_ctx *c, int uw, int uh, int uwf, int uhf) {
  int st;
  if (uw && (st = sf_w_update(c, 0, kSfOtherPhi))) return st;
  if (uh && (st = sf_h_update(c, 0, kSfOtherPhi))) return st;
  if (uwf && (st = sf_w_update(c, 1, kSfOtherF0))) return st;
  if (uhf) {
    if ((st = sf_h_update(c, 1, kSfOtherF0))) return st;
    if ((st = sf_hfilt_norm(c))) return st;
  }
  if ((st = sf_w_update(c, 2, kSfOtherOne))) return st;
  return sf_h_update(c, 2, kSfOtherOne);
}

int even(int x) { return x + (x & 1); }

}  // namespace

extern "C" {

int sfnmf_create(int device, int F, int N, int K, int Kf, int Kr, sfnmf_ctx **out) {
  // planes are indexed with 64-bit offsets; the doubled, padded pitches and
  // the kernels' row / column indices must stay inside int
  constexpr int kMaxDim = 1 << 29;
  if (!out || F < 1 || N < 1 || K < 1 || Kf < 1 || Kr < 1 || F > kMaxDim || N > kMaxDim ||
      K > kMaxDim || Kf > kMaxDim || Kr > kMaxDim) {
    set_error("sfnmf_create: bad sizes F=%d N=%d K=%d Kf=%d Kr=%d", F, N, K, Kf, Kr);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  sfnmf_ctx *c = new sfnmf_ctx();
  c->device = device;
  c->F = F;
  c->N = N;
  c->pF = even(F);
  c->pN = even(N);
  const int Ks[3] = {K, Kf, Kr};
  int st = FASST_OK;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) st = FASST_ERR_DEVICE;
  const size_t plane = (size_t)F * c->pN;
  size_t gw = 1, nd = 0;
  for (int i = 0; i < 3; ++i) {
    SfFactor &f = c->fac[i];
    f.K = Ks[i];
    f.pK = even(f.K);
    f.wide = f.K >= kSfWide;
    if (!st) st = f.W.alloc((size_t)F * f.pK);
    if (!st) st = f.H.alloc((size_t)f.K * c->pN);
    if (!st) st = f.s.alloc(f.K);
    if (f.wide) {
      if (!st) st = f.WT.alloc((size_t)f.K * c->pF);
      if (!st) st = f.Ht.alloc((size_t)N * f.pK);
    } else {
      gw = std::max({gw, gemm_workspace(f.K, F, N, 2), gemm_workspace(f.K, N, F, 2)});
    }
    nd = std::max(nd, (size_t)f.K * 2 * std::max(c->pF, c->pN));
    if (!st) st = c->P[i].alloc(plane);
  }
  if (!st) st = c->SX.alloc(plane);
  // zero-filled: the pad columns are read by dgemm2 (into pad columns of nd)
  if (!st) st = c->xy.alloc(std::max((size_t)F * 2 * c->pN, (size_t)N * 2 * c->pF));
  if (!st) st = c->nd.alloc(nd);
  if (!st) st = c->fsum.alloc(N);
  if (!st) st = c->work.alloc(gw);
  if (st) {
    sfnmf_destroy(c);
    return st;
  }
  *out = c;
  return FASST_OK;
}

int sfnmf_destroy(sfnmf_ctx *c) {
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

int sfnmf_set_data(sfnmf_ctx *c, const double *SX) {
  if (!c || !SX) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  FASST_TRY(c->SX.at(0).put_rows(SX, c->F, c->N, c->N, c->pN, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int sfnmf_set_params(sfnmf_ctx *c, const double *W, const double *H, const double *WFilt,
                     const double *HFilt, const double *Wres, const double *Hres) {
  if (!c || !W || !H || !WFilt || !HFilt || !Wres || !Hres) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const double *Ws[3] = {W, WFilt, Wres}, *Hs[3] = {H, HFilt, Hres};
  for (int i = 0; i < 3; ++i) {
    SfFactor &f = c->fac[i];
    FASST_TRY(f.W.at(0).put_rows(Ws[i], c->F, f.K, f.K, f.pK, c->stream));
    FASST_TRY(f.H.at(0).put_rows(Hs[i], f.K, c->N, c->N, c->pN, c->stream));
    f.wt_ok = f.ht_ok = false;
    c->valid[i] = false;
  }
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int sfnmf_run(sfnmf_ctx *c, int n_iter, int update_w, int update_h, int update_wfilt,
              int update_hfilt) {
  if (!c || n_iter < 0) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  for (int it = 0; it < n_iter; ++it) {
    int st = sf_iteration(c, update_w, update_h, update_wfilt, update_hfilt);
    if (st) return st;
  }
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int sfnmf_get_params(sfnmf_ctx *c, double *W, double *H, double *WFilt, double *HFilt,
                     double *Wres, double *Hres) {
  if (!c) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  double *Ws[3] = {W, WFilt, Wres}, *Hs[3] = {H, HFilt, Hres};
  for (int i = 0; i < 3; ++i) {
    SfFactor &f = c->fac[i];
    if (Ws[i]) FASST_TRY(f.W.at(0).get_rows(Ws[i], c->F, f.K, f.K, f.pK, c->stream));
    if (Hs[i]) FASST_TRY(f.H.at(0).get_rows(Hs[i], f.K, c->N, c->N, c->pN, c->stream));
  }
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

}  // extern "C"
