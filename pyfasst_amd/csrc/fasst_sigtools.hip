// Signal tools on MI355X (gfx950), FP64: tools/signalTools.py of the reference.
//
//   k_pca2d         prinComp2D (:26-118): one block per (bin, chunk of 256
//                   windows); |x0|^2, |x1|^2 and x0 conj(x1) of the chunk plus
//                   its neighbor_nb - 1 halo frames are staged once in LDS as
//                   four planes, each thread sums its own window in ascending
//                   frame order (no running window: its rounding would depend
//                   on the chunking) and evaluates the closed form.
//   k_median        medianFilter (:13-24): one thread per output sample, the
//                   chunk's span staged in LDS; selection by rank counting,
//                   ties broken by index, so any window length works (a span
//                   beyond the LDS budget is read from global memory).
//   k_hsum_colsum,  f0detectionFunction (:198-318): one block per (F0, tile of
//   k_hsum          256 frames), frames along the fast axis; the harmonic bins
//                   come as a CSR list whose entries are block-uniform loads.
//   k_invherm_elem  invHermMat2D (:120-131).
//
// All four are bandwidth- or latency-bound; none has a matrix product in it.
// The expressions follow NumPy's operation order with contraction off, and
// np.abs of a complex number is NumPy's own loop (np_cabs, fasst_device.h),
// which is what makes the median and the 2x2 inverse bit-equal to the reference.
#include "fasst_device.h"
#include "../../include/fasst_sigtools.h"

#include <atomic>
#include <climits>
#include <vector>

namespace fasst {

static std::atomic<long> g_sig_launches{0};

// ---------------------------------------------------------------- prinComp2D
constexpr int kPcaChunk = 256;

struct PcaArgs {
  const double2 *x0, *x1;  // [F][N]
  double *lM, *lm;         // [F][L]
  double2 *vM, *vm;        // [2][F][L]
  int *flags;              // [2]
  int F, N, nb, L, nchunks;
};

__global__ __launch_bounds__(kPcaChunk) void k_pca2d(const PcaArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int S = kPcaChunk + a.nb - 1;
  double *p0 = sm, *p1 = sm + S, *cr = sm + 2 * S, *ci = sm + 3 * S;
  const int f = blockIdx.x / a.nchunks;
  const int l0 = (blockIdx.x % a.nchunks) * kPcaChunk;
  const int nl = min(kPcaChunk, a.L - l0);
  const int span = nl + a.nb - 1;  // frames l0 .. l0 + span - 1 <= N - 1
  const double2 *r0 = a.x0 + (size_t)f * a.N + l0, *r1 = a.x1 + (size_t)f * a.N + l0;
  for (int i = threadIdx.x; i < span; i += kPcaChunk) {
    const double2 u = r0[i], v = r1[i];
    const double m0 = np_cabs(u.x, u.y), m1 = np_cabs(v.x, v.y);
    p0[i] = m0 * m0;
    p1[i] = m1 * m1;
    cr[i] = u.x * v.x + u.y * v.y;  // x0 * conj(x1)
    ci[i] = u.y * v.x - u.x * v.y;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= nl) return;
  double s0 = 0.0, s1 = 0.0, sr = 0.0, si = 0.0;
  for (int k = 0; k < a.nb; ++k) {
    s0 += p0[t + k];
    s1 += p1[t + k];
    sr += cr[t + k];
    si += ci[t + k];
  }
  const double nm1 = (double)a.nb - 1.0;
  const double c0 = fabs(s0) / nm1, c1 = fabs(s1) / nm1;
  // complex / real in NumPy: multiply by the reciprocal
  const double inv = 1.0 / nm1;
  const double er = sr * inv, ei = si * inv;
  const double m01 = np_cabs(er, ei), a01 = m01 * m01;
  const double tra = c0 + c1;
  const double det = c0 * c1 - a01;
  const double delta = sqrt(tra * tra - 4.0 * det);
  const double lM = 0.5 * (tra + delta), lm = 0.5 * (tra - delta);
  if (lM < 0.0) atomicOr(a.flags, 1);
  if (lm < 0.0) atomicOr(a.flags + 1, 1);
  const size_t o = (size_t)f * a.L + l0 + t, plane = (size_t)a.F * a.L;
  a.lM[o] = lM;
  a.lm[o] = lm;
  {
    const double d = lM - c0;
    const double den = sqrt(a01 + d * d);
    if (den == 0.0) {
      a.vM[o] = make_double2(1.0, 0.0);
      a.vM[plane + o] = make_double2(0.0, 0.0);
    } else {
      const double scl = 1.0 / den;
      a.vM[o] = make_double2(er * scl, ei * scl);
      a.vM[plane + o] = make_double2(d / den, 0.0);
    }
  }
  {
    const double d = lm - c0;
    const double den = sqrt(a01 + d * d);
    if (den == 0.0) {
      a.vm[o] = make_double2(0.0, 0.0);
      a.vm[plane + o] = make_double2(1.0, 0.0);
    } else {
      const double scl = 1.0 / den;
      a.vm[o] = make_double2(er * scl, ei * scl);
      a.vm[plane + o] = make_double2(d / den, 0.0);
    }
  }
}

// -------------------------------------------------------------- medianFilter
constexpr int kMedChunk = 128;  // (kMedLdsSpan, fasst_device.h: a wider span stays in global memory)

struct MedArgs {
  const double *in;  // [R][N]
  double *out;
  int R, N, length, nchunks;
};

template <bool kStaged>
__global__ __launch_bounds__(kMedChunk) void k_median(const MedArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double sm[];  // [kMedChunk + 2 length] if staged
  const int r = blockIdx.x / a.nchunks;
  const int c0 = (blockIdx.x % a.nchunks) * kMedChunk;
  const double *row = a.in + (size_t)r * a.N;
  // the samples any window of this chunk can hold: [s_lo, s_hi), s_hi <= N - 1
  const int s_lo = max(c0 - a.length, 0);
  const int s_hi = (int)min((long)c0 + kMedChunk - 1 + a.length, (long)a.N - 1);
  if (kStaged) {
    for (int i = s_lo + (int)threadIdx.x; i < s_hi; i += kMedChunk) sm[i - s_lo] = row[i];
    __syncthreads();
  }
  const double *src = kStaged ? sm - s_lo : row;
  const int n = c0 + threadIdx.x;
  if (n >= a.N) return;
  a.out[(size_t)r * a.N + n] = median_at(src, row[n], n, a.length, a.N);
}

// ------------------------------------------------------- f0detectionFunction
constexpr int kHsTile = 256, kHsSumBlock = 64;

struct HsArgs {
  const double *tf;  // [F][T]
  const double *w;   // [F]
  const int *ptr;    // [n_f0 * n_harm + 1]
  const int *idx;    // [nnz]
  double *colsum;    // [T]
  double *hs;        // [n_f0][T]
  int F, T, n_f0, n_harm, nnz, ntiles, prod;
};

// TFmatrix.sum(axis=0): each frame's bins in ascending order
__global__ __launch_bounds__(kHsSumBlock) void k_hsum_colsum(const HsArgs a) {
  const int t = blockIdx.x * kHsSumBlock + threadIdx.x;
  if (t >= a.T) return;
  double s = 0.0;
  const double *p = a.tf + t;
#pragma unroll 8
  for (int f = 0; f < a.F; ++f) s += p[(size_t)f * a.T];
  a.colsum[t] = s;
}

__global__ __launch_bounds__(kHsTile) void k_hsum(const HsArgs a) {
#pragma clang fp contract(off)
  const int i0 = blockIdx.x / a.ntiles;
  const int t = (blockIdx.x % a.ntiles) * kHsTile + threadIdx.x;
  if (t >= a.T) return;
  const double tot = a.colsum[t];
  const int *ptr = a.ptr + (size_t)i0 * a.n_harm;
  double acc = 0.0;
  bool any = false;
  for (int h = 0; h < a.n_harm; ++h) {
    const int b0 = max(ptr[h], 0), b1 = min(ptr[h + 1], a.nnz);
    double m = 0.0;
    bool have = false;
    for (int k = b0; k < b1; ++k) {
      const int b = a.idx[k];
      if ((unsigned)b >= (unsigned)a.F) continue;
      const double v = a.w[b] * a.tf[(size_t)b * a.T + t];
      m = (!have || v > m || v != v) ? v : m;  // np.max: a NaN wins
      have = true;
    }
    if (!have) continue;
    const double q = m / tot;
    acc = !any ? q : (a.prod ? acc * q : acc + q);
    any = true;
  }
  a.hs[(size_t)i0 * a.T + t] = acc;
}

// -------------------------------------------------------------- invHermMat2D
struct InvArgs {
  const double *a00, *a01, *a11;
  double *i00, *i01, *i11;
  int *nzero;
  long n;
  int off_complex;
};

__global__ __launch_bounds__(256) void k_invherm_elem(const InvArgs a) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const double d0 = a.a00[i], d1 = a.a11[i];
  if (a.off_complex) {
    const double re = a.a01[2 * i], im = a.a01[2 * i + 1];
    const double m = np_cabs(re, im);
    const double det = d0 * d1 - m * m;
    if (det == 0.0) atomicAdd(a.nzero, 1);
    a.i00[i] = d1 / det;
    a.i11[i] = d0 / det;
    // NumPy's complex division by (det, 0)
    const double nr = -re, ni = -im;
    if (det == 0.0) {
      a.i01[2 * i] = nr / 0.0;
      a.i01[2 * i + 1] = ni / 0.0;
    } else {
      const double rat = 0.0 / det;
      const double scl = 1.0 / (det + 0.0 * rat);
      a.i01[2 * i] = (nr + ni * rat) * scl;
      a.i01[2 * i + 1] = (ni - nr * rat) * scl;
    }
  } else {
    const double o = a.a01[i];
    const double m = fabs(o);
    const double det = d0 * d1 - m * m;
    if (det == 0.0) atomicAdd(a.nzero, 1);
    a.i00[i] = d1 / det;
    a.i01[i] = -o / det;
    a.i11[i] = d0 / det;
  }
}

// ----------------------------------------------------------------- host side
static float g_sig_ms = 0.f;

// tm: the HIP events around the kernels of one call (sig_last_ms)
static int finish_launch(int n_kernels, Events &tm) {
  FASST_LAUNCH_CHECK();
  g_sig_launches += n_kernels;
  int st = elapsed_ms(tm.e[0], tm.e[1], 0, &g_sig_ms);
  if (st) return st;
  FASST_HIP(hipDeviceSynchronize());
  return FASST_OK;
}

static bool pca_shape_ok(int F, int N, int nb) {
  if (F < 1 || N < 1 || nb < 1 || nb > N) {
    set_error("sig_pca2d: bad shape (F %d, N %d, neighbor_nb %d: 1 <= neighbor_nb <= N)", F, N,
              nb);
    return false;
  }
  const long nchunks = ((long)N - nb + 1 + kPcaChunk - 1) / kPcaChunk;
  if (nchunks * F > INT_MAX) {
    set_error("sig_pca2d: %d bins x %d frames exceed the grid", F, N);
    return false;
  }
  return true;
}

}  // namespace fasst

using namespace fasst;

extern "C" {

int sig_last_ms(double *device_ms) {
  if (device_ms) *device_ms = g_sig_ms;
  return FASST_OK;
}

int sig_launch_count(long *count) {
  if (count) *count = g_sig_launches.load();
  return FASST_OK;
}

int sig_pca2d_dev(int device, int F, int N, int nb, const double *x0, const double *x1,
                  double *lambda_M, double *lambda_m, double *v_M, double *v_m, int *flags) {
  if (!pca_shape_ok(F, N, nb)) return FASST_ERR_SHAPE;
  if (!x0 || !x1 || !lambda_M || !lambda_m || !v_M || !v_m || !flags) {
    set_error("sig_pca2d: null argument");
    return FASST_ERR_SHAPE;
  }
  if (nb > SIG_PCA_MAX_NEIGHBORS) {
    set_error("sig_pca2d: neighbor_nb %d > %d (the chunk and its halo are staged in LDS)", nb,
              SIG_PCA_MAX_NEIGHBORS);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(device);
  int st;
  DBuf<int> dflags;
  if ((st = dflags.alloc(2))) return st;
  PcaArgs a;
  a.x0 = (const double2 *)x0;
  a.x1 = (const double2 *)x1;
  a.lM = lambda_M;
  a.lm = lambda_m;
  a.vM = (double2 *)v_M;
  a.vm = (double2 *)v_m;
  a.flags = dflags.p;
  a.F = F;
  a.N = N;
  a.nb = nb;
  a.L = N - nb + 1;
  a.nchunks = (a.L + kPcaChunk - 1) / kPcaChunk;
  const size_t smem = (size_t)4 * (kPcaChunk + nb - 1) * sizeof(double);
  if (smem > 64 * 1024)
    FASST_HIP(hipFuncSetAttribute((const void *)k_pca2d,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  Events tm;
  if ((st = tm.start(0))) return st;
  k_pca2d<<<a.nchunks * F, kPcaChunk, smem>>>(a);
  if ((st = finish_launch(1, tm))) return st;
  return dflags.get(flags, 2);
}

int sig_pca2d(int device, int F, int N, int nb, const double *x0, const double *x1,
              double *lambda_M, double *lambda_m, double *v_M, double *v_m, int *flags) {
  if (!pca_shape_ok(F, N, nb)) return FASST_ERR_SHAPE;
  if (!x0 || !x1 || !lambda_M || !lambda_m || !v_M || !v_m || !flags) {
    set_error("sig_pca2d: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  int st;
  const size_t nin = (size_t)2 * F * N, nl = (size_t)F * (N - nb + 1);
  DBuf<double> d0, d1, dM, dm, dvM, dvm;
  if ((st = d0.upload(x0, nin)) || (st = d1.upload(x1, nin)) || (st = dM.alloc_uninit(nl)) ||
      (st = dm.alloc_uninit(nl)) || (st = dvM.alloc_uninit(4 * nl)) ||
      (st = dvm.alloc_uninit(4 * nl)))
    return st;
  if ((st = sig_pca2d_dev(device, F, N, nb, d0.p, d1.p, dM.p, dm.p, dvM.p, dvm.p, flags)))
    return st;
  if ((st = dM.get(lambda_M, nl)) || (st = dm.get(lambda_m, nl)) || (st = dvM.get(v_M, 4 * nl)))
    return st;
  return dvm.get(v_m, 4 * nl);
}

static bool median_shape_ok(int R, int N, int length, const double *in, const double *out) {
  if (R < 1 || N < 1 || length < 0 || !in || !out) {
    set_error("sig_median: bad shape (R %d, N %d, length %d >= 0)", R, N, length);
    return false;
  }
  const long nchunks = ((long)N + kMedChunk - 1) / kMedChunk;
  if (nchunks * R > INT_MAX) {
    set_error("sig_median: %d rows x %d samples exceed the grid", R, N);
    return false;
  }
  return true;
}

int sig_median_dev(int device, int R, int N, int length, const double *in, double *out) {
  if (!median_shape_ok(R, N, length, in, out)) return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  MedArgs a;
  a.in = in;
  a.out = out;
  a.R = R;
  a.N = N;
  a.length = length < N ? length : N;  // the same windows, and n + length stays an int
  a.nchunks = (N + kMedChunk - 1) / kMedChunk;
  Events tm;
  if ((st = tm.start(0))) return st;
  if ((long)kMedChunk + 2L * a.length <= kMedLdsSpan)
    k_median<true><<<a.nchunks * R, kMedChunk, (kMedChunk + 2 * (size_t)a.length) * sizeof(double)>>>(a);
  else
    k_median<false><<<a.nchunks * R, kMedChunk>>>(a);
  return finish_launch(1, tm);
}

int sig_median(int device, int R, int N, int length, const double *in, double *out) {
  if (!median_shape_ok(R, N, length, in, out)) return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  const size_t n = (size_t)R * N;
  DBuf<double> din, dout;
  if ((st = din.upload(in, n)) || (st = dout.alloc_uninit(n))) return st;
  if ((st = sig_median_dev(device, R, N, length, din.p, dout.p))) return st;
  return dout.get(out, n);
}

static bool hsum_shape_ok(int F, int T, int n_f0, int n_harm, const void *tf, const void *w,
                          const void *ptr, const void *idx, long nnz, const void *hs) {
  if (F < 1 || T < 1 || n_f0 < 1 || n_harm < 1 || nnz < 0 || !tf || !w || !ptr || !hs ||
      (nnz > 0 && !idx)) {
    set_error("sig_hsum: bad shape (F %d, T %d, n_f0 %d, n_harm %d, nnz %ld)", F, T, n_f0, n_harm,
              nnz);
    return false;
  }
  const long ntiles = ((long)T + kHsTile - 1) / kHsTile;
  if (ntiles * n_f0 > INT_MAX || (long)n_f0 * n_harm + 1 > INT_MAX) {
    set_error("sig_hsum: %d F0s x %d frames x %d harmonics exceed the grid", n_f0, T, n_harm);
    return false;
  }
  return true;
}

int sig_hsum_dev(int device, int F, int T, int n_f0, int n_harm, const double *tf,
                 const double *weights, const int *bin_ptr, const int *bin_idx, int nnz, int prod,
                 double *hs) {
  if (!hsum_shape_ok(F, T, n_f0, n_harm, tf, weights, bin_ptr, bin_idx, nnz, hs))
    return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  DBuf<double> dsum;
  if ((st = dsum.alloc_uninit(T))) return st;
  HsArgs a;
  a.tf = tf;
  a.w = weights;
  a.ptr = bin_ptr;
  a.idx = bin_idx;
  a.colsum = dsum.p;
  a.hs = hs;
  a.F = F;
  a.T = T;
  a.n_f0 = n_f0;
  a.n_harm = n_harm;
  a.nnz = nnz;
  a.ntiles = (T + kHsTile - 1) / kHsTile;
  a.prod = prod != 0;
  Events tm;
  if ((st = tm.start(0))) return st;
  k_hsum_colsum<<<(T + kHsSumBlock - 1) / kHsSumBlock, kHsSumBlock>>>(a);
  k_hsum<<<a.ntiles * n_f0, kHsTile>>>(a);
  return finish_launch(2, tm);
}

int sig_hsum(int device, int F, int T, int n_f0, int n_harm, const double *tf,
             const double *weights, const int *bin_ptr, const int *bin_idx, int prod, double *hs) {
  if (!bin_ptr) {
    set_error("sig_hsum: null bin_ptr");
    return FASST_ERR_SHAPE;
  }
  if (n_f0 < 1 || n_harm < 1 || (long)n_f0 * n_harm + 1 > INT_MAX) {
    set_error("sig_hsum: bad shape (n_f0 %d, n_harm %d)", n_f0, n_harm);
    return FASST_ERR_SHAPE;
  }
  const size_t np = (size_t)n_f0 * n_harm + 1;
  const int nnz = bin_ptr[np - 1];
  if (!hsum_shape_ok(F, T, n_f0, n_harm, tf, weights, bin_ptr, bin_idx, nnz, hs))
    return FASST_ERR_SHAPE;
  if (bin_ptr[0] != 0) {
    set_error("sig_hsum: bin_ptr[0] = %d, not 0", bin_ptr[0]);
    return FASST_ERR_SHAPE;
  }
  for (size_t i = 1; i < np; ++i)
    if (bin_ptr[i] < bin_ptr[i - 1]) {
      set_error("sig_hsum: bin_ptr decreases at %zu", i);
      return FASST_ERR_SHAPE;
    }
  for (int k = 0; k < nnz; ++k)
    if (bin_idx[k] < 0 || bin_idx[k] >= F) {
      set_error("sig_hsum: bin_idx[%d] = %d outside [0, %d)", k, bin_idx[k], F);
      return FASST_ERR_SHAPE;
    }
  DeviceGuard g(device);
  int st;
  DBuf<double> dtf, dw, dhs;
  DBuf<int> dptr_, didx;
  const size_t nout = (size_t)n_f0 * T;
  if ((st = dtf.upload(tf, (size_t)F * T)) || (st = dw.upload(weights, (size_t)F)) ||
      (st = dptr_.upload(bin_ptr, np)) || (st = didx.upload(bin_idx, (size_t)nnz)) ||
      (st = dhs.alloc_uninit(nout)))
    return st;
  if ((st = sig_hsum_dev(device, F, T, n_f0, n_harm, dtf.p, dw.p, dptr_.p, didx.p, nnz, prod,
                         dhs.p)))
    return st;
  return dhs.get(hs, nout);
}

static bool invherm_shape_ok(long n, const void *a00, const void *a01, const void *a11,
                             const void *i00, const void *i01, const void *i11,
                             const void *nzero) {
  if (n < 1 || (n + 255) / 256 > INT_MAX || !a00 || !a01 || !a11 || !i00 || !i01 || !i11 ||
      !nzero) {
    set_error("sig_invherm: bad shape (n %ld) or null argument", n);
    return false;
  }
  return true;
}

int sig_invherm_dev(int device, long n, int off_complex, const double *a00, const double *a01,
                    const double *a11, double *i00, double *i01, double *i11, int *n_zero_det) {
  if (!invherm_shape_ok(n, a00, a01, a11, i00, i01, i11, n_zero_det)) return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  DBuf<int> dz;
  if ((st = dz.alloc(1))) return st;
  InvArgs a;
  a.a00 = a00;
  a.a01 = a01;
  a.a11 = a11;
  a.i00 = i00;
  a.i01 = i01;
  a.i11 = i11;
  a.nzero = dz.p;
  a.n = n;
  a.off_complex = off_complex != 0;
  Events tm;
  if ((st = tm.start(0))) return st;
  k_invherm_elem<<<(int)((n + 255) / 256), 256>>>(a);
  if ((st = finish_launch(1, tm))) return st;
  return dz.get(n_zero_det, 1);
}

int sig_invherm(int device, long n, int off_complex, const double *a00, const double *a01,
                const double *a11, double *i00, double *i01, double *i11, int *n_zero_det) {
  if (!invherm_shape_ok(n, a00, a01, a11, i00, i01, i11, n_zero_det)) return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  const size_t m = (size_t)n, mo = off_complex ? 2 * m : m;
  DBuf<double> d00, d01, d11, o00, o01, o11;
  if ((st = d00.upload(a00, m)) || (st = d01.upload(a01, mo)) || (st = d11.upload(a11, m)) ||
      (st = o00.alloc_uninit(m)) || (st = o01.alloc_uninit(mo)) || (st = o11.alloc_uninit(m)))
    return st;
  if ((st = sig_invherm_dev(device, n, off_complex, d00.p, d01.p, d11.p, o00.p, o01.p, o11.p,
                            n_zero_det)))
    return st;
  if ((st = o00.get(i00, m)) || (st = o01.get(i01, mo))) return st;
  return o11.get(i11, m);
}

}  // extern "C"
