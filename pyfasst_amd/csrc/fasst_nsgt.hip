// The non-stationary Gabor transform on MI355X (gfx950), FP64: the reference's
// tftransforms/nsgt/nsgtf.py and nsigtf.py on a whole signal and, sliced,
// slicq.py (include/fasst_nsgt.h), on an FFT of any length.
//
//   k_small     one transform per block, all in LDS: a power-of-two FFT of up
//               to 4096 points, or Bluestein's convolution of padded size
//               P <= 4096 (chirp, FFT, product with the chirp's spectrum,
//               inverse FFT, chirp).  The operand is a plain array or, for the
//               forward band stage, the windowed and folded spectrum gathered
//               on the fly.
//   k_cols,     the four-step FFT of P = N1 N2 > 4096 points.  k_cols takes a
//   k_rows      tile of C adjacent columns (C N1 <= 4096) through LDS, so its
//               HBM accesses are runs of C elements, and carries the twiddle
//               exp(-2 pi i r c / P) on its load or its store; k_rows takes R
//               whole rows (R N2 <= 4096).  cols then rows leaves the spectrum
//               in [k1][k2] order (element k1 + N1 k2 at k1 N2 + k2); rows then
//               cols reads that order and returns natural order, so Bluestein's
//               convolution never transposes.  A natural-order power-of-two
//               FFT stores its rows transposed, in runs of R.
//   k_bfill     b[p] = conj(chirp) wrapped to P, whose FFT is tabulated once.
//   k_ola       the inverse's overlap-add as a gather: each spectrum bin sums
//               the bands that cover it in ascending band order from a
//               host-built cover table (no atomics), forming mirrored bands
//               as conjugate reversals on the fly.
//   k_slice,    the sliced transform (slicing.py, unslicing.py): k_slice cuts
//   k_unslice   quarter-blocks of a stream into Tukey-windowed slices in the
//               rotated quarter order, one pass; the plan's forward / backward
//               then run with every slice as one more channel; k_unslice
//               gathers the at most two slice quarters over each output sample,
//               older slice first, the previous call's last slice through a
//               carry buffer (no atomics).  arrange()'s per-slice rotation of
//               each band by M/4 or 3M/4 is a factor i^(r m) on the operand of
//               the band's length-M transform: band_fold and k_ola apply it
//               as a sign flip and a re/im swap (rot_nch = 0: none).
//
// Inverse transforms are conj . forward . conj on the loads and stores, so only
// forward twiddles exist.  Each pass reads and writes its array once: the
// engine is bound by HBM.
#include "fasst_common.h"
#include "fasst_fft.h"
#include "../../include/fasst_nsgt.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>

namespace fasst {
namespace {

constexpr int kLdsN = 4096;       // complex points of one block's LDS
constexpr int kMaxP = 1 << 24;    // largest power-of-two FFT
constexpr int kSmallLoP = 512;    // the in-LDS band batches split here (8 KB of LDS)
constexpr int kSmallGroups = 2;

std::atomic<long> g_launches{0};
thread_local int t_timing = 0;
thread_local double t_ms[2] = {0.0, 0.0};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ int brev(int i, int logN) { return logN ? bitrev(i, logN) : 0; }

// One transform of a batch.  Offsets are in elements of the array they index.
struct Job {
  long long in_off, out_off;   // operand and result (per channel: + ch * stride)
  long long ch_off, bh_off;    // chirp [n] and its spectrum [P] (Bluestein)
  long long g_off;             // window (the gather mode)
  int n, n_in, n_out;          // length; operand valid below n_in; stored below n_out
  int P, logP;                 // k_small: the block's FFT size
  int Lg, start, col;          // the gather mode: window length, first bin, fold
  double scale;
};

// v i^k
__device__ __forceinline__ double2 quarter_turns(double2 v, int k) {
  k &= 3;
  if (k == 1) return make_double2(-v.y, v.x);
  if (k == 2) return make_double2(-v.x, -v.y);
  if (k == 3) return make_double2(v.y, -v.x);
  return v;
}

// Quarter turns per index of a band of slice (rot_first + ch / rot_nch):
// `even` on even slices, 4 - even on odd ones; rot_nch = 0 (not sliced): none.
__device__ __forceinline__ int slice_turns(int rot_nch, int rot_first, int ch, int even) {
  if (!rot_nch) return 0;
  return ((rot_first + ch / rot_nch) & 1) ? 4 - even : even;
}

// temp of nsgtf.py:65-83 folded to M points: t[m] = sum_j temp[m col + j],
// temp[:(Lg+1)//2] = g[:(Lg+1)//2] ft[win[Lg//2:]], temp[-(Lg//2):] =
// g[-(Lg//2):] ft[win[:Lg//2]], win[j] = (start + j) mod nn
__device__ inline double2 band_fold(const double2 *__restrict__ ft, int nn,
                                    const double *__restrict__ g, const Job &jb, int m) {
  const int h1 = (jb.Lg + 1) >> 1, h2 = jb.Lg >> 1;
  const long long total = (long long)jb.col * jb.n;
  double2 acc = make_double2(0.0, 0.0);
  for (int j = 0; j < jb.col; ++j) {
    const long long i = (long long)m * jb.col + j;
    double w;
    int pos;
    if (i < h1) {
      w = g[jb.g_off + i];
      pos = jb.start + h2 + (int)i;
    } else if (i >= total - h2) {
      const int q = (int)(i - (total - h2));
      w = g[jb.g_off + h1 + q];
      pos = jb.start + q;
    } else {
      continue;
    }
    if (pos >= nn) pos -= nn;
    const double2 v = ft[pos];
    acc.x += w * v.x;
    acc.y += w * v.y;
  }
  return acc;
}

// ------------------------------------------------------------------ k_small
struct SmallArgs {
  const double *in;
  double *out;
  const double2 *ft;
  const double *g;
  const double2 *chirp, *bhat, *tw;
  const Job *jobs;
  long long in_chs, out_chs;
  int nn, gather, sign, in_real, out_real;
  int rot_nch, rot_first;   // the sliced forward's band rotation (0: none)
};

// kRot: the sliced forward's band rotation; the plain transform's instantiation
// carries none of it
template <bool kRot>
__global__ __launch_bounds__(256) void k_small(const SmallArgs a) {
  extern __shared__ double2 s[];
  const Job jb = a.jobs[blockIdx.x];
  const int ch = blockIdx.y;
  const int n = jb.n, P = jb.P, logP = jb.logP;
  const bool blu = P != n;
  const double2 *tw = a.tw + (P > 1 ? P / 2 - 1 : 0);
  const int turns = kRot ? slice_turns(a.rot_nch, a.rot_first, ch, 3) : 0;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    double2 v = make_double2(0.0, 0.0);
    if (p < n) {
      if (a.gather) {
        v = band_fold(a.ft + (long long)ch * a.nn, a.nn, a.g, jb, p);
        if (kRot) v = quarter_turns(v, turns * (p & 3));
      } else if (p < jb.n_in) {
        const long long idx = jb.in_off + (long long)ch * a.in_chs + p;
        v = a.in_real ? make_double2(a.in[idx], 0.0) : ((const double2 *)a.in)[idx];
      }
      if (a.sign > 0) v.y = -v.y;
      if (blu) v = cmul(v, a.chirp[jb.ch_off + p]);
    }
    s[brev(p, logP)] = v;
  }
  __syncthreads();
  lds_fft(s, tw, P, logP);
  if (blu) {
    // conj(A B) into bit-reversed order in place: i and rev(i) swap
    const double2 *B = a.bhat + jb.bh_off;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      const int j = brev(i, logP);
      if (i < j) {
        double2 x = cmul(s[i], B[i]), y = cmul(s[j], B[j]);
        x.y = -x.y;
        y.y = -y.y;
        s[i] = y;
        s[j] = x;
      } else if (i == j) {
        double2 x = cmul(s[i], B[i]);
        x.y = -x.y;
        s[i] = x;
      }
    }
    __syncthreads();
    lds_fft(s, tw, P, logP);
  }
  const double invP = 1.0 / (double)P;
  for (int k = threadIdx.x; k < n && k < jb.n_out; k += blockDim.x) {
    double2 v = s[k];
    if (blu) {
      v.y = -v.y;
      v = cmul(v, a.chirp[jb.ch_off + k]);
      v.x *= invP;
      v.y *= invP;
    }
    if (a.sign > 0) v.y = -v.y;
    v.x *= jb.scale;
    v.y *= jb.scale;
    const long long idx = jb.out_off + (long long)ch * a.out_chs + k;
    if (a.out_real)
      a.out[idx] = v.x;
    else
      ((double2 *)a.out)[idx] = v;
  }
}

// ------------------------------------------------------------ k_cols, k_rows
enum { SRC_EXT = 0, SRC_W = 1, SRC_GATHER = 2 };
enum { MUL_NONE = 0, MUL_CHIRP = 1, MUL_BHAT = 2 };

struct PassArgs {
  const double *in;
  double *out;
  double2 *W;                 // [nch][njobs][P] work array
  const double2 *ft;          // SRC_GATHER: [nch][nn]
  const double *g;
  const double2 *chirp, *bhat, *tw;
  const Job *jobs;
  long long in_chs, out_chs;
  double scale_mul;
  int nn, njobs, P, N1, N2, logN1, logN2, tile;  // tile: C (k_cols) or R (k_rows)
  int src, dst_w, in_real, out_real;
  int lconj, lmul, twid;      // twid: 0 none, 1 on the load, 2 on the store (k_cols)
  int sconj1, smul, sconj2, transpose_out;
  int rot_nch, rot_first;     // SRC_GATHER: the sliced forward's band rotation (0: none)
};

template <bool kRot>
__device__ __forceinline__ double2 pass_ld(const PassArgs &a, const Job &jb, long long wbase,
                                           int ch, int idx) {
  double2 v = make_double2(0.0, 0.0);
  if (a.src == SRC_W) {
    v = a.W[wbase + idx];
  } else if (a.src == SRC_GATHER) {
    if (idx < jb.n) {
      v = band_fold(a.ft + (long long)ch * a.nn, a.nn, a.g, jb, idx);
      if (kRot) v = quarter_turns(v, slice_turns(a.rot_nch, a.rot_first, ch, 3) * (idx & 3));
    }
  } else if (idx < jb.n_in) {
    const long long i = jb.in_off + (long long)ch * a.in_chs + idx;
    v = a.in_real ? make_double2(a.in[i], 0.0) : ((const double2 *)a.in)[i];
  }
  if (a.lconj) v.y = -v.y;
  if (a.lmul && idx < jb.n) v = cmul(v, a.chirp[jb.ch_off + idx]);
  return v;
}

__device__ __forceinline__ void pass_st(const PassArgs &a, const Job &jb, long long wbase, int ch,
                                        int idx, double2 v) {
  if (a.sconj1) v.y = -v.y;
  if (a.smul == MUL_BHAT) {
    v = cmul(v, a.bhat[jb.bh_off + idx]);
  } else if (a.smul == MUL_CHIRP) {
    if (idx < jb.n) v = cmul(v, a.chirp[jb.ch_off + idx]);
  }
  if (a.sconj2) v.y = -v.y;
  if (a.dst_w) {
    a.W[wbase + idx] = v;
    return;
  }
  if (idx >= jb.n_out) return;
  const double sc = jb.scale * a.scale_mul;
  const long long i = jb.out_off + (long long)ch * a.out_chs + idx;
  if (a.out_real)
    a.out[i] = v.x * sc;
  else
    ((double2 *)a.out)[i] = make_double2(v.x * sc, v.y * sc);
}

// exp(-2 pi i m / P); P is a power of two, so 2 m / P is exact
__device__ __forceinline__ double2 big_twiddle(long long m, double two_over_P) {
  double sn, cs;
  sincospi((double)m * two_over_P, &sn, &cs);
  return make_double2(cs, -sn);
}

// consecutive tiles on one XCD (blocks go round-robin over the 8 XCDs), so
// the partial lines of neighbouring column tiles meet in one L2
__device__ __forceinline__ int xcd_tile() {
  const int nb = gridDim.x, b = blockIdx.x;
  return (nb & 7) ? b : (b & 7) * (nb >> 3) + (b >> 3);
}

template <bool kRot>
__global__ __launch_bounds__(256) void k_cols(const PassArgs a) {
  extern __shared__ double2 s[];
  const int j = blockIdx.y, ch = blockIdx.z;
  const Job jb = a.jobs[j];
  const long long wbase = ((long long)ch * a.njobs + j) * a.P;
  const int C = a.tile, c0 = xcd_tile() * C, N1 = a.N1, N2 = a.N2;
  const double top = 2.0 / (double)a.P;
  const int cnt = N1 * C;
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int r = i / C, c = i - r * C;
    double2 v = pass_ld<kRot>(a, jb, wbase, ch, r * N2 + c0 + c);
    if (a.twid == 1) v = cmul(v, big_twiddle((long long)r * (c0 + c), top));
    s[c * N1 + brev(r, a.logN1)] = v;
  }
  __syncthreads();
  lds_fft_batch(s, a.tw + (N1 / 2 - 1), N1, a.logN1, C);
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int r = i / C, c = i - r * C;
    double2 v = s[c * N1 + r];
    if (a.twid == 2) v = cmul(v, big_twiddle((long long)r * (c0 + c), top));
    pass_st(a, jb, wbase, ch, r * N2 + c0 + c, v);
  }
}

__global__ __launch_bounds__(256) void k_rows(const PassArgs a) {
  extern __shared__ double2 s[];
  const int j = blockIdx.y, ch = blockIdx.z;
  const Job jb = a.jobs[j];
  const long long wbase = ((long long)ch * a.njobs + j) * a.P;
  const int R = a.tile, r0 = blockIdx.x * R, N1 = a.N1, N2 = a.N2;
  const int cnt = R * N2;
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int rr = i >> a.logN2, c = i & (N2 - 1);
    s[rr * N2 + brev(c, a.logN2)] = pass_ld<false>(a, jb, wbase, ch, (r0 + rr) * N2 + c);
  }
  __syncthreads();
  lds_fft_batch(s, a.tw + (N2 / 2 - 1), N2, a.logN2, R);
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    int rr, c, idx;
    if (a.transpose_out) {   // element k1 + N1 k2: runs of R along k1
      c = i / R;
      rr = i - c * R;
      idx = (r0 + rr) + N1 * c;
    } else {
      rr = i >> a.logN2;
      c = i & (N2 - 1);
      idx = (r0 + rr) * N2 + c;
    }
    pass_st(a, jb, wbase, ch, idx, s[rr * N2 + c]);
  }
}

// b of Bluestein's convolution: conj(chirp[|p|]) for |p| < n, wrapped to P
// (the rest of the zero-filled array stays zero)
__global__ __launch_bounds__(256) void k_bfill(const double2 *__restrict__ chirp, double2 *b, int n,
                                               int P) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const double2 c = chirp[p];
  const double2 v = make_double2(c.x, -c.y);
  b[p] = v;
  if (p > 0) b[P - p] = v;
}

// ------------------------------------------------------------------- k_ola
struct OlaTerm {
  long long gd_off, src_off;  // dual window; the source band's DFT in fc
  int start, Lg, srcM, mirror;
};

struct OlaArgs {
  const double2 *fc;   // [nch][coef_len] DFTs of the coefficient bands
  double2 *spec;       // [nch][nn]
  const double *gd;
  const OlaTerm *terms;
  const int *cov_ptr;  // [nn + 1]
  const int *cov;      // terms covering each bin, ascending
  long long coef_len;
  int nn, nbins, real;
  int rot_nch, rot_first;   // the sliced backward's band rotation (0: none)
};

// nsigtf.py:104-116 as a gather: fr[b] = sum over the covering bands, in
// ascending band order, of temp[i] gd[i] M
template <bool kRot>
__global__ __launch_bounds__(256) void k_ola(const OlaArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nbins) return;
  const int ch = blockIdx.y;
  const double2 *fc = a.fc + (long long)ch * a.coef_len;
  const int turns = kRot ? slice_turns(a.rot_nch, a.rot_first, ch, 1) : 0;
  double2 acc = make_double2(0.0, 0.0);
  for (int e = a.cov_ptr[b]; e < a.cov_ptr[b + 1]; ++e) {
    const OlaTerm t = a.terms[a.cov[e]];
    int j = b - t.start;
    if (j < 0) j += a.nn;
    const int h1 = (t.Lg + 1) >> 1, h2 = t.Lg >> 1;
    // window position j holds temp[i]: win[:Lg//2] takes temp[-(Lg//2):]
    const int i = j < h2 ? h1 + j : j - h2;
    int m = i < h1 ? i : t.srcM - t.Lg + i;
    double2 v;
    if (t.mirror) {   // fftsymm: conj(c[(M - m) mod M])
      m = m ? t.srcM - m : 0;
      v = fc[t.src_off + m];
      if (kRot) v = quarter_turns(v, turns * (m & 3));
      v.y = -v.y;
    } else {
      v = fc[t.src_off + m];
      if (kRot) v = quarter_turns(v, turns * (m & 3));
    }
    const double w = a.gd[t.gd_off + i];
    const double M = (double)t.srcM;
    acc.x += v.x * w * M;
    acc.y += v.y * w * M;
  }
  double2 *spec = a.spec + (long long)ch * a.nn;
  if (!a.real) {
    spec[b] = acc;
    return;
  }
  // irfft reads bins 0 .. nn/2 and drops the imaginary parts of DC and Nyquist
  if (b == 0 || 2 * b == a.nn) acc.y = 0.0;
  spec[b] = acc;
  if (b > 0 && 2 * b != a.nn) spec[a.nn - b] = make_double2(acc.x, -acc.y);
}

// -------------------------------------------------------- k_slice, k_unslice
// Quarter i of the four consecutive stream blocks of a slice sits at quarter
// (i + 3 - 2 k) mod 4 of the slice, k the slice's parity (slicing.py).
__device__ __forceinline__ int slice_quarter(int i, int k) { return (i + 3 - 2 * k) & 3; }

struct SliceArgs {
  const double *blocks;   // [nchan] runs of (2 nslices + 2) hhop samples, blk_chs apart
  double *xs;             // [nslices nchan][4 hhop]
  const double *wnd;      // [4 hhop] Tukey window, in stream order
  long long blk_chs;
  int hhop, nchan, first;
};

// slice s = blockIdx.y / nchan takes stream blocks 2s .. 2s+3, each times its
// quarter of the window; one thread per slice sample
__global__ __launch_bounds__(256) void k_slice(const SliceArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= 4 * a.hhop) return;
  const int s = blockIdx.y / a.nchan, c = blockIdx.y - s * a.nchan;
  const int qp = p / a.hhop, j = p - qp * a.hhop;
  const int i = (qp + 1 + 2 * ((a.first + s) & 1)) & 3;   // slice_quarter(i, k) == qp
  const double v = a.blocks[(long long)c * a.blk_chs + (long long)(2 * s + i) * a.hhop + j];
  a.xs[(long long)blockIdx.y * 4 * a.hhop + p] = v * a.wnd[i * a.hhop + j];
}

struct UnsliceArgs {
  const double *y;    // [nslices nchan][4 hhop] slices, real or complex
  double *out;        // [nchan] runs of 2 nslices hhop samples, out_chs apart
  double *carry;      // [nchan][2 hhop]: quarters 2, 3 of the slice before; in and out
  const double *wnd;  // [4 hhop] synthesis window, or null: plain addition
  long long out_chs;
  int hhop, nchan, nslices, first;
};

// Every product and sum rounds on its own: a sum formed through the carry
// buffer has the bits of the same sum formed inside one call.
template <typename T>
__device__ __forceinline__ T uns_term(const T *y, const double *wnd, long long at, int widx);
template <>
__device__ __forceinline__ double uns_term<double>(const double *y, const double *wnd,
                                                   long long at, int widx) {
#pragma clang fp contract(off)
  return wnd ? y[at] * wnd[widx] : y[at];
}
template <>
__device__ __forceinline__ double2 uns_term<double2>(const double2 *y, const double *wnd,
                                                     long long at, int widx) {
#pragma clang fp contract(off)
  const double2 v = y[at];
  if (!wnd) return v;
  const double w = wnd[widx];
  return make_double2(v.x * w, v.y * w);
}
__device__ __forceinline__ double uns_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double2 uns_add(double2 a, double2 b) {
#pragma clang fp contract(off)
  return make_double2(a.x + b.x, a.y + b.y);
}

// Output block b = 2s + i (i = 0, 1) of a call is quarter i + 2 of slice s - 1
// (the carry when s = 0) plus quarter i of slice s, in that order; the thread
// that reads a carry element then writes the last slice's quarter i + 2 there.
template <typename T>
__global__ __launch_bounds__(256) void k_unslice(const UnsliceArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2LL * a.nslices * a.hhop) return;
  const int c = blockIdx.y;
  const int b = (int)(t / a.hhop), j = (int)(t - (long long)b * a.hhop);
  const int s = b >> 1, i = b & 1, k = (a.first + s) & 1;
  const long long sl = 4LL * a.hhop;
  const T *y = (const T *)a.y;
  T *carry = (T *)a.carry + (long long)c * 2 * a.hhop;
  const T newer = uns_term<T>(y, a.wnd, ((long long)s * a.nchan + c) * sl +
                                            (long long)slice_quarter(i, k) * a.hhop + j,
                              i * a.hhop + j);
  T older;
  if (s > 0) {
    older = uns_term<T>(y, a.wnd, ((long long)(s - 1) * a.nchan + c) * sl +
                                      (long long)slice_quarter(i + 2, k ^ 1) * a.hhop + j,
                        (i + 2) * a.hhop + j);
  } else {
    const int last = a.nslices - 1, kl = (a.first + last) & 1;
    older = carry[i * a.hhop + j];
    carry[i * a.hhop + j] =
        uns_term<T>(y, a.wnd, ((long long)last * a.nchan + c) * sl +
                                  (long long)slice_quarter(i + 2, kl) * a.hhop + j,
                    (i + 2) * a.hhop + j);
  }
  ((T *)a.out)[(long long)c * a.out_chs + t] = uns_add(older, newer);
}

// ------------------------------------------------------------------- host
inline int next_pow2(long long n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
inline bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// chirp[k] = exp(-i pi k^2 / n): k^2 reduced mod 2n in integers, the angle in
// long double (in double the phase at k ~ 1e6 has no significant bit left)
void host_chirp(int n, double2 *out) {
  const long double pi = 3.141592653589793238462643383279502884L;
  const unsigned long long two_n = 2ull * (unsigned long long)n;
  for (int k = 0; k < n; ++k) {
    const unsigned long long r = ((unsigned long long)k * (unsigned long long)k) % two_n;
    const long double ang = pi * (long double)r / (long double)n;
    out[k] = make_double2((double)cosl(ang), (double)(-sinl(ang)));
  }
}

// forward FFT of size P on the host in long double (the small chirp spectra)
void host_fft(std::vector<long double> &re, std::vector<long double> &im, int P) {
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int i = 1, j = 0; i < P; ++i) {
    int bit = P >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (int len = 2; len <= P; len <<= 1) {
    for (int k = 0; k < len / 2; ++k) {
      const long double ang = -2.0L * pi * (long double)k / (long double)len;
      const long double wr = cosl(ang), wi = sinl(ang);
      for (int i = k; i < P; i += len) {
        const int j = i + len / 2;
        const long double tr = wr * re[j] - wi * im[j], ti = wr * im[j] + wi * re[j];
        re[j] = re[i] - tr;
        im[j] = im[i] - ti;
        re[i] += tr;
        im[i] += ti;
      }
    }
  }
}

struct Shape {   // how a length is transformed
  int n, P, logP, N1, N2, l1, l2, ctile, rtile;
  bool blu, small;
};

// force_blu: a band of a power-of-two length above 4096 shares the Bluestein
// batches of its neighbours
Shape make_shape(int n, bool force_blu) {
  Shape s{};
  s.n = n;
  s.blu = !is_pow2(n) || (force_blu && n > kLdsN);
  s.P = s.blu ? next_pow2(2LL * n - 1) : n;
  s.logP = ilog2(s.P);
  s.small = s.P <= kLdsN;
  if (!s.small) {
    if (s.blu) {
      s.l2 = 12;
      s.l1 = s.logP - 12;
    } else {
      s.l1 = s.logP / 2;
      s.l2 = s.logP - s.l1;
    }
    s.N1 = 1 << s.l1;
    s.N2 = 1 << s.l2;
    s.ctile = std::min(kLdsN / s.N1, s.N2);
    s.rtile = std::min(kLdsN / s.N2, s.N1);
  }
  return s;
}

struct TabRef {
  long long ch_off = 0, bh_off = 0;
};

// Twiddles, chirps and chirp spectra of a set of lengths, built once.
struct Tables {
  DBuf<double2> tw, chirp, bhat;
  DBuf<Job> dummy;
  std::map<int, TabRef> ref;   // Bluestein lengths
  std::vector<Shape> want;

  void add(const Shape &s) {
    if (s.blu && !ref.count(s.n)) {
      ref[s.n] = TabRef();
      want.push_back(s);
    }
  }
  int build(hipStream_t st);
};

int launch_pass(hipStream_t st, bool cols, const PassArgs &a, int nch) {
  const dim3 grid(cols ? a.N2 / a.tile : a.N1 / a.tile, a.njobs, nch);
  const size_t lds = sizeof(double2) * (size_t)a.tile * (cols ? a.N1 : a.N2);
  if (cols && a.rot_nch)
    k_cols<true><<<grid, 256, lds, st>>>(a);
  else if (cols)
    k_cols<false><<<grid, 256, lds, st>>>(a);
  else
    k_rows<<<grid, 256, lds, st>>>(a);
  FASST_LAUNCH_CHECK();
  ++g_launches;
  return FASST_OK;
}

PassArgs base_pass(const Tables &T, const Shape &s, const Job *jobs, int njobs, double2 *W) {
  PassArgs a{};
  a.W = W;
  a.chirp = T.chirp.p;
  a.bhat = T.bhat.p;
  a.tw = T.tw.p;
  a.jobs = jobs;
  a.njobs = njobs;
  a.P = s.P;
  a.N1 = s.N1;
  a.N2 = s.N2;
  a.logN1 = s.l1;
  a.logN2 = s.l2;
  a.scale_mul = 1.0;
  return a;
}

int Tables::build(hipStream_t st) {
  std::vector<double2> h_tw;
  for (int n = 2; n <= kLdsN; n <<= 1) {
    const std::vector<double2> t = twiddles(n, -1);
    h_tw.insert(h_tw.end(), t.begin(), t.end());
  }
  int e = tw.alloc_uninit(h_tw.size());
  if (e) return e;
  FASST_TRY(tw.put(h_tw.data(), h_tw.size()));
  if ((e = dummy.alloc(1))) return e;
  if (want.empty()) return FASST_OK;
  std::sort(want.begin(), want.end(), [](const Shape &x, const Shape &y) {
    return x.P != y.P ? x.P < y.P : x.n < y.n;
  });
  long long nch_tot = 0, nbh_tot = 0, nbh_small = 0;
  for (const Shape &s : want) {
    TabRef &r = ref[s.n];
    r.ch_off = nch_tot;
    r.bh_off = nbh_tot;
    nch_tot += s.n;
    nbh_tot += s.P;
    if (s.small) nbh_small = nbh_tot;
  }
  std::vector<double2> h_ch((size_t)nch_tot), h_bh((size_t)nbh_small);
  std::vector<long double> re, im;
  for (const Shape &s : want) {
    const TabRef &r = ref[s.n];
    double2 *c = h_ch.data() + r.ch_off;
    host_chirp(s.n, c);
    if (!s.small) continue;
    re.assign(s.P, 0.0L);
    im.assign(s.P, 0.0L);
    for (int p = 0; p < s.n; ++p) {
      re[p] = c[p].x;
      im[p] = -c[p].y;
      if (p) {
        re[s.P - p] = c[p].x;
        im[s.P - p] = -c[p].y;
      }
    }
    host_fft(re, im, s.P);
    for (int p = 0; p < s.P; ++p)
      h_bh[r.bh_off + p] = make_double2((double)re[p], (double)im[p]);
  }
  if ((e = chirp.alloc_uninit((size_t)nch_tot))) return e;
  if ((e = bhat.alloc((size_t)nbh_tot))) return e;   // zero-filled
  FASST_TRY(chirp.put(h_ch.data(), h_ch.size()));
  FASST_TRY(bhat.put(h_bh.data(), h_bh.size()));
  // the large chirp spectra on the device, left in [k1][k2] order
  for (const Shape &s : want) {
    if (s.small) continue;
    const TabRef &r = ref[s.n];
    double2 *b = bhat.p + r.bh_off;
    k_bfill<<<(s.n + 255) / 256, 256, 0, st>>>(chirp.p + r.ch_off, b, s.n, s.P);
    FASST_LAUNCH_CHECK();
    ++g_launches;
    PassArgs a = base_pass(*this, s, dummy.p, 1, b);
    a.src = SRC_W;
    a.dst_w = 1;
    a.twid = 2;
    a.tile = s.ctile;
    if ((e = launch_pass(st, true, a, 1))) return e;
    a.twid = 0;
    a.tile = s.rtile;
    if ((e = launch_pass(st, false, a, 1))) return e;
  }
  FASST_HIP(hipStreamSynchronize(st));
  return FASST_OK;
}

// where a batch reads and writes
struct Io {
  int src = SRC_EXT;          // SRC_EXT or SRC_GATHER
  const double *in = nullptr;
  int in_real = 0;
  long long in_chs = 0;
  const double2 *ft = nullptr;
  const double *g = nullptr;
  int nn = 0;
  double *out = nullptr;
  int out_real = 0;
  long long out_chs = 0;
  int rot_nch = 0, rot_first = 0;   // SRC_GATHER of a sliced plan
};

// `njobs` transforms of one shape, out = sum in exp(sign 2 pi i n k / N) * scale
int run_batch(hipStream_t st, const Tables &T, const Shape &s, const Job *jobs, int njobs, int sign,
              int nch, const Io &io, double2 *W) {
  int e;
  if (s.small) {
    SmallArgs a{};
    a.in = io.in;
    a.out = io.out;
    a.ft = io.ft;
    a.g = io.g;
    a.chirp = T.chirp.p;
    a.bhat = T.bhat.p;
    a.tw = T.tw.p;
    a.jobs = jobs;
    a.in_chs = io.in_chs;
    a.out_chs = io.out_chs;
    a.nn = io.nn;
    a.gather = io.src == SRC_GATHER;
    a.sign = sign;
    a.in_real = io.in_real;
    a.out_real = io.out_real;
    a.rot_nch = io.rot_nch;
    a.rot_first = io.rot_first;
    if (a.rot_nch)
      k_small<true><<<dim3(njobs, nch), 256, sizeof(double2) * (size_t)s.P, st>>>(a);
    else
      k_small<false><<<dim3(njobs, nch), 256, sizeof(double2) * (size_t)s.P, st>>>(a);
    FASST_LAUNCH_CHECK();
    ++g_launches;
    return FASST_OK;
  }
  PassArgs a = base_pass(T, s, jobs, njobs, W);
  a.in = io.in;
  a.in_real = io.in_real;
  a.in_chs = io.in_chs;
  a.ft = io.ft;
  a.g = io.g;
  a.nn = io.nn;
  a.out = io.out;
  a.out_real = io.out_real;
  a.out_chs = io.out_chs;
  a.rot_nch = io.rot_nch;
  a.rot_first = io.rot_first;
  const int conj = sign > 0;
  // columns first, twiddle on the store, into the work array
  a.src = io.src;
  a.dst_w = 1;
  a.lconj = conj;
  a.lmul = s.blu;
  a.twid = 2;
  a.tile = s.ctile;
  if ((e = launch_pass(st, true, a, nch))) return e;
  a.src = SRC_W;
  a.lconj = a.lmul = a.twid = 0;
  a.tile = s.rtile;
  if (!s.blu) {   // rows, stored transposed: natural order
    a.dst_w = 0;
    a.transpose_out = 1;
    a.sconj1 = conj;
    return launch_pass(st, false, a, nch);
  }
  a.smul = MUL_BHAT;   // rows; the product with the chirp's spectrum
  if ((e = launch_pass(st, false, a, nch))) return e;
  a.smul = MUL_NONE;   // the inverse: conj, rows, twiddle, columns, conj
  a.lconj = 1;
  if ((e = launch_pass(st, false, a, nch))) return e;
  a.lconj = 0;
  a.twid = 1;
  a.tile = s.ctile;
  a.dst_w = 0;
  a.sconj1 = 1;
  a.smul = MUL_CHIRP;
  a.sconj2 = conj;
  a.scale_mul = 1.0 / (double)s.P;
  return launch_pass(st, true, a, nch);
}

struct Group {
  Shape shape;
  std::vector<Job> h;
  DBuf<Job> jobs;
};

struct Plan {
  int device = 0, Ls = 0, nn = 0, nbands = 0, real = 0, nused = 0, nterms = 0;
  long long coef_len = 0;
  Tables T;
  Shape sh_ls{}, sh_nn{};
  DBuf<Job> job_ls, job_nn;
  DBuf<double> g, gd;
  // band batches: [0] every band with P <= kSmallLoP and [1] every other band
  // with P <= 4096 (one k_small launch each), then one batch per larger P
  std::vector<Group> fwd, bwd;
  int small_lds_P[2] = {1, 1};
  DBuf<OlaTerm> terms;
  DBuf<int> cov_ptr, cov;
  // grown to the largest nch seen, never shrunk
  int nch_cap = 0;
  long long w_per_ch = 0;
  DBuf<double2> ft, fc, spec, W, coef_h;
  DBuf<double> sig_h, y_h;

  int ensure(int nch) {
    if (nch <= nch_cap) return FASST_OK;
    int e;
    if ((e = ft.alloc((size_t)nch * nn))) return e;   // zero tail beyond Ls stays zero
    if ((e = fc.alloc_uninit((size_t)nch * coef_len))) return e;
    if ((e = spec.alloc_uninit((size_t)nch * nn))) return e;
    if ((e = W.alloc_uninit((size_t)nch * w_per_ch))) return e;
    if ((e = coef_h.alloc_uninit((size_t)nch * coef_len))) return e;
    if ((e = sig_h.alloc_uninit((size_t)nch * Ls))) return e;
    if ((e = y_h.alloc_uninit((size_t)nch * Ls * 2))) return e;
    nch_cap = nch;
    return FASST_OK;
  }

  // a sliced plan (Ls = sl_len = 4 hhop): the slicing and synthesis windows,
  // and the host route's staging of stream blocks, output and carry
  int hhop = 0, tr_area = 0;
  DBuf<double> slwnd, recwnd, blk_h, out_h, carry_h;

  int ensure_sliced(int nchan, int nslices) {
    int e;
    const size_t nblk = (size_t)nchan * (2 * (size_t)nslices + 2) * hhop;
    if (blk_h.n < nblk && (e = blk_h.alloc_uninit(nblk))) return e;
    if (out_h.n < 2 * nblk && (e = out_h.alloc_uninit(2 * nblk))) return e;
    const size_t ncar = (size_t)nchan * 4 * hhop;
    if (carry_h.n < ncar && (e = carry_h.alloc_uninit(ncar))) return e;
    return FASST_OK;
  }
};

int bad(int code, const char *fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  set_error("%s", buf);
  return code;
}

// bands with P <= 4096 share two launches of k_small, split at kSmallLoP so
// that the many narrow bands do not carry the LDS of the widest (a launch's
// LDS is the largest P in it); the others batch by P
void add_job(std::vector<Group> &groups, const Shape &s, const Job &j) {
  if (s.small) {
    groups[s.P <= kSmallLoP ? 0 : 1].h.push_back(j);
    return;
  }
  for (size_t i = kSmallGroups; i < groups.size(); ++i)
    if (groups[i].shape.P == s.P) {
      groups[i].h.push_back(j);
      return;
    }
  groups.emplace_back();
  groups.back().shape = s;
  groups.back().h.push_back(j);
}

int upload_groups(std::vector<Group> &groups) {
  for (Group &gr : groups) {
    if (gr.h.empty()) continue;
    // widest first: the long blocks of the shared launch start early
    std::stable_sort(gr.h.begin(), gr.h.end(), [](const Job &x, const Job &y) { return x.P > y.P; });
    int e = gr.jobs.alloc_uninit(gr.h.size());
    if (e) return e;
    FASST_TRY(gr.jobs.put(gr.h.data(), gr.h.size()));
  }
  return FASST_OK;
}

int run_groups(hipStream_t st, Plan *p, std::vector<Group> &groups, int sign, int nch, const Io &io) {
  for (size_t i = 0; i < groups.size(); ++i) {
    Group &gr = groups[i];
    if (gr.h.empty()) continue;
    Shape s = gr.shape;
    if (i < (size_t)kSmallGroups) {
      s = Shape{};
      s.small = true;
      s.P = p->small_lds_P[i];
    }
    int e = run_batch(st, p->T, s, gr.jobs.p, (int)gr.h.size(), sign, nch, io, p->W.p);
    if (e) return e;
  }
  return FASST_OK;
}

Job single_job(const Tables &T, const Shape &s, int n_in, int n_out, double scale) {
  Job j{};
  j.n = s.n;
  j.n_in = n_in;
  j.n_out = n_out;
  j.P = s.P;
  j.logP = s.logP;
  j.scale = scale;
  if (s.blu) {
    const TabRef &r = T.ref.at(s.n);
    j.ch_off = r.ch_off;
    j.bh_off = r.bh_off;
  }
  return j;
}

int upload_job(DBuf<Job> &d, const Job &j) {
  int e = d.alloc_uninit(1);
  if (e) return e;
  return d.put(&j, 1);
}

struct CallTimer {
  Events ev;
  bool on = false;
  int start(hipStream_t st) {
    on = t_timing != 0;
    if (!on) return FASST_OK;
    int e = ev.create(3);
    if (e) return e;
    FASST_HIP(hipEventRecord(ev.e[0], st));
    return FASST_OK;
  }
  int mark(hipStream_t st) {
    if (on) FASST_HIP(hipEventRecord(ev.e[2], st));
    return FASST_OK;
  }
  // fft_first: the whole-signal FFT ran before the mark, else after it
  int finish(hipStream_t st, bool fft_first) {
    if (!on) return FASST_OK;
    float total = 0.f, part = 0.f;
    int e = elapsed_ms(ev.e[0], ev.e[1], st, &total);
    if (e) return e;
    if (fft_first)
      FASST_HIP(hipEventElapsedTime(&part, ev.e[0], ev.e[2]));
    else
      FASST_HIP(hipEventElapsedTime(&part, ev.e[2], ev.e[1]));
    t_ms[0] = total;
    t_ms[1] = part;
    return FASST_OK;
  }
};

// The kernels of one forward on device arrays: x [nch][Ls] -> coef.  rot_nch /
// rot_first: the band rotation of a sliced plan (0: none).
int forward_kernels(Plan *p, hipStream_t st, CallTimer &tm, int nch, const double *dx, double *dc,
                    int rot_nch, int rot_first) {
  int e;
  Io io;
  io.in = dx;
  io.in_real = 1;
  io.in_chs = p->Ls;
  io.out = (double *)p->ft.p;
  io.out_chs = p->nn;
  if ((e = run_batch(st, p->T, p->sh_ls, p->job_ls.p, 1, -1, nch, io, p->W.p))) return e;
  if ((e = tm.mark(st))) return e;
  Io bio;
  bio.src = SRC_GATHER;
  bio.ft = p->ft.p;
  bio.g = p->g.p;
  bio.nn = p->nn;
  bio.out = dc;
  bio.out_chs = p->coef_len;
  bio.rot_nch = rot_nch;
  bio.rot_first = rot_first;
  return run_groups(st, p, p->fwd, +1, nch, bio);
}

// The kernels of one backward on device arrays: coef -> y [nch][Ls].
int backward_kernels(Plan *p, hipStream_t st, CallTimer &tm, int nch, const double *dc, double *dy,
                     int rot_nch, int rot_first) {
  int e;
  Io bio;
  bio.in = dc;
  bio.in_chs = p->coef_len;
  bio.out = (double *)p->fc.p;
  bio.out_chs = p->coef_len;
  if ((e = run_groups(st, p, p->bwd, -1, nch, bio))) return e;
  OlaArgs oa{};
  oa.fc = p->fc.p;
  oa.spec = p->spec.p;
  oa.gd = p->gd.p;
  oa.terms = p->terms.p;
  oa.cov_ptr = p->cov_ptr.p;
  oa.cov = p->cov.p;
  oa.coef_len = p->coef_len;
  oa.nn = p->nn;
  oa.real = p->real;
  oa.nbins = p->real ? p->nn / 2 + 1 : p->nn;
  oa.rot_nch = rot_nch;
  oa.rot_first = rot_first;
  if (rot_nch)
    k_ola<true><<<dim3((oa.nbins + 255) / 256, nch), 256, 0, st>>>(oa);
  else
    k_ola<false><<<dim3((oa.nbins + 255) / 256, nch), 256, 0, st>>>(oa);
  FASST_LAUNCH_CHECK();
  ++g_launches;
  if ((e = tm.mark(st))) return e;
  Io io;
  io.in = (const double *)p->spec.p;
  io.in_chs = p->nn;
  io.out = dy;
  io.out_real = p->real;
  io.out_chs = p->Ls;
  return run_batch(st, p->T, p->sh_nn, p->job_nn.p, 1, +1, nch, io, p->W.p);
}

// what a sliced call refuses before any device call
int check_sliced(const char *who, Plan *p, int nchan, int nslices, int first) {
  if (!p) return bad(FASST_ERR_SHAPE, "%s: null plan", who);
  if (!p->hhop) return bad(FASST_ERR_SHAPE, "%s: the plan is not a sliced plan", who);
  if (nchan < 1 || nslices < 1 || first < 0 || (long long)nchan * nslices > 65535)
    return bad(FASST_ERR_SHAPE,
               "%s: %d channels x %d slices from slice %d (at most 65535 slices x channels a call)",
               who, nchan, nslices, first);
  return FASST_OK;
}

}  // namespace
}  // namespace fasst

using namespace fasst;

extern "C" {

int fasst_nsgt_plan_create(int device, int Ls, int nn, int nbands, const int *M, const int *Lg,
                           const int *start, const double *g, const double *gd, int real,
                           int reducedform, void **plan) {
  if (!plan) return bad(FASST_ERR_SHAPE, "nsgt_plan_create: null plan pointer");
  *plan = nullptr;
  if (!M || !Lg || !start || !g || !gd)
    return bad(FASST_ERR_SHAPE, "nsgt_plan_create: null argument");
  if (nbands < 1 || Ls < 1 || nn < Ls)
    return bad(FASST_ERR_SHAPE, "nsgt_plan_create: bad sizes (nbands %d, Ls %d, nn %d)", nbands, Ls,
               nn);
  if (reducedform < 0 || reducedform > 2 || (real && (nbands & 1)) ||
      (real && nbands / 2 + 1 - 2 * reducedform < 1))
    return bad(FASST_ERR_SHAPE, "nsgt_plan_create: %d bands, real %d, reducedform %d", nbands, real,
               reducedform);
  if (Ls > FASST_NSGT_MAX_N || nn > FASST_NSGT_MAX_N)
    return bad(FASST_ERR_UNSUPPORTED, "nsgt_plan_create: Ls %d / nn %d above the ceiling %d", Ls, nn,
               FASST_NSGT_MAX_N);
  long long glen = 0;
  for (int k = 0; k < nbands; ++k) {
    if (M[k] < 1) return bad(FASST_ERR_SHAPE, "nsgt_plan_create: band %d has M %d < 1", k, M[k]);
    if (Lg[k] < 2 || Lg[k] > nn)
      return bad(FASST_ERR_SHAPE, "nsgt_plan_create: band %d has a window of %d points (nn %d)", k,
                 Lg[k], nn);
    if (start[k] < 0 || start[k] >= nn)
      return bad(FASST_ERR_SHAPE, "nsgt_plan_create: band %d starts at bin %d (nn %d)", k, start[k],
                 nn);
    if (M[k] > FASST_NSGT_MAX_N)
      return bad(FASST_ERR_UNSUPPORTED, "nsgt_plan_create: band %d has M %d above the ceiling %d", k,
                 M[k], FASST_NSGT_MAX_N);
    glen += Lg[k];
  }
  // the bands a transform uses, and the terms of the inverse's overlap-add
  const int nh = nbands / 2;
  const int b0 = real ? reducedform : 0, b1 = real ? nh + 1 - reducedform : nbands;
  std::vector<long long> goff(nbands), coff(nbands, -1);
  {
    long long o = 0;
    for (int k = 0; k < nbands; ++k) {
      goff[k] = o;
      o += Lg[k];
    }
  }
  long long coef_len = 0;
  for (int k = b0; k < b1; ++k) {
    coff[k] = coef_len;
    coef_len += M[k];
  }
  std::vector<OlaTerm> terms;
  auto add_term = [&](int k, int src, int mirror) {
    OlaTerm t{};
    t.gd_off = goff[k];
    t.src_off = coff[src];
    t.start = start[k];
    t.Lg = Lg[k];
    t.srcM = M[src];
    t.mirror = mirror;
    terms.push_back(t);
  };
  for (int k = b0; k < b1; ++k) add_term(k, k, 0);
  if (real)
    for (int k = nh + (reducedform ? reducedform : 1); k <= 2 * nh - (reducedform ? reducedform : 1);
         ++k)
      add_term(k, 2 * nh - k, 1);
  for (size_t i = 0; i < terms.size(); ++i)
    if (terms[i].srcM < (terms[i].Lg + 1) / 2)
      return bad(FASST_ERR_SHAPE,
                 "nsgt_plan_create: a band of M %d under a window of %d points: the inverse's "
                 "slices do not fit",
                 terms[i].srcM, terms[i].Lg);

  Plan *p = new Plan();
  p->device = device;
  p->Ls = Ls;
  p->nn = nn;
  p->nbands = nbands;
  p->real = real;
  p->nused = b1 - b0;
  p->coef_len = coef_len;
  p->nterms = (int)terms.size();
  p->sh_ls = make_shape(Ls, false);
  p->sh_nn = make_shape(nn, false);
  p->T.add(p->sh_ls);
  p->T.add(p->sh_nn);
  std::vector<Shape> bshape(nbands);
  for (int k = b0; k < b1; ++k) {
    bshape[k] = make_shape(M[k], true);
    p->T.add(bshape[k]);
  }
  // the cover table: terms over each bin, ascending
  std::vector<int> cptr((size_t)nn + 1, 0);
  for (const OlaTerm &t : terms)
    for (int j = 0; j < t.Lg; ++j) ++cptr[(t.start + j) % nn + 1];
  for (int b = 0; b < nn; ++b) cptr[b + 1] += cptr[b];
  std::vector<int> cov((size_t)cptr[nn]), fill(cptr.begin(), cptr.end() - 1);
  for (size_t i = 0; i < terms.size(); ++i)
    for (int j = 0; j < terms[i].Lg; ++j) cov[fill[(terms[i].start + j) % nn]++] = (int)i;

  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  int e = FASST_OK;
  auto fail = [&](int code) {
    delete p;
    return code;
  };
  if ((e = p->T.build(st))) return fail(e);
  p->fwd.resize(kSmallGroups);
  p->bwd.resize(kSmallGroups);
  for (int k = b0; k < b1; ++k) {
    const Shape &s = bshape[k];
    Job j = single_job(p->T, s, M[k], M[k], 1.0 / (double)M[k]);
    j.out_off = coff[k];
    j.g_off = goff[k];
    j.Lg = Lg[k];
    j.start = start[k];
    j.col = (Lg[k] + M[k] - 1) / M[k];
    add_job(p->fwd, s, j);
    Job b = single_job(p->T, s, M[k], M[k], 1.0);
    b.in_off = coff[k];
    b.out_off = coff[k];
    add_job(p->bwd, s, b);
    if (s.small) {
      int &lds = p->small_lds_P[s.P <= kSmallLoP ? 0 : 1];
      lds = std::max(lds, s.P);
    }
  }
  if ((e = upload_groups(p->fwd)) || (e = upload_groups(p->bwd))) return fail(e);
  p->w_per_ch = 1;
  if (!p->sh_ls.small) p->w_per_ch = std::max<long long>(p->w_per_ch, p->sh_ls.P);
  if (!p->sh_nn.small) p->w_per_ch = std::max<long long>(p->w_per_ch, p->sh_nn.P);
  for (size_t i = kSmallGroups; i < p->fwd.size(); ++i)
    p->w_per_ch = std::max<long long>(p->w_per_ch, (long long)p->fwd[i].shape.P * p->fwd[i].h.size());
  if ((e = upload_job(p->job_ls, single_job(p->T, p->sh_ls, Ls, Ls, 1.0)))) return fail(e);
  if ((e = upload_job(p->job_nn, single_job(p->T, p->sh_nn, nn, Ls, 1.0 / (double)nn))))
    return fail(e);
  if ((e = p->g.alloc_uninit((size_t)glen)) || (e = p->gd.alloc_uninit((size_t)glen)) ||
      (e = p->terms.alloc_uninit(terms.size())) || (e = p->cov_ptr.alloc_uninit(cptr.size())) ||
      (e = p->cov.alloc_uninit(cov.size())))
    return fail(e);
  if ((e = p->g.put(g, glen)) || (e = p->gd.put(gd, glen)) ||
      (e = p->terms.put(terms.data(), terms.size())) ||
      (e = p->cov_ptr.put(cptr.data(), cptr.size())) || (e = p->cov.put(cov.data(), cov.size())))
    return fail(e);
  *plan = p;
  return FASST_OK;
}

int fasst_nsgt_plan_destroy(void *plan) {
  Plan *p = (Plan *)plan;
  if (!p) return FASST_OK;
  DeviceGuard guard(p->device);
  delete p;
  return FASST_OK;
}

int fasst_nsgt_coef_len(void *plan, long *out) {
  if (!plan || !out) return bad(FASST_ERR_SHAPE, "nsgt_coef_len: null argument");
  *out = (long)((Plan *)plan)->coef_len;
  return FASST_OK;
}

int fasst_nsgt_forward(void *plan, int nch, const double *x, int is_device, double *coef) {
  Plan *p = (Plan *)plan;
  if (!p || !x || !coef || nch < 1 || nch > 65535)
    return bad(FASST_ERR_SHAPE, "nsgt_forward: null argument or bad channel count %d", nch);
  DeviceGuard guard(p->device);
  hipStream_t st = nullptr;
  int e = p->ensure(nch);
  if (e) return e;
  const double *dx = x;
  double *dc = coef;
  if (!is_device) {
    FASST_TRY(p->sig_h.put(x, (size_t)nch * p->Ls));
    dx = p->sig_h.p;
    dc = (double *)p->coef_h.p;
  }
  CallTimer tm;
  if ((e = tm.start(st))) return e;
  if ((e = forward_kernels(p, st, tm, nch, dx, dc, 0, 0))) return e;
  if ((e = tm.finish(st, true))) return e;
  FASST_HIP(hipStreamSynchronize(st));
  if (!is_device) FASST_TRY(p->coef_h.get(coef, (size_t)nch * p->coef_len));
  return FASST_OK;
}

int fasst_nsgt_backward(void *plan, int nch, const double *coef, int is_device, double *y) {
  Plan *p = (Plan *)plan;
  if (!p || !coef || !y || nch < 1 || nch > 65535)
    return bad(FASST_ERR_SHAPE, "nsgt_backward: null argument or bad channel count %d", nch);
  DeviceGuard guard(p->device);
  hipStream_t st = nullptr;
  int e = p->ensure(nch);
  if (e) return e;
  const double *dc = coef;
  double *dy = y;
  // y_h holds doubles: a complex output is two of them per sample
  const size_t ny = (p->real ? 1 : 2) * (size_t)nch * p->Ls;
  if (!is_device) {
    FASST_TRY(p->coef_h.put(coef, (size_t)nch * p->coef_len));
    dc = (const double *)p->coef_h.p;
    dy = p->y_h.p;
  }
  CallTimer tm;
  if ((e = tm.start(st))) return e;
  if ((e = backward_kernels(p, st, tm, nch, dc, dy, 0, 0))) return e;
  if ((e = tm.finish(st, false))) return e;
  FASST_HIP(hipStreamSynchronize(st));
  if (!is_device) FASST_TRY(p->y_h.get(y, ny));
  return FASST_OK;
}

int fasst_nsgt_sliced_plan_create(int device, int sl_len, int tr_area, int nn, int nbands,
                                  const int *M, const int *Lg, const int *start, const double *g,
                                  const double *gd, int real, int reducedform, const double *slwnd,
                                  const double *recwnd, void **plan) {
  if (!plan) return bad(FASST_ERR_SHAPE, "nsgt_sliced_plan_create: null plan pointer");
  *plan = nullptr;
  if (!M || !slwnd) return bad(FASST_ERR_SHAPE, "nsgt_sliced_plan_create: null argument");
  if (sl_len < 4 || sl_len % 4)
    return bad(FASST_ERR_SHAPE, "nsgt_sliced_plan_create: sl_len %d is not a multiple of 4", sl_len);
  if (tr_area < 0 || tr_area % 2 || sl_len <= 2 * tr_area)
    return bad(FASST_ERR_SHAPE,
               "nsgt_sliced_plan_create: tr_area %d must be even, >= 0 and below sl_len / 2 = %d",
               tr_area, sl_len / 2);
  for (int k = 0; k < nbands; ++k)
    if (M[k] % 4)
      return bad(FASST_ERR_SHAPE,
                 "nsgt_sliced_plan_create: band %d has M %d, not a multiple of 4: the slices' "
                 "rotations by M/4 and 3M/4 would not undo each other",
                 k, M[k]);
  void *h = nullptr;
  int e = fasst_nsgt_plan_create(device, sl_len, nn, nbands, M, Lg, start, g, gd, real, reducedform,
                                 &h);
  if (e) return e;
  Plan *p = (Plan *)h;
  DeviceGuard guard(device);
  p->hhop = sl_len / 4;
  p->tr_area = tr_area;
  if ((e = p->slwnd.upload(slwnd, (size_t)sl_len)) ||
      (recwnd && (e = p->recwnd.upload(recwnd, (size_t)sl_len)))) {
    delete p;
    return e;
  }
  *plan = p;
  return FASST_OK;
}

int fasst_nsgt_sliced_forward(void *plan, int nchan, int nslices, int first_slice_index,
                              const double *blocks, long blocks_stride, int is_device,
                              double *coef) {
  Plan *p = (Plan *)plan;
  int e = check_sliced("nsgt_sliced_forward", p, nchan, nslices, first_slice_index);
  if (e) return e;
  const long long run = (2LL * nslices + 2) * p->hhop;
  if (!blocks || !coef || blocks_stride < run || (!is_device && blocks_stride != run))
    return bad(FASST_ERR_SHAPE,
               "nsgt_sliced_forward: null argument or a channel stride of %ld under runs of %lld",
               blocks_stride, run);
  DeviceGuard guard(p->device);
  hipStream_t st = nullptr;
  const int nch = nchan * nslices;
  if ((e = p->ensure(nch)) || (e = p->ensure_sliced(nchan, nslices))) return e;
  const double *db = blocks;
  double *dc = coef;
  if (!is_device) {
    FASST_TRY(p->blk_h.put(blocks, (size_t)nchan * run));
    db = p->blk_h.p;
    dc = (double *)p->coef_h.p;
  }
  CallTimer tm;
  if ((e = tm.start(st))) return e;
  SliceArgs sa{};
  sa.blocks = db;
  sa.xs = p->sig_h.p;
  sa.wnd = p->slwnd.p;
  sa.blk_chs = blocks_stride;
  sa.hhop = p->hhop;
  sa.nchan = nchan;
  sa.first = first_slice_index & 1;
  k_slice<<<dim3((p->Ls + 255) / 256, nch), 256, 0, st>>>(sa);
  FASST_LAUNCH_CHECK();
  ++g_launches;
  if ((e = forward_kernels(p, st, tm, nch, p->sig_h.p, dc, nchan, first_slice_index & 1))) return e;
  if ((e = tm.finish(st, true))) return e;
  FASST_HIP(hipStreamSynchronize(st));
  if (!is_device) FASST_TRY(p->coef_h.get(coef, (size_t)nch * p->coef_len));
  return FASST_OK;
}

int fasst_nsgt_sliced_backward(void *plan, int nchan, int nslices, int first_slice_index,
                               const double *coef, double *carry_in_out, int is_device, double *y,
                               long y_stride) {
  Plan *p = (Plan *)plan;
  int e = check_sliced("nsgt_sliced_backward", p, nchan, nslices, first_slice_index);
  if (e) return e;
  const long long run = 2LL * nslices * p->hhop;
  if (!coef || !carry_in_out || !y || y_stride < run || (!is_device && y_stride != run))
    return bad(FASST_ERR_SHAPE,
               "nsgt_sliced_backward: null argument or a channel stride of %ld under runs of %lld",
               y_stride, run);
  DeviceGuard guard(p->device);
  hipStream_t st = nullptr;
  const int nch = nchan * nslices;
  if ((e = p->ensure(nch)) || (e = p->ensure_sliced(nchan, nslices))) return e;
  const size_t width = p->real ? 1 : 2;   // doubles per sample
  const size_t ncarry = width * (size_t)nchan * 2 * p->hhop, nout = width * (size_t)nchan * run;
  const double *dc = coef;
  double *dcar = carry_in_out, *dout = y;
  if (!is_device) {
    FASST_TRY(p->coef_h.put(coef, (size_t)nch * p->coef_len));
    FASST_TRY(p->carry_h.put(carry_in_out, ncarry));
    dc = (const double *)p->coef_h.p;
    dcar = p->carry_h.p;
    dout = p->out_h.p;
  }
  CallTimer tm;
  if ((e = tm.start(st))) return e;
  if ((e = backward_kernels(p, st, tm, nch, dc, p->y_h.p, nchan, first_slice_index & 1))) return e;
  UnsliceArgs ua{};
  ua.y = p->y_h.p;
  ua.out = dout;
  ua.carry = dcar;
  ua.wnd = p->recwnd.p;
  ua.out_chs = y_stride;
  ua.hhop = p->hhop;
  ua.nchan = nchan;
  ua.nslices = nslices;
  ua.first = first_slice_index & 1;
  const dim3 grid((unsigned)((run + 255) / 256), nchan);
  if (p->real)
    k_unslice<double><<<grid, 256, 0, st>>>(ua);
  else
    k_unslice<double2><<<grid, 256, 0, st>>>(ua);
  FASST_LAUNCH_CHECK();
  ++g_launches;
  if ((e = tm.finish(st, false))) return e;
  FASST_HIP(hipStreamSynchronize(st));
  if (!is_device) {
    FASST_TRY(p->out_h.get(y, nout));
    FASST_TRY(p->carry_h.get(carry_in_out, ncarry));
  }
  return FASST_OK;
}

int fasst_nsgt_fft(int device, int n, int sign, const double *in, double *out) {
  if (!in || !out || n < 1 || (sign != 1 && sign != -1))
    return bad(FASST_ERR_SHAPE, "nsgt_fft: bad arguments (n %d, sign %d)", n, sign);
  if (n > FASST_NSGT_MAX_N && !(is_pow2(n) && n <= kMaxP))
    return bad(FASST_ERR_UNSUPPORTED, "nsgt_fft: n %d above the ceiling %d", n, FASST_NSGT_MAX_N);
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  Tables T;
  const Shape s = make_shape(n, false);
  T.add(s);
  int e = T.build(st);
  if (e) return e;
  DBuf<Job> job;
  DBuf<double2> din, dout, W;
  if ((e = upload_job(job, single_job(T, s, n, n, 1.0)))) return e;
  if ((e = din.alloc_uninit(n)) || (e = dout.alloc_uninit(n)) ||
      (e = W.alloc_uninit(s.small ? 1 : s.P)))
    return e;
  FASST_TRY(din.put(in, n));
  Io io;
  io.in = (const double *)din.p;
  io.out = (double *)dout.p;
  if ((e = run_batch(st, T, s, job.p, 1, sign, 1, io, W.p))) return e;
  FASST_HIP(hipStreamSynchronize(st));
  return dout.get(out, n);
}

int fasst_nsgt_launch_count(long *count) {
  if (!count) return bad(FASST_ERR_SHAPE, "nsgt_launch_count: null argument");
  *count = g_launches.load();
  return FASST_OK;
}

int fasst_nsgt_set_timing(int on) {
  t_timing = on != 0;
  return FASST_OK;
}

int fasst_nsgt_last_ms(double *total_ms, double *fft_ms) {
  if (total_ms) *total_ms = t_ms[0];
  if (fft_ms) *fft_ms = t_ms[1];
  return FASST_OK;
}

}  // extern "C"
