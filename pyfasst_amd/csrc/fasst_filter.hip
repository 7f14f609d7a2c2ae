// Fused STFT-domain filtering on MI355X (tftransforms/stft.py:133-334,
// filter_stft / filter_conv_stft): analyse, multiply, overlap-add, with no
// spectrogram kept.
//
//   k_filter_frames  one block per frame.  The M_in windowed channels are
//                    packed two real channels to one complex buffer in LDS
//                    and transformed by a decimation-in-frequency FFT
//                    (natural order in, bit-reversed out).  One thread per
//                    bin pair (k, nfft-k) separates the channel spectra,
//                    applies the M_out x M_in matrix of the bin and repacks
//                    two output channels per buffer, at the same bit-reversed
//                    places; the decimation-in-time inverse (lds_fft) then
//                    needs no permutation.  Real and imaginary parts of the
//                    inverse are two channels' frames.
//   k_ola_ch         k_ola of fasst_tf.hip over the channels of
//                    frames[ch][n][wlen], into y[row][ch]
#include "fasst_common.h"
#include "fasst_fft.h"
#include "../../include/fasst_filter.h"

#include <algorithm>
#include <climits>

namespace fasst {

constexpr int kFiltRegM = FILTER_REG_M;
constexpr int kFiltMaxGridYZ = 65535;

struct FiltArgs {
  const double *x;      // [L][Min]
  const double2 *W;     // entry e = o*Min + c, bin k of frame n: W[n*w_frame + e*w_entry + k]
  size_t w_frame, w_entry;
  const double *awin, *swin;
  const double2 *twf, *twi;   // exp(-/+ 2 pi i k / N)
  double *frames;             // [Mout][nframes][wlen]
  int L, Min, Mout, wlen, N, logN, hop, nframes;
};

// lds_fft run backwards: natural order in, bit-reversed order out
__device__ inline void lds_fft_dif(double2 *x, const double2 *__restrict__ tw, int N, int logN) {
  for (int s = logN - 1; s >= 0; --s) {
    const int m = 1 << s;
    const int stride = N >> (s + 1);
    for (int b = threadIdx.x; b < (N >> 1); b += blockDim.x) {
      const int grp = b >> s, pos = b & (m - 1);
      const int i0 = grp * 2 * m + pos, i1 = i0 + m;
      const double2 w = tw[pos * stride];
      const double2 u = x[i0], v = x[i1];
      const double2 d = make_double2(u.x - v.x, u.y - v.y);
      x[i0] = make_double2(u.x + v.x, u.y + v.y);
      x[i1] = make_double2(w.x * d.x - w.y * d.y, w.x * d.y + w.y * d.x);
    }
    __syncthreads();
  }
}

// Z = FFT(a + i b), a and b real: A[k] = (Z[k] + conj Z[N-k]) / 2,
// B[k] = (Z[k] - conj Z[N-k]) / 2i
__device__ __forceinline__ void split_pair(double2 z1, double2 z2, double2 &A, double2 &B) {
  A = make_double2(0.5 * (z1.x + z2.x), 0.5 * (z1.y - z2.y));
  B = make_double2(0.5 * (z1.y + z2.y), -0.5 * (z1.x - z2.x));
}

__device__ __forceinline__ void cmac(double2 &y, double2 w, double2 x) {
  y.x += w.x * x.x - w.y * x.y;
  y.y += w.x * x.y + w.y * x.x;
}

// REG: Min <= kFiltRegM, the channel spectra of a bin pair are held in
// registers and the outputs overwrite the inputs' buffers.  Otherwise the
// outputs have buffers of their own and the spectra are re-read from LDS.
template <bool REG>
__global__ __launch_bounds__(256) void k_filter_frames(const FiltArgs a) {
  extern __shared__ __attribute__((aligned(16))) double2 fbuf[];
  const int n = blockIdx.x, N = a.N, h = N / 2, half = a.wlen / 2;
  const int Pin = (a.Min + 1) / 2, Pout = (a.Mout + 1) / 2;
  double2 *zin = fbuf;
  double2 *zout = REG ? fbuf : fbuf + (size_t)Pin * N;
  for (int p = 0; p < Pin; ++p) {
    const int c0 = 2 * p;
    const bool two = c0 + 1 < a.Min;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      double va = 0.0, vb = 0.0;
      if (i < a.wlen) {
        const long s = (long)n * a.hop + i - half;
        if (s >= 0 && s < a.L) {
          const double w = a.awin[i];
          const double *xs = a.x + (size_t)s * a.Min + c0;
          va = w * xs[0];
          if (two) vb = w * xs[1];
        }
      }
      zin[(size_t)p * N + i] = make_double2(va, vb);
    }
  }
  __syncthreads();
  for (int p = 0; p < Pin; ++p) lds_fft_dif(zin + (size_t)p * N, a.twf, N, a.logN);

  const double2 *Wn = a.W + (size_t)n * a.w_frame;
  for (int k = threadIdx.x; k <= h; k += blockDim.x) {
    const int i1 = bitrev(k, a.logN), i2 = bitrev((N - k) & (N - 1), a.logN);
    const bool edge = k == 0 || k == h;
    double2 X[kFiltRegM];
    if (REG) {
#pragma unroll
      for (int p = 0; p < kFiltRegM / 2; ++p) {
        X[2 * p] = X[2 * p + 1] = make_double2(0.0, 0.0);
        if (p < Pin) split_pair(zin[(size_t)p * N + i1], zin[(size_t)p * N + i2], X[2 * p], X[2 * p + 1]);
      }
    }
    for (int q = 0; q < Pout; ++q) {
      const int o0 = 2 * q;
      const bool two = o0 + 1 < a.Mout;
      const double2 *wa = Wn + (size_t)o0 * a.Min * a.w_entry + k;
      const double2 *wb = wa + (size_t)a.Min * a.w_entry;
      double2 Ya = make_double2(0.0, 0.0), Yb = make_double2(0.0, 0.0);
      if (REG) {
#pragma unroll
        for (int c = 0; c < kFiltRegM; ++c)
          if (c < a.Min) {
            cmac(Ya, wa[(size_t)c * a.w_entry], X[c]);
            if (two) cmac(Yb, wb[(size_t)c * a.w_entry], X[c]);
          }
      } else {
        for (int p = 0; p < Pin; ++p) {
          double2 A, B;
          split_pair(zin[(size_t)p * N + i1], zin[(size_t)p * N + i2], A, B);
          const int c = 2 * p;
          cmac(Ya, wa[(size_t)c * a.w_entry], A);
          if (two) cmac(Yb, wb[(size_t)c * a.w_entry], A);
          if (c + 1 < a.Min) {
            cmac(Ya, wa[(size_t)(c + 1) * a.w_entry], B);
            if (two) cmac(Yb, wb[(size_t)(c + 1) * a.w_entry], B);
          }
        }
      }
      // U = Ya + i Yb at k, conj(Ya) + i conj(Yb) at N-k (irfft reads bins 0
      // and N/2 as real)
      if (edge) {
        zout[(size_t)q * N + i1] = make_double2(Ya.x, Yb.x);
      } else {
        zout[(size_t)q * N + i1] = make_double2(Ya.x - Yb.y, Ya.y + Yb.x);
        zout[(size_t)q * N + i2] = make_double2(Ya.x + Yb.y, Yb.x - Ya.y);
      }
    }
  }
  __syncthreads();
  for (int q = 0; q < Pout; ++q) lds_fft(zout + (size_t)q * N, a.twi, N, a.logN);

  const double invN = 1.0 / (double)N;
  for (int q = 0; q < Pout; ++q) {
    const bool two = 2 * q + 1 < a.Mout;
    double *fa = a.frames + ((size_t)(2 * q) * a.nframes + n) * a.wlen;
    double *fb = fa + (size_t)a.nframes * a.wlen;
    for (int i = threadIdx.x; i < a.wlen; i += blockDim.x) {
      const double2 v = zout[(size_t)q * N + i];
      const double w = a.swin[i];
      fa[i] = w * (v.x * invN);
      if (two) fb[i] = w * (v.y * invN);
    }
  }
}

// k_ola (fasst_tf.hip) of channel blockIdx.y: frames [M][nframes][wlen] -> y [len_out][M]
__global__ void k_ola_ch(const double *__restrict__ frames, int nframes, int wlen, int hop,
                         const double *__restrict__ win, const double *__restrict__ awin,
                         double *__restrict__ y, int len_out, int M) {
  const int half = wlen / 2, ch = blockIdx.y;
  const double *fr = frames + (size_t)ch * nframes * wlen;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < len_out; o += gridDim.x * blockDim.x) {
    const long s = (long)o + half;
    long nlo = (s - wlen) / hop + 1;
    if (s - wlen < 0) nlo = 0;
    long nhi = s / hop;
    if (nhi > nframes - 1) nhi = nframes - 1;
    double acc = 0.0, nrm = 0.0;
    for (long n = nlo; n <= nhi; ++n) {
      const int p = (int)(s - n * hop);
      if (p < 0 || p >= wlen) continue;
      nrm = nrm + win[p] * awin[p];
      acc = acc + fr[(size_t)n * wlen + p];
    }
    y[(size_t)o * M + ch] = acc / (nrm == 0.0 ? 1.0 : nrm);
  }
}

struct FiltShape {
  int nframes, len_out;
  size_t lds;
  bool reg;
};

// Host-only validation (no device call): the framing of stft.py:155-158 and
// the LDS form of one frame.
static int filter_shape(int L, int Min, int Mout, const void *W, int w_tv, int nwf,
                        const void *awin, const void *swin, int wlen, int nfft, int hop,
                        FiltShape &s) {
  if (L < 1 || Min < 1 || Mout < 1 || !W || !awin || !swin || wlen < 2 || hop < 1 || nfft < 2) {
    set_error("filter_stft: bad shape (L %d, M_in %d, M_out %d, wlen %d, nfft %d, hop %d)", L, Min,
              Mout, wlen, nfft, hop);
    return FASST_ERR_SHAPE;
  }
  if (ilog2(nfft) < 1) {
    set_error("filter_stft: nfft=%d is not a power of two (radix-2 transforms only)", nfft);
    return FASST_ERR_UNSUPPORTED;
  }
  if (wlen > nfft || nfft > 8192) {
    set_error("filter_stft: FFT size %d must be >= wlen %d and <= 8192", nfft, wlen);
    return FASST_ERR_SHAPE;
  }
  const long nframes = ((long)L + hop - 1) / hop;
  const long framed = (nframes - 1) * hop + wlen;
  if (wlen / 2 + (long)L > framed) {
    set_error("filter_stft: hop %d leaves %ld framed samples for wlen/2 + L = %ld (negative "
              "tail padding)", hop, framed, wlen / 2 + (long)L);
    return FASST_ERR_SHAPE;
  }
  if (w_tv && nwf < nframes) {
    set_error("filter_stft: W has %d frames, the signal needs %ld", nwf, nframes);
    return FASST_ERR_SHAPE;
  }
  const long len_out = framed - wlen / 2;
  if (len_out > INT_MAX || nframes > INT_MAX) {
    set_error("filter_stft: %ld output rows exceed the index range", len_out);
    return FASST_ERR_SHAPE;
  }
  // M_out is a grid y extent (k_ola_ch), M_in * M_out a grid z extent (the W transpose)
  if (Mout > kFiltMaxGridYZ || (long)Min * Mout > kFiltMaxGridYZ) {
    set_error("filter_stft: M_in %d x M_out %d passes %d filter entries", Min, Mout,
              kFiltMaxGridYZ);
    return FASST_ERR_SHAPE;
  }
  const long Pin = (Min + 1) / 2, Pout = (Mout + 1) / 2;
  s.reg = Min <= kFiltRegM;
  const long nbuf = s.reg ? std::max(Pin, Pout) : Pin + Pout;
  if (nbuf * nfft * (long)sizeof(double2) > FILTER_LDS_BYTES) {
    set_error("filter_stft: M=%d (in) x %d (out) channels at nfft=%d need %ld complex buffers of "
              "nfft, %ld bytes of LDS; the ceiling is %d", Min, Mout, nfft, nbuf,
              nbuf * nfft * (long)sizeof(double2), FILTER_LDS_BYTES);
    return FASST_ERR_UNSUPPORTED;
  }
  s.lds = (size_t)nbuf * nfft * sizeof(double2);
  s.nframes = (int)nframes;
  s.len_out = (int)len_out;
  return FASST_OK;
}

// Kernel timing is off unless the calling thread asked for it
// (fasst_filter_set_timing); flag and results belong to that thread.
static thread_local bool t_filter_timing = false;
static thread_local double t_filter_ms = 0.0, t_filter_tr_ms = 0.0;

// Every pointer a device pointer; returns after the kernels have finished.
static int filter_run(hipStream_t st, const double *dx, int L, int Min, int Mout, const double2 *dW,
                      int w_tv, int nwf, int w_layout, const double *dawin, const double *dswin,
                      int wlen, int nfft, int hop, double *dy, const FiltShape &s) {
  int rc;
  const int F = nfft / 2 + 1, MM = Min * Mout;
  DBuf<double2> dtwf, dtwi, dWt;
  DBuf<double> dframes;
  if ((rc = dtwf.alloc_uninit(nfft / 2)) || (rc = dtwi.alloc_uninit(nfft / 2)) ||
      (rc = dframes.alloc_uninit((size_t)Mout * s.nframes * wlen)))
    return rc;
  const bool transpose = w_tv && w_layout == FILTER_W_NUMPY;
  if (transpose && (rc = dWt.alloc_uninit((size_t)MM * nwf * F))) return rc;
  const auto twf = twiddles(nfft, -1), twi = twiddles(nfft, +1);
  FASST_TRY(dtwf.put(twf.data(), twf.size(), st));
  FASST_TRY(dtwi.put(twi.data(), twi.size(), st));
  const bool timing = t_filter_timing;
  Events ev;   // start, after the transpose, end
  if (timing) {
    if ((rc = ev.create(3))) return rc;
    FASST_HIP(hipEventRecord(ev.e[0], st));
  }
  if (transpose)   // [MM][F][nwf] -> [MM][nwf][F]
    if ((rc = tf_launch_ft_to_tf(st, dW, dWt.p, F, nwf, F, nwf, MM))) return rc;
  if (timing) FASST_HIP(hipEventRecord(ev.e[1], st));
  FiltArgs a;
  a.x = dx;
  a.W = transpose ? dWt.p : dW;
  a.w_frame = w_tv ? (size_t)F : 0;
  a.w_entry = w_tv ? (size_t)nwf * F : (size_t)F;
  a.awin = dawin;
  a.swin = dswin;
  a.twf = dtwf.p;
  a.twi = dtwi.p;
  a.frames = dframes.p;
  a.L = L;
  a.Min = Min;
  a.Mout = Mout;
  a.wlen = wlen;
  a.N = nfft;
  a.logN = ilog2(nfft);
  a.hop = hop;
  a.nframes = s.nframes;
  // the dynamic-LDS ceiling is raised for the launch that needs it only
  const void *fn = s.reg ? (const void *)k_filter_frames<true> : (const void *)k_filter_frames<false>;
  if (s.lds > 64 * 1024)
    FASST_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
  if (s.reg)
    k_filter_frames<true><<<s.nframes, 256, s.lds, st>>>(a);
  else
    k_filter_frames<false><<<s.nframes, 256, s.lds, st>>>(a);
  FASST_LAUNCH_CHECK();
  k_ola_ch<<<dim3((s.len_out + 255) / 256, Mout), 256, 0, st>>>(dframes.p, s.nframes, wlen, hop,
                                                                dswin, dawin, dy, s.len_out, Mout);
  FASST_LAUNCH_CHECK();
  float t01 = 0.f, t02 = 0.f;
  if (timing && (rc = elapsed_ms(ev.e[0], ev.e[2], st, &t02))) return rc;
  FASST_HIP(hipStreamSynchronize(st));   // the scratch above is freed on return
  if (timing) {
    FASST_HIP(hipEventElapsedTime(&t01, ev.e[0], ev.e[1]));
    t_filter_ms = t02;
    t_filter_tr_ms = transpose ? t01 : 0.0;
  }
  return FASST_OK;
}

}  // namespace fasst

using namespace fasst;

extern "C" {

int fasst_filter_stft_dev(int device, const double *data, int L, int M_in, int M_out,
                          const double *W, int w_tv, int n_w_frames, const double *awin,
                          const double *swin, int wlen, int nfft, int hop, double *y_out,
                          int *len_out, int w_layout, void *stream) {
  FiltShape s;
  int rc = filter_shape(L, M_in, M_out, W, w_tv, n_w_frames, awin, swin, wlen, nfft, hop, s);
  if (rc) return rc;
  if (w_layout != FILTER_W_NUMPY && w_layout != FILTER_W_FRAMES) {
    set_error("filter_stft: unknown W layout %d", w_layout);
    return FASST_ERR_SHAPE;
  }
  if (len_out) *len_out = s.len_out;
  if (!y_out) return FASST_OK;
  if (!data) {
    set_error("filter_stft: no data");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  return filter_run((hipStream_t)stream, data, L, M_in, M_out, (const double2 *)W, w_tv,
                    n_w_frames, w_layout, awin, swin, wlen, nfft, hop, y_out, s);
}

int fasst_filter_stft(int device, const double *data, int L, int M_in, int M_out, const double *W,
                      int w_tv, int n_w_frames, const double *awin, const double *swin, int wlen,
                      int nfft, int hop, double *y_out, int *len_out) {
  FiltShape s;
  int rc = filter_shape(L, M_in, M_out, W, w_tv, n_w_frames, awin, swin, wlen, nfft, hop, s);
  if (rc) return rc;
  if (len_out) *len_out = s.len_out;
  if (!y_out) return FASST_OK;
  if (!data) {
    set_error("filter_stft: no data");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  const size_t F = nfft / 2 + 1;
  const size_t nW = (size_t)M_in * M_out * F * (w_tv ? (size_t)n_w_frames : 1);
  const size_t nx = (size_t)L * M_in, ny = (size_t)s.len_out * M_out;
  DBuf<double> dx, daw, dsw, dy;
  DBuf<double2> dW;
  if ((rc = dx.alloc_uninit(nx)) || (rc = daw.alloc_uninit(wlen)) || (rc = dsw.alloc_uninit(wlen)) ||
      (rc = dy.alloc_uninit(ny)) || (rc = dW.alloc_uninit(nW)))
    return rc;
  FASST_TRY(dx.put(data, nx));
  FASST_TRY(daw.put(awin, wlen));
  FASST_TRY(dsw.put(swin, wlen));
  FASST_TRY(dW.put(W, nW));
  if ((rc = filter_run(nullptr, dx.p, L, M_in, M_out, dW.p, w_tv, n_w_frames, FILTER_W_NUMPY, daw.p,
                       dsw.p, wlen, nfft, hop, dy.p, s)))
    return rc;
  return dy.get(y_out, ny);
}

int fasst_filter_set_timing(int on) {
  t_filter_timing = on != 0;
  return FASST_OK;
}

int fasst_filter_last_ms(double *total_ms, double *transpose_ms) {
  if (total_ms) *total_ms = t_filter_ms;
  if (transpose_ms) *transpose_ms = t_filter_tr_ms;
  return FASST_OK;
}

}  // extern "C"
