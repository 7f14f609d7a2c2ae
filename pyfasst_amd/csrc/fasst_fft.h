// Radix-2 complex FFT in LDS (FP64) shared by the STFT / iSTFT and the
// CQT / MinQT kernels, plus the host-side twiddle tables.
#pragma once
#include "fasst_common.h"

#include <cmath>

namespace fasst {

// In-LDS complex FFT of size N (power of two), data already in bit-reversed
// order.  tw[k] = exp(sign * 2 pi i k / N), k < N/2.
__device__ inline void lds_fft(double2 *x, const double2 *__restrict__ tw, int N, int logN) {
  for (int s = 0; s < logN; ++s) {
    const int m = 1 << s;
    const int stride = N >> (s + 1);
    for (int b = threadIdx.x; b < (N >> 1); b += blockDim.x) {
      const int grp = b >> s, pos = b & (m - 1);
      const int i0 = grp * 2 * m + pos, i1 = i0 + m;
      const double2 w = tw[pos * stride];
      const double2 u = x[i0], v = x[i1];
      const double2 t = make_double2(w.x * v.x - w.y * v.y, w.x * v.y + w.y * v.x);
      x[i0] = make_double2(u.x + t.x, u.y + t.y);
      x[i1] = make_double2(u.x - t.x, u.y - t.y);
    }
    __syncthreads();
  }
}

// `count` independent FFTs of size N laid end to end in LDS (x[c * N + i]), the
// butterflies of all of them spread over the block; count == 1 is lds_fft.
__device__ inline void lds_fft_batch(double2 *x, const double2 *__restrict__ tw, int N, int logN,
                                     int count) {
  const int half = N >> 1, total = half * count;
  for (int s = 0; s < logN; ++s) {
    const int m = 1 << s;
    const int stride = N >> (s + 1);
    for (int b = threadIdx.x; b < total; b += blockDim.x) {
      const int which = b >> (logN - 1), bb = b & (half - 1);
      const int grp = bb >> s, pos = bb & (m - 1);
      const int i0 = which * N + grp * 2 * m + pos, i1 = i0 + m;
      const double2 w = tw[pos * stride];
      const double2 u = x[i0], v = x[i1];
      const double2 t = make_double2(w.x * v.x - w.y * v.y, w.x * v.y + w.y * v.x);
      x[i0] = make_double2(u.x + t.x, u.y + t.y);
      x[i1] = make_double2(u.x - t.x, u.y - t.y);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int bitrev(int i, int logN) { return (int)(__brev((unsigned)i) >> (32 - logN)); }

// twiddles exp(sign 2 pi i k / N), k < N/2, computed on the host in long double
static inline std::vector<double2> twiddles(int N, int sign) {
  std::vector<double2> tw(N / 2);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int k = 0; k < N / 2; ++k) {
    const long double ang = 2.0L * pi * (long double)k / (long double)N;
    tw[k] = make_double2((double)cosl(ang), (double)(sign * sinl(ang)));
  }
  return tw;
}

static inline int ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return (1 << l) == n ? l : -1;
}

// Host side of the fasst_tf.hip kernels for the other translation units (HIP
// kernels do not link across TUs without -fgpu-rdc).  A separation call is an
// image producer followed by one of the sinks below or cqt_inverse_batch.
// [nm][F][T] (host order) -> [nm][Tp][Fp] (frame-major, bins contiguous)
int tf_launch_ft_to_tf(hipStream_t s, const double2 *src, double2 *dst, int F, int T, int Fp,
                       int Tp, int nm);

// iSTFT of frame-major images (T rows of `ld` bins) into len_out() samples each
// (tftransforms/stft.py:71-131).  init refuses a bad geometry before it
// allocates, and owns what the images share: the windows (analysis_window
// nullptr: the window), the +1 twiddles of nfft and the [T][wlen] frames.
struct IstftSink {
  int init(hipStream_t s, const double *window, const double *analysis_window, int wlen, int nfft,
           int hop, int T, bool simm = false);   // simm: fasst_istft_simm's overlap-add
  int len_out() const { return hop * (T - 1) + wlen - (simm ? 0 : wlen / 2); }
  int run(const double2 *S, int ld, double *y_dev);
  // the image g0 X0 + g1 X1 (X [2] planes `plane` apart), formed as a frame is loaded
  int run_gain(const double2 *X, size_t plane, int ld, const double2 *g0, const double2 *g1,
               double *y_dev);

  hipStream_t s = nullptr;
  int wlen = 0, nfft = 0, hop = 0, T = 0;
  bool simm = false;
  std::vector<double2> tw;   // outlives its asynchronous upload
  DBuf<double> dw, daw, dframes;
  DBuf<double2> dtw;
  int ola(double *y_dev);
};

// `nimg` images `plane` apart through the sink into y_host [nimg][len_out()];
// n [Tp][Fp] planes into S_host [n][F][T].  Both drain the stream.
int images_to_waveforms(IstftSink &sink, const double2 *S, size_t plane, int ld, int nimg,
                        double *y_host);
int images_to_host(hipStream_t s, const double2 *dS, int n, int F, int T, int Fp, int Tp,
                   double *S_host);

}  // namespace fasst
