// SIMM source dictionary (KLGLOTT88 harmonic combs) on MI355X (gfx950), FP64.
//
// generate_WF0_TR_chirped (separateLeadFunctions.py:696-886) synthesises, for
// each of ~1100 F0s, a complex harmonic sum of up to Fs/(2 F0) partials over
// 2 NFT samples and keeps the power spectrum of ONE frame of its STFT: the
// reference materialises the full partials x samples outer product per F0
// ("Horribly slow", :744).  Here one workgroup per column synthesises only
// the wlen samples of that frame -- each sample's partial sum in the
// reference's order, with the reference's phase expression evaluated in the
// same double operations -- windows them into LDS and runs the radix-2 FFT in
// LDS; the column of |X|^2 is written straight into WF0.
#include "fasst_fft.h"
#include "fasst_odgd.h"
#include "../../include/fasst_dict.h"

#include <algorithm>
#include <cmath>

namespace fasst {

struct DictArgs {
  const double *f1, *f2;
  const int *np_;
  const double2 *amps;   // [n_cols][max_partials]
  const double *win;
  const double2 *tw;
  double *wf0;           // [nfft/2+1][n_cols]
  double fs;
  long frame_start;
  int n_cols, max_partials, length_odgd, wlen, nfft, logn;
};

__global__ __launch_bounds__(256) void k_wf0_column(const DictArgs a) {
  extern __shared__ __attribute__((aligned(16))) double2 sm[];
  double2 *buf = sm;                 // [nfft]
  double2 *amp = sm + a.nfft;        // [max_partials]
  const int j = blockIdx.x;
  const int P = a.np_[j];
  const double F1 = a.f1[j], F2 = a.f2[j];
  for (int h = threadIdx.x; h < P; h += blockDim.x) amp[h] = a.amps[(size_t)j * a.max_partials + h];
  __syncthreads();
  const double den = 2.0 * (double)a.length_odgd / a.fs;
  for (int i = threadIdx.x; i < a.nfft; i += blockDim.x) {
    double v = 0.0;
    const long t = a.frame_start + i;
    if (i < a.wlen && t >= 0 && t < a.length_odgd)
      v = a.win[i] * odgd_sample(amp, P, F1, F2, a.fs, den, t).x;
    buf[bitrev(i, a.logn)] = make_double2(v, 0.0);
  }
  __syncthreads();
  lds_fft(buf, a.tw, a.nfft, a.logn);
  for (int k = threadIdx.x; k <= a.nfft / 2; k += blockDim.x) {
    const double m = hypot(buf[k].x, buf[k].y);      // np.abs(X) ** 2
    a.wf0[(size_t)k * a.n_cols + j] = m * m;
  }
}

// The public ODGD family (generate_ODGD_spec :888-949, _chirped :1010-1072,
// generate_WF0_chirped :237-345): per column the whole complex waveform at
// ts = n / fs + t_off, the full nfft-point spectrum of Re(odgd * window)
// (cropped to the first nfft samples or zero-padded, as np.fft.fft(x, n) does)
// and its power.  The windowed signal is real: bins 0 .. nfft/2 come out of
// the LDS FFT and the upper half is their Hermitian mirror, so power[k] and
// power[nfft - k] are the same double.  Columns pick their window by index
// (generate_WF0_chirped mixes two).
struct OdgdArgs {
  const double *f1, *f2, *toff;
  const int *np_, *wsel;
  const double2 *amps;   // [n_cols][max_partials]
  const double *win;     // [n_windows][length_odgd]
  const double2 *tw;
  double2 *odgd;         // [n_cols][length_odgd] or null
  double2 *spec;         // [n_cols][nfft] or null
  double *power;         // [nfft][n_cols] or null
  double fs;
  int n_cols, max_partials, length_odgd, nfft, logn;
};

__global__ __launch_bounds__(256) void k_odgd_column(const OdgdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double2 sm[];
  double2 *buf = sm;                 // [nfft]
  double2 *amp = sm + a.nfft;        // [max_partials]
  const int j = blockIdx.x;
  const int P = a.np_[j];
  const double F1 = a.f1[j], F2 = a.f2[j], t_off = a.toff[j];
  const int L = a.length_odgd;
  const bool transform = a.spec || a.power;
  for (int h = threadIdx.x; h < P; h += blockDim.x) amp[h] = a.amps[(size_t)j * a.max_partials + h];
  __syncthreads();
  const double den = 2.0 * (double)L / a.fs;
  const double *win = a.win + (size_t)a.wsel[j] * L;
  // samples past nfft only matter to the waveform
  const int n_syn = a.odgd ? L : min(L, a.nfft);
  const int n_buf = transform ? a.nfft : 0;
  for (int i = threadIdx.x; i < max(n_syn, n_buf); i += blockDim.x) {
    double v = 0.0;
    if (i < n_syn) {
      const double2 z = odgd_sample_at(amp, P, F1, F2, den, (double)i / a.fs + t_off);
      if (a.odgd) a.odgd[(size_t)j * L + i] = z;
      v = z.x * win[i];
    }
    if (i < n_buf) buf[bitrev(i, a.logn)] = make_double2(v, 0.0);
  }
  if (!transform) return;
  __syncthreads();
  lds_fft(buf, a.tw, a.nfft, a.logn);
  const int N = a.nfft;
  for (int k = threadIdx.x; k <= N / 2; k += blockDim.x) {
    double2 X = buf[k];
    if (k == 0 || 2 * k == N) X.y = 0.0;   // real input: DC and Nyquist are real
    const int km = (N - k) & (N - 1);      // mirror bin (k itself for DC and Nyquist)
    if (a.spec) {
      a.spec[(size_t)j * N + k] = X;
      if (km != k) a.spec[(size_t)j * N + km] = make_double2(X.x, -X.y);
    }
    if (a.power) {
      const double m = hypot(X.x, X.y);    // np.abs(X) ** 2
      a.power[(size_t)k * a.n_cols + j] = m * m;
      if (km != k) a.power[(size_t)km * a.n_cols + j] = m * m;
    }
  }
}

static float g_dict_ms = 0.f;

}  // namespace fasst

using namespace fasst;

extern "C" {

int dict_wf0_stft(int device, int n_cols, const double *f1, const double *f2,
                  const int *n_partials, int max_partials, const double *amps, double fs,
                  int length_odgd, const double *window, int wlen, int nfft, long frame_start,
                  double *wf0) {
  if (n_cols < 1 || max_partials < 1 || !f1 || !f2 || !n_partials || !amps || !window || !wf0 ||
      ilog2(nfft) < 1 || nfft > 8192 || wlen < 1 || wlen > nfft || length_odgd < 1 || fs <= 0) {
    set_error("dict_wf0_stft: bad shape (cols %d, partials %d, nfft %d, wlen %d)", n_cols,
              max_partials, nfft, wlen);
    return FASST_ERR_SHAPE;
  }
  for (int j = 0; j < n_cols; ++j)
    if (n_partials[j] < 0 || n_partials[j] > max_partials) {
      set_error("dict_wf0_stft: column %d has %d partials > %d", j, n_partials[j], max_partials);
      return FASST_ERR_SHAPE;
    }
  const size_t smem = ((size_t)nfft + max_partials) * sizeof(double2);
  if (smem > 160 * 1024) {
    set_error("dict_wf0_stft: nfft %d + %d partials exceed the LDS", nfft, max_partials);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  int st;
  const int F = nfft / 2 + 1;
  DBuf<double> d1, d2, dw, dout;
  DBuf<int> dnp;
  DBuf<double2> damps, dtw;
  auto tw = twiddles(nfft, -1);
  if ((st = dout.alloc((size_t)F * n_cols)) || (st = d1.upload(f1, n_cols)) ||
      (st = d2.upload(f2, n_cols)) || (st = dnp.upload(n_partials, n_cols)) ||
      (st = damps.upload(amps, (size_t)n_cols * max_partials)) ||
      (st = dw.upload(window, wlen)) || (st = dtw.upload(tw.data(), tw.size())))
    return st;
  if (smem > 64 * 1024)
    FASST_HIP(hipFuncSetAttribute((const void *)k_wf0_column,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  DictArgs a;
  a.f1 = d1.p;
  a.f2 = d2.p;
  a.np_ = dnp.p;
  a.amps = damps.p;
  a.win = dw.p;
  a.tw = dtw.p;
  a.wf0 = dout.p;
  a.fs = fs;
  a.frame_start = frame_start;
  a.n_cols = n_cols;
  a.max_partials = max_partials;
  a.length_odgd = length_odgd;
  a.wlen = wlen;
  a.nfft = nfft;
  a.logn = ilog2(nfft);
  Events tm;
  if ((st = tm.start(0))) return st;
  k_wf0_column<<<n_cols, 256, smem>>>(a);
  FASST_LAUNCH_CHECK();
  if ((st = elapsed_ms(tm.e[0], tm.e[1], 0, &g_dict_ms))) return st;
  return dout.get(wf0, dout.n);
}

int dict_odgd(int device, int n_cols, const double *f1, const double *f2, const int *n_partials,
              int max_partials, const double *amps, const double *t_offset, double fs,
              int length_odgd, int n_windows, const double *windows, const int *window_sel,
              int nfft, double *odgd, double *spectrum, double *power) {
  if (n_cols < 1 || max_partials < 1 || !f1 || !f2 || !n_partials || !amps || !t_offset ||
      n_windows < 1 || !windows || !window_sel || ilog2(nfft) < 1 || nfft > 8192 ||
      length_odgd < 1 || !(fs > 0) || (!odgd && !spectrum && !power)) {
    set_error("dict_odgd: bad shape (cols %d, partials %d, nfft %d not a power of two in "
              "2..8192, length %d, windows %d) or no output requested", n_cols, max_partials,
              nfft, length_odgd, n_windows);
    return FASST_ERR_SHAPE;
  }
  for (int j = 0; j < n_cols; ++j) {
    if (n_partials[j] < 0 || n_partials[j] > max_partials) {
      set_error("dict_odgd: column %d has %d partials > %d", j, n_partials[j], max_partials);
      return FASST_ERR_SHAPE;
    }
    if (window_sel[j] < 0 || window_sel[j] >= n_windows) {
      set_error("dict_odgd: column %d selects window %d of %d", j, window_sel[j], n_windows);
      return FASST_ERR_SHAPE;
    }
  }
  const size_t smem = ((size_t)nfft + max_partials) * sizeof(double2);
  if (smem > 160 * 1024) {
    set_error("dict_odgd: nfft %d + %d partials exceed the LDS", nfft, max_partials);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  int st;
  const size_t L = (size_t)length_odgd, C = (size_t)n_cols, N = (size_t)nfft;
  DBuf<double> d1, d2, dt, dw, dpow;
  DBuf<int> dnp, dsel;
  DBuf<double2> damps, dtw, dodgd, dspec;
  auto tw = twiddles(nfft, -1);
  if ((st = dodgd.alloc(odgd ? C * L : 0)) || (st = dspec.alloc(spectrum ? C * N : 0)) ||
      (st = dpow.alloc(power ? N * C : 0)) || (st = d1.upload(f1, C)) ||
      (st = d2.upload(f2, C)) || (st = dt.upload(t_offset, C)) ||
      (st = dnp.upload(n_partials, C)) || (st = dsel.upload(window_sel, C)) ||
      (st = damps.upload(amps, C * max_partials)) ||
      (st = dw.upload(windows, (size_t)n_windows * L)) ||
      (st = dtw.upload(tw.data(), tw.size())))
    return st;
  if (smem > 64 * 1024)
    FASST_HIP(hipFuncSetAttribute((const void *)k_odgd_column,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  OdgdArgs a;
  a.f1 = d1.p;
  a.f2 = d2.p;
  a.toff = dt.p;
  a.np_ = dnp.p;
  a.wsel = dsel.p;
  a.amps = damps.p;
  a.win = dw.p;
  a.tw = dtw.p;
  a.odgd = dodgd.p;
  a.spec = dspec.p;
  a.power = dpow.p;
  a.fs = fs;
  a.n_cols = n_cols;
  a.max_partials = max_partials;
  a.length_odgd = length_odgd;
  a.nfft = nfft;
  a.logn = ilog2(nfft);
  Events tm;
  if ((st = tm.start(0))) return st;
  k_odgd_column<<<n_cols, 256, smem>>>(a);
  FASST_LAUNCH_CHECK();
  if ((st = elapsed_ms(tm.e[0], tm.e[1], 0, &g_dict_ms))) return st;
  // (a buffer whose output was not requested is empty: nothing is copied)
  if ((st = dodgd.get(odgd, dodgd.n)) || (st = dspec.get(spectrum, dspec.n))) return st;
  return dpow.get(power, dpow.n);
}

int dict_last_ms(double *device_ms) {
  if (device_ms) *device_ms = g_dict_ms;
  return FASST_OK;
}

}  // extern "C"
