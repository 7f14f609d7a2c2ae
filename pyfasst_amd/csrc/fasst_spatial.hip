// The spatial package on MI355X (gfx950), FP64: spatial/steering_vectors.py and
// spatial/dirdiag.py of the reference (include/fasst_spatial.h).
//
//   k_steer_ula      far-field steering vectors of a uniform linear array, one
//                    thread per (theta, sensor, bin).
//   k_steer_acous    near-field steering vectors with the 1 / r gains.
//   k_cx_tmean,      per-bin time mean of the four resident Cx planes: one
//   k_cx_tmean_fin   block per (chunk of kTmFrames frames, tile of 256 bins),
//                    bins along the lanes (the planes are frame-major, so every
//                    load is a coalesced row segment), each thread summing its
//                    chunk in ascending frame order; the combine sums the
//                    chunks in ascending order and divides by T.  The split
//                    depends on T alone, so two runs give the same bits.
//   k_capon_diagram  Capon directivity diagram, one thread per (theta, bin), the
//                    steering pair formed in registers.
//   k_ula_response   response of a given filter over the angles, one thread
//                    per (theta, bin), the sensors summed in ascending order.
//   k_mvdr_target    make_MVDR_filter_target for stereo, one thread per bin.
//
// k_cx_tmean streams 4 T F doubles once and is bound by HBM; the others are
// bound by the sine / cosine pairs they evaluate.  The expressions follow
// NumPy's operation order with contraction off: the phase handed to sincos is
// the reference's own, bit for bit.
#include "fasst_ctx.h"
#include "fasst_device.h"
#include "../../include/fasst_spatial.h"

#include <atomic>
#include <climits>
#include <cmath>

namespace fasst {

static std::atomic<long> g_sp_launches[FASST_SPATIAL_NK];
static std::atomic<long> g_sp_bytes{0};
static float g_sp_ms[FASST_SPATIAL_NK] = {0.f};

constexpr double kMinusTwoPi = -6.283185307179586;  // -1j * 2. * np.pi

// phase of sensor m at frequency fr (steering_vectors.py:48-52):
// (((-2 pi) * (m * fr)) * (d / c)) * sin(theta), the products in that order
__device__ __forceinline__ double ula_phase(int m, double fr, double k, double s) {
#pragma clang fp contract(off)
  const double mf = (double)m * fr;
  const double y = kMinusTwoPi * mf;
  const double yk = y * k;
  return yk * s;
}

__device__ __forceinline__ double2 cexp_i(double y) {
  double s, c;
  sincos(y, &s, &c);
  return make_double2(c, s);
}

// NumPy's complex128 division
__device__ __forceinline__ double2 np_cdiv(double2 a, double2 b) {
#pragma clang fp contract(off)
  const double br = fabs(b.x), bi = fabs(b.y);
  if (br >= bi) {
    if (br == 0.0 && bi == 0.0) return make_double2(a.x / br, a.y / bi);
    const double rat = b.y / b.x;
    const double scl = 1.0 / (b.x + b.y * rat);
    return make_double2((a.x + a.y * rat) * scl, (a.y - a.x * rat) * scl);
  }
  const double rat = b.x / b.y;
  const double scl = 1.0 / (b.y + b.x * rat);
  return make_double2((a.x * rat + a.y) * scl, (a.y * rat - a.x) * scl);
}

// NumPy's complex128 product
__device__ __forceinline__ double2 np_cmul(double2 a, double2 b) {
#pragma clang fp contract(off)
  const double re = a.x * b.x - a.y * b.y;
  const double im = a.x * b.y + a.y * b.x;
  return make_double2(re, im);
}

// ---------------------------------------------------------- steering vectors
struct SteerArgs {
  const double *freqs;  // [F]
  const double *par;    // ULA: sin(theta) [ntheta]; near field: dist [nch]
  double2 *out;         // ULA: [ntheta][nch][F]; near field: [nch][F]
  double k;             // ULA: d / c; near field: c
  double sqrt4pi;
  int nch, F, ntheta;
};

__global__ __launch_bounds__(256) void k_steer_ula(const SteerArgs a) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  const int m = blockIdx.y % a.nch, th = blockIdx.y / a.nch;
  const double y = ula_phase(m, a.freqs[f], a.k, a.par[th]);
  a.out[((size_t)th * a.nch + m) * a.F + f] = cexp_i(y);
}

__global__ __launch_bounds__(256) void k_steer_acous(const SteerArgs a) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  const int m = blockIdx.y;
  const double d = a.par[m];
  const double g = 1.0 / (a.sqrt4pi * d);
  // complex / real in NumPy: a product with the reciprocal
  const double df = d * a.freqs[f];
  const double y = kMinusTwoPi * df;
  const double scl = 1.0 / a.k;
  const double2 e = cexp_i(y * scl);
  a.out[(size_t)m * a.F + f] = make_double2(g * e.x, g * e.y);
}

// ------------------------------------------------------------- Cx time mean
constexpr int kTmFrames = 64, kTmBins = 256;

struct TmArgs {
  const double *cx;  // 4 planes [Tp][Fp]: Cx00, Cx11, Re Cx01, Im Cx01
  double *part;      // [nchunks][4][F]
  double *mean;      // [4][F]: Cx00, Re Cx01, Im Cx01, Cx11
  double *dd;        // [2][F]: Cx00, Cx11   (k_inv_herm's operand layout)
  double2 *doff;     // [F]
  size_t plane;
  int F, T, Fp, nchunks, ntiles;
};

__global__ __launch_bounds__(kTmBins) void k_cx_tmean(const TmArgs a) {
  const int c = blockIdx.x / a.ntiles;
  const int f = (blockIdx.x % a.ntiles) * kTmBins + threadIdx.x;
  if (f >= a.F) return;
  const int t0 = c * kTmFrames;
  const int nt = min(kTmFrames, a.T - t0);
  const double *p = a.cx + (size_t)t0 * a.Fp + f;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 8
  for (int t = 0; t < nt; ++t) {
    const double *q = p + (size_t)t * a.Fp;
    s0 += q[0];
    s1 += q[a.plane];
    s2 += q[2 * a.plane];
    s3 += q[3 * a.plane];
  }
  double *o = a.part + (size_t)c * 4 * a.F + f;
  o[0] = s0;
  o[a.F] = s1;
  o[2 * (size_t)a.F] = s2;
  o[3 * (size_t)a.F] = s3;
}

__global__ __launch_bounds__(256) void k_cx_tmean_fin(const TmArgs a) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < a.nchunks; ++c) {
    const double *o = a.part + (size_t)c * 4 * a.F + f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += o[(size_t)q * a.F];
  }
  const double n = (double)a.T;
  const double m00 = s[0] / n, m11 = s[1] / n, mre = s[2] / n, mim = s[3] / n;
  a.mean[f] = m00;
  a.mean[(size_t)a.F + f] = mre;
  a.mean[2 * (size_t)a.F + f] = mim;
  a.mean[3 * (size_t)a.F + f] = m11;
  a.dd[f] = m00;
  a.dd[(size_t)a.F + f] = m11;
  a.doff[f] = make_double2(mre, mim);
}

// ------------------------------------------------------------ Capon diagram
struct CaponArgs {
  const double *freqs;      // [F]
  const double *sin_theta;  // [ntheta]
  const double *idiag;      // [2][F]
  const double2 *ioff;      // [F]
  double *out;              // [ntheta][F]
  double k;
  int F, ntheta;
};

__global__ __launch_bounds__(256) void k_capon_diagram(const CaponArgs a) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  const int th = blockIdx.y;
  const double fr = a.freqs[f], s = a.sin_theta[th];
  const double2 a0 = cexp_i(ula_phase(0, fr, a.k, s)), a1 = cexp_i(ula_phase(1, fr, a.k, s));
  const double i00 = a.idiag[f], i11 = a.idiag[(size_t)a.F + f];
  const double2 io = a.ioff[f];
  // np.abs(filt ** 2), as written (steering_vectors.py:152-153)
  const double2 q0 = np_cmul(a0, a0), q1 = np_cmul(a1, a1);
  const double p0 = np_cabs(q0.x, q0.y) * i00;
  const double p1 = np_cabs(q1.x, q1.y) * i11;
  const double2 cr = np_cmul(np_cmul(cconj(a0), a1), io);
  a.out[(size_t)th * a.F + f] = (p0 + p1) + 2.0 * cr.x;
}

// ------------------------------------------------- filter response over angles
struct RespArgs {
  const double *freqs;      // [F]
  const double *sin_theta;  // [ntheta]
  const double2 *w;         // [n][F]
  double *out;              // [ntheta][F]
  double k, sqrtn;
  int n, F, ntheta;
};

__global__ __launch_bounds__(256) void k_ula_response(const RespArgs a) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  const int th = blockIdx.y;
  const double fr = a.freqs[f], s = a.sin_theta[th];
  const double scl = 1.0 / a.sqrtn;  // complex / real in NumPy
  double2 acc = make_double2(0.0, 0.0);
  for (int m = 0; m < a.n; ++m) {
    const double2 e = cexp_i(ula_phase(m, fr, a.k, s));
    const double2 v = np_cmul(a.w[(size_t)m * a.F + f], make_double2(e.x * scl, e.y * scl));
    acc.x += v.x;
    acc.y += v.y;
  }
  const double r = np_cabs(acc.x, acc.y);
  a.out[(size_t)th * a.F + f] = r * r;
}

// -------------------------------------------------- make_MVDR_filter_target
struct MvdrArgs {
  const double2 *target;  // [F][2]
  const double2 *interf;  // [n_interf][F][2]
  double2 *w;             // [2][F]
  int F, n_interf;
};

__global__ __launch_bounds__(256) void k_mvdr_target(const MvdrArgs a) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  const double2 t0 = a.target[2 * (size_t)f], t1 = a.target[2 * (size_t)f + 1];
  double s0 = 0.0, s1 = 0.0;
  double2 so = make_double2(0.0, 0.0);
  for (int i = 0; i < a.n_interf; ++i) {
    const double2 u = a.interf[((size_t)i * a.F + f) * 2], v = a.interf[((size_t)i * a.F + f) * 2 + 1];
    const double mu = np_cabs(u.x, u.y), mv = np_cabs(v.x, v.y);
    const double2 c = np_cmul(u, cconj(v));
    if (i == 0) {  // np.sum over axis 0 starts from the first row
      s0 = mu * mu;
      s1 = mv * mv;
      so = c;
    } else {
      s0 += mu * mu;
      s1 += mv * mv;
      so.x += c.x;
      so.y += c.y;
    }
  }
  const double m0 = np_cabs(t0.x, t0.y), m1 = np_cabs(t1.x, t1.y);
  const double r0 = m0 * m0 + s0, r1 = m1 * m1 + s1;
  const double2 tc = np_cmul(t0, cconj(t1));
  const double2 ro = make_double2(tc.x + so.x, tc.y + so.y);
  // invHermMat2D (tools/signalTools.py:120-131): no determinant floor
  const double mo = np_cabs(ro.x, ro.y);
  const double det = r0 * r1 - mo * mo;
  const double i00 = r1 / det, i11 = r0 / det;
  const double2 i01 = np_cdiv(make_double2(-ro.x, -ro.y), make_double2(det, 0.0));
  const double2 a00 = np_cmul(make_double2(i00, 0.0), t0), a01 = np_cmul(i01, t1);
  const double2 a10 = np_cmul(cconj(i01), t0), a11 = np_cmul(make_double2(i11, 0.0), t1);
  const double2 w0 = make_double2(a00.x + a01.x, a00.y + a01.y);
  const double2 w1 = make_double2(a10.x + a11.x, a10.y + a11.y);
  const double2 n0 = np_cmul(w0, cconj(t0)), n1 = np_cmul(w1, cconj(t1));
  const double2 nrm = make_double2(n0.x + n1.x, n0.y + n1.y);
  a.w[f] = cconj(np_cdiv(w0, nrm));
  a.w[(size_t)a.F + f] = cconj(np_cdiv(w1, nrm));
}

// ----------------------------------------------------------------- host side
// the launches of one slot between tm.start() and here; returns once they ran
static int finish_launch(int slot, int n_kernels, Events &tm, hipStream_t stream) {
  FASST_LAUNCH_CHECK();
  g_sp_launches[slot] += n_kernels;
  return elapsed_ms(tm.e[0], tm.e[1], stream, &g_sp_ms[slot]);
}

// DBuf's upload / get, counted into fasst_spatial_transfer_bytes
template <typename T>
static int sp_send(DBuf<T> &d, const void *h, size_t n) {
  FASST_TRY(d.upload(h, n));
  g_sp_bytes += (long)(n * sizeof(T));
  return FASST_OK;
}

template <typename T>
static int sp_fetch(void *h, const DBuf<T> &d, size_t n) {
  FASST_TRY(d.get(h, n));
  g_sp_bytes += (long)(n * sizeof(T));
  return FASST_OK;
}

static int bin_blocks(int F) { return (F + 255) / 256; }

// a grid of bin_blocks(F) x rows blocks, and an output of rows x F elements
static bool grid_ok(const char *what, int F, long rows) {
  if (F < 1 || rows < 1) {
    set_error("%s: bad shape (F %d, rows %ld)", what, F, rows);
    return false;
  }
  if (rows > 65535) {
    set_error("%s: %ld rows exceed the grid (65535)", what, rows);
    return false;
  }
  return true;
}

// the mean of the resident planes into work buffers of the caller
struct MeanWork {
  DBuf<double> part, mean, dd;
  DBuf<double2> doff;
};

static int run_cx_tmean(fasst_ctx *c, MeanWork &w) {
  if (!c->cx_ready || !c->cx.p) {
    set_error("cx_tmean: the model has no observation yet");
    return FASST_ERR_SHAPE;
  }
  TmArgs a;
  a.F = c->F;
  a.T = c->T;
  a.Fp = c->Fp;
  a.plane = (size_t)c->Tp * c->Fp;
  a.nchunks = (c->T + kTmFrames - 1) / kTmFrames;
  a.ntiles = (c->F + kTmBins - 1) / kTmBins;
  if ((long)a.nchunks * a.ntiles > INT_MAX) {
    set_error("cx_tmean: %d bins x %d frames exceed the grid", c->F, c->T);
    return FASST_ERR_SHAPE;
  }
  int st;
  if ((st = w.part.alloc_uninit((size_t)a.nchunks * 4 * c->F)) ||
      (st = w.mean.alloc_uninit((size_t)4 * c->F)) || (st = w.dd.alloc_uninit((size_t)2 * c->F)) ||
      (st = w.doff.alloc_uninit((size_t)c->F)))
    return st;
  a.cx = c->cx.p;
  a.part = w.part.p;
  a.mean = w.mean.p;
  a.dd = w.dd.p;
  a.doff = w.doff.p;
  Events tm;
  if ((st = tm.start(c->stream))) return st;
  k_cx_tmean<<<a.nchunks * a.ntiles, kTmBins, 0, c->stream>>>(a);
  k_cx_tmean_fin<<<bin_blocks(c->F), 256, 0, c->stream>>>(a);
  return finish_launch(FASST_SPATIAL_K_CX_TMEAN, 2, tm, c->stream);
}

}  // namespace fasst

using namespace fasst;

extern "C" {

int fasst_spatial_launch_count(long *counts) {
  if (!counts) return FASST_ERR_SHAPE;
  for (int i = 0; i < FASST_SPATIAL_NK; ++i) counts[i] = g_sp_launches[i].load();
  return FASST_OK;
}

int fasst_spatial_last_ms(double *ms) {
  if (!ms) return FASST_ERR_SHAPE;
  for (int i = 0; i < FASST_SPATIAL_NK; ++i) ms[i] = g_sp_ms[i];
  return FASST_OK;
}

int fasst_spatial_transfer_bytes(long *bytes) {
  if (!bytes) return FASST_ERR_SHAPE;
  *bytes = g_sp_bytes.load();
  return FASST_OK;
}

int fasst_steer_ula(int device, int nch, int F, int ntheta, const double *freqs,
                    const double *sin_theta, double k, double *out) {
  if (nch < 1 || ntheta < 1 || !freqs || !sin_theta || !out) {
    set_error("steer_ula: bad shape (nch %d, ntheta %d) or null argument", nch, ntheta);
    return FASST_ERR_SHAPE;
  }
  if (!grid_ok("steer_ula", F, (long)nch * ntheta)) return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  DBuf<double> dfr, dsn;
  DBuf<double2> dout;
  const size_t nout = (size_t)ntheta * nch * F;
  if ((st = sp_send(dfr, freqs, (size_t)F)) || (st = sp_send(dsn, sin_theta, (size_t)ntheta)) ||
      (st = dout.alloc_uninit(nout)))
    return st;
  SteerArgs a;
  a.freqs = dfr.p;
  a.par = dsn.p;
  a.out = dout.p;
  a.k = k;
  a.sqrt4pi = 0.0;
  a.nch = nch;
  a.F = F;
  a.ntheta = ntheta;
  Events tm;
  if ((st = tm.start(0))) return st;
  k_steer_ula<<<dim3(bin_blocks(F), nch * ntheta), 256>>>(a);
  if ((st = finish_launch(FASST_SPATIAL_K_STEER_ULA, 1, tm, 0))) return st;
  return sp_fetch(out, dout, nout);
}

int fasst_steer_acous(int device, int nch, int F, const double *freqs, const double *dist,
                      double celerity, double *out) {
  if (!freqs || !dist || !out) {
    set_error("steer_acous: null argument");
    return FASST_ERR_SHAPE;
  }
  if (!grid_ok("steer_acous", F, nch)) return FASST_ERR_SHAPE;
  DeviceGuard g(device);
  int st;
  DBuf<double> dfr, dds;
  DBuf<double2> dout;
  const size_t nout = (size_t)nch * F;
  if ((st = sp_send(dfr, freqs, (size_t)F)) || (st = sp_send(dds, dist, (size_t)nch)) ||
      (st = dout.alloc_uninit(nout)))
    return st;
  SteerArgs a;
  a.freqs = dfr.p;
  a.par = dds.p;
  a.out = dout.p;
  a.k = celerity;
  a.sqrt4pi = std::sqrt(4.0 * 3.141592653589793);
  a.nch = nch;
  a.F = F;
  a.ntheta = 1;
  Events tm;
  if ((st = tm.start(0))) return st;
  k_steer_acous<<<dim3(bin_blocks(F), nch), 256>>>(a);
  if ((st = finish_launch(FASST_SPATIAL_K_STEER_ACOUS, 1, tm, 0))) return st;
  return sp_fetch(out, dout, nout);
}

int fasst_cx_tmean(fasst_ctx *c, double *mean) {
  if (!c || !mean) {
    set_error("cx_tmean: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  MeanWork w;
  int st;
  if ((st = run_cx_tmean(c, w))) return st;
  return sp_fetch(mean, w.mean, (size_t)4 * c->F);
}

int fasst_dir_diag(fasst_ctx *c, int ntheta, const double *freqs, const double *sin_theta,
                   double k, double *diagram, double *det, double *mean) {
  if (!c || !freqs || !sin_theta || !diagram || !det) {
    set_error("dir_diag: null argument");
    return FASST_ERR_SHAPE;
  }
  if (!grid_ok("dir_diag", c->F, ntheta)) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const int F = c->F;
  int st;
  MeanWork w;
  DBuf<double> dfr, dsn, did, ddet, dout;
  DBuf<double2> dioff;
  if ((st = sp_send(dfr, freqs, (size_t)F)) || (st = sp_send(dsn, sin_theta, (size_t)ntheta)) ||
      (st = did.alloc_uninit((size_t)2 * F)) || (st = ddet.alloc_uninit((size_t)F)) ||
      (st = dioff.alloc_uninit((size_t)F)) || (st = dout.alloc_uninit((size_t)ntheta * F)))
    return st;
  if ((st = run_cx_tmean(c, w))) return st;
  if ((st = launch_inv_herm(F, w.dd.p, w.doff.p, did.p, dioff.p, ddet.p, c->stream))) return st;
  CaponArgs a;
  a.freqs = dfr.p;
  a.sin_theta = dsn.p;
  a.idiag = did.p;
  a.ioff = dioff.p;
  a.out = dout.p;
  a.k = k;
  a.F = F;
  a.ntheta = ntheta;
  Events tm;
  if ((st = tm.start(c->stream))) return st;
  k_capon_diagram<<<dim3(bin_blocks(F), ntheta), 256, 0, c->stream>>>(a);
  if ((st = finish_launch(FASST_SPATIAL_K_CAPON, 1, tm, c->stream))) return st;
  if ((st = sp_fetch(diagram, dout, (size_t)ntheta * F)) || (st = sp_fetch(det, ddet, (size_t)F)))
    return st;
  if (mean && (st = sp_fetch(mean, w.mean, (size_t)4 * F))) return st;
  return FASST_OK;
}

int fasst_ula_response(int device, int n, int F, int ntheta, const double *w, const double *freqs,
                       const double *sin_theta, double k, double *diagram) {
  if (n < 1 || !w || !freqs || !sin_theta || !diagram) {
    set_error("ula_response: bad shape (n %d) or null argument", n);
    return FASST_ERR_SHAPE;
  }
  if (!grid_ok("ula_response", F, ntheta)) return FASST_ERR_SHAPE;
  if (n > FASST_SPATIAL_MAX_SENSORS) {
    set_error("ula_response: %d sensors > %d", n, FASST_SPATIAL_MAX_SENSORS);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(device);
  int st;
  DBuf<double> dfr, dsn, dout;
  DBuf<double2> dw;
  const size_t nout = (size_t)ntheta * F;
  if ((st = sp_send(dfr, freqs, (size_t)F)) || (st = sp_send(dsn, sin_theta, (size_t)ntheta)) ||
      (st = sp_send(dw, w,(size_t)n * F)) || (st = dout.alloc_uninit(nout)))
    return st;
  RespArgs a;
  a.freqs = dfr.p;
  a.sin_theta = dsn.p;
  a.w = dw.p;
  a.out = dout.p;
  a.k = k;
  a.sqrtn = std::sqrt((double)n);
  a.n = n;
  a.F = F;
  a.ntheta = ntheta;
  Events tm;
  if ((st = tm.start(0))) return st;
  k_ula_response<<<dim3(bin_blocks(F), ntheta), 256>>>(a);
  if ((st = finish_launch(FASST_SPATIAL_K_ULA_RESPONSE, 1, tm, 0))) return st;
  return sp_fetch(diagram, dout, nout);
}

int fasst_mvdr_target(int device, int F, int n_interf, const double *target, const double *interf,
                      double *w) {
  if (F < 1 || n_interf < 0 || !target || (n_interf > 0 && !interf) || !w) {
    set_error("mvdr_target: bad shape (F %d, n_interf %d) or null argument", F, n_interf);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  int st;
  DBuf<double2> dt, di, dw;
  if ((st = sp_send(dt, target,(size_t)2 * F)) ||
      (n_interf > 0 && (st = sp_send(di, interf,(size_t)n_interf * 2 * F))) ||
      (st = dw.alloc_uninit((size_t)2 * F)))
    return st;
  MvdrArgs a;
  a.target = dt.p;
  a.interf = di.p;
  a.w = dw.p;
  a.F = F;
  a.n_interf = n_interf;
  Events tm;
  if ((st = tm.start(0))) return st;
  k_mvdr_target<<<bin_blocks(F), 256>>>(a);
  if ((st = finish_launch(FASST_SPATIAL_K_MVDR_TARGET, 1, tm, 0))) return st;
  return sp_fetch(w, dw, (size_t)2 * F);
}

}  // extern "C"
