// DEMIX's device side on MI355X (gfx950), FP64: demixTF.py of the reference.
//
//   k_energy_max1/2   lexicographic complex maximum of mean(X**2) over the
//                     cropped frames (two stages, fixed order)
//   k_features        confidence, theta, phi, thetaVar from the PCA outputs
//                     and the two STFT planes, one thread per point
//   k_argmax1/2       get_max_confidence_point: masked argmax, lowest flat
//                     index on ties (two stages)
//   k_theta_pass      one block per bin row, frames along the fast axis: the
//                     candidate mask and compute_temporal's three per-bin
//                     sums (per-thread strided partial sums, then a fixed
//                     shared-memory tree)
//   k_delta_pass      getTFPointsNearDelta: writes cluster mask n, clears its
//                     points from the set still to classify, counts both
//   k_exclusive       create_exclusive_clusters over the stack of masks
//   k_csums1/2        per-cluster thresholded sums (two stages, fixed order)
//
// k_theta_pass reads theta, phi, var (24 B) and the subset byte per point and
// writes one byte; it runs at 0.75 of the measured HBM copy rate.
// k_delta_pass reads the four planes (32 B) and the subset byte and writes two
// bytes, but its FP64 sincos / cos / sin / sqrt per point bound it, at 0.07 of
// that rate (profiles/demix_bench.jsonl).  The expressions
// follow NumPy's operation order with contraction off.
#include "fasst_device.h"
#include "../../include/fasst_demix.h"
#include "../../include/fasst_sigtools.h"

#include <atomic>
#include <climits>
#include <cmath>
#include <vector>

namespace fasst {

static std::atomic<long> g_dmx_launches{0};
static std::atomic<long> g_dmx_transfers{0};
static float g_dmx_ms = 0.f;

constexpr int kDB = 256;           // threads per block, every kernel here
constexpr int kDmxMaxBlocks = 1024;  // stage-1 blocks of the two-stage reductions
constexpr double kUBound = 2.33;   // uVarBound == uDistBound (demixTF.py:50-51)

// estim_var_theta (:497-512) of one confidence
__device__ __forceinline__ double dmx_var_theta(double conf, double nm1) {
#pragma clang fp contract(off)
  double v = 1.0;
  if (conf > kEps) {
    const double p = pow(10.0, conf / 20.0);
    const double q = p - 1.0;
    v = p / (nm1 * (q * q));
  }
  if (conf >= 3073.0) v = 0.0;
  if (conf <= kEps) v = INFINITY;
  return v;
}

// fixed-order tree over the block's kDB values (the sums do not go through
// block_sum of fasst_device.h: its blockDim.x loop compiles differently from
// this constant-bound one, and the other operators need the template anyway)
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T *sm, Op op) {
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = kDB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = op(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  const T r = sm[0];
  __syncthreads();
  return r;
}

struct CMax {
  double re, im;
};
__device__ __forceinline__ CMax cmax_op(CMax a, CMax b) {
  // NumPy's complex order: real parts first, then imaginary parts
  return (a.re > b.re || (a.re == b.re && a.im >= b.im)) ? a : b;
}

// mean(array([X0, X1]) ** 2, axis=0) at one point: NumPy's complex square and
// an exact halving
__device__ __forceinline__ CMax dmx_energy(double2 a, double2 b) {
#pragma clang fp contract(off)
  const double ar = a.x * a.x - a.y * a.y, ai = a.x * a.y + a.y * a.x;
  const double br = b.x * b.x - b.y * b.y, bi = b.x * b.y + b.y * b.x;
  CMax e;
  e.re = (ar + br) * 0.5;
  e.im = (ai + bi) * 0.5;
  return e;
}

struct FeatArgs {
  const double2 *x0, *x1;  // [F][N]
  const double *lM, *lm;   // [F][L]
  const double2 *vM;       // [2][F][L]
  double *conf, *theta, *phi, *var;
  CMax *part;  // [kDmxMaxBlocks] + the result at [kDmxMaxBlocks]
  int F, N, L, nb, nblocks;
};

__global__ __launch_bounds__(kDB) void k_energy_max1(const FeatArgs a) {
  __shared__ CMax sm[kDB];
  const size_t n = (size_t)a.F * a.L;
  const int start = a.nb / 2;
  CMax m;
  m.re = -INFINITY;
  m.im = -INFINITY;
  for (size_t i = (size_t)blockIdx.x * kDB + threadIdx.x; i < n; i += (size_t)gridDim.x * kDB) {
    const size_t f = i / a.L, l = i - f * a.L;
    const size_t o = f * a.N + start + l;
    m = cmax_op(m, dmx_energy(a.x0[o], a.x1[o]));
  }
  m = block_reduce(m, sm, cmax_op);
  if (threadIdx.x == 0) a.part[blockIdx.x] = m;
}

__global__ __launch_bounds__(kDB) void k_energy_max2(const FeatArgs a) {
  __shared__ CMax sm[kDB];
  CMax m;
  m.re = -INFINITY;
  m.im = -INFINITY;
  for (int i = threadIdx.x; i < a.nblocks; i += kDB) m = cmax_op(m, a.part[i]);
  m = block_reduce(m, sm, cmax_op);
  if (threadIdx.x == 0) a.part[kDmxMaxBlocks] = m;
}

__global__ __launch_bounds__(kDB) void k_features(const FeatArgs a) {
#pragma clang fp contract(off)
  const size_t n = (size_t)a.F * a.L;
  const size_t i = (size_t)blockIdx.x * kDB + threadIdx.x;
  if (i >= n) return;
  const size_t f = i / a.L, l = i - f * a.L;
  // confidence (:459-469, :481)
  double conf = 20.0 * log10(a.lM[i] / fmax(a.lm[i], kEps));
  if (conf != conf) conf = 0.0;
  const CMax mx = a.part[kDmxMaxBlocks];
  const double tr = mx.re * 1e-6, ti = mx.im * 1e-6;
  const size_t o = f * a.N + a.nb / 2 + l;
  const CMax e = dmx_energy(a.x0[o], a.x1[o]);
  if (e.re < tr || (e.re == tr && e.im < ti)) conf = 0.0;
  if (f < 2) conf = kEps;
  // phi = angle(e1 / e0), theta = arctan(|e1| / |e0|) (:492-493)
  const double2 e0 = a.vM[i], e1 = a.vM[n + i];
  double qr, qi;
  if (e0.x == 0.0 && e0.y == 0.0) {  // NumPy's complex division by zero
    qr = e1.x / fabs(e0.x);
    qi = e1.y / fabs(e0.y);
  } else if (fabs(e0.x) >= fabs(e0.y)) {
    const double rat = e0.y / e0.x;
    const double scl = 1.0 / (e0.x + e0.y * rat);
    qr = (e1.x + e1.y * rat) * scl;
    qi = (e1.y - e1.x * rat) * scl;
  } else {
    const double rat = e0.x / e0.y;
    const double scl = 1.0 / (e0.y + e0.x * rat);
    qr = (e1.x * rat + e1.y) * scl;
    qi = (e1.y * rat - e1.x) * scl;
  }
  a.phi[i] = atan2(qi, qr);
  a.theta[i] = atan(np_cabs(e1.x, e1.y) / np_cabs(e0.x, e0.y));
  a.conf[i] = conf;
  a.var[i] = dmx_var_theta(conf, (double)a.nb - 1.0);
}

// ------------------------------------------------------------------ argmax
struct AMax {
  double v;
  long long i;
};
__device__ __forceinline__ AMax amax_op(AMax a, AMax b) {
  return (a.v > b.v || (a.v == b.v && a.i < b.i)) ? a : b;
}

struct RoundArgs {
  const double *conf, *theta, *phi, *var;
  unsigned char *rem, *cand, *mask;  // [F][L] each; mask: this round's slot
  AMax *apart;                       // [kDmxMaxBlocks]
  double *aout;                      // [4]
  double *sums;                      // [F][3]
  const double2 *v1;                 // [F]
  unsigned long long *cnt;           // [2]
  size_t n;
  int F, L, nblocks, only_centroid;
  long long centroid;
  double theta_c, bound, v0, conf_c, sq_err;
};

__global__ __launch_bounds__(kDB) void k_argmax1(const RoundArgs a) {
  __shared__ AMax sm[kDB];
  AMax m;
  m.v = -INFINITY;
  m.i = LLONG_MAX;
  for (size_t i = (size_t)blockIdx.x * kDB + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kDB) {
    AMax c;
    c.v = a.rem[i] ? a.conf[i] : 0.0;
    c.i = (long long)i;
    // np.argmax: a NaN is the maximum (the confidence holds none)
    m = amax_op(m, c);
  }
  m = block_reduce(m, sm, amax_op);
  if (threadIdx.x == 0) a.apart[blockIdx.x] = m;
}

__global__ __launch_bounds__(kDB) void k_argmax2(const RoundArgs a) {
  __shared__ AMax sm[kDB];
  AMax m;
  m.v = -INFINITY;
  m.i = LLONG_MAX;
  for (int i = threadIdx.x; i < a.nblocks; i += kDB) m = amax_op(m, a.apart[i]);
  m = block_reduce(m, sm, amax_op);
  if (threadIdx.x == 0) {
    const size_t i = (m.i >= 0 && (size_t)m.i < a.n) ? (size_t)m.i : 0;
    a.aout[0] = (double)i;
    a.aout[1] = a.conf[i];
    a.aout[2] = a.theta[i];
    a.aout[3] = a.phi[i];
  }
}

// -------------------------------------------------- theta mask + bin sums
__device__ __forceinline__ double add_op(double x, double y) { return x + y; }

__global__ __launch_bounds__(kDB) void k_theta_pass(const RoundArgs a) {
#pragma clang fp contract(off)
  __shared__ double sm[kDB];
  const int f = blockIdx.x;
  const size_t row = (size_t)f * a.L;
  double sr = 0.0, si = 0.0, sn = 0.0;
  for (int t = threadIdx.x; t < a.L; t += kDB) {
    const size_t i = row + t;
    const bool in = (fabs(a.theta[i] - a.theta_c) < a.bound) && a.rem[i];
    a.cand[i] = in ? 1 : 0;
    if (in) {
      double v = a.var[i];
      if (v == 0.0) v = kEps;
      const double w = 1.0 / v;
      double s, c;
      sincos(a.phi[i], &s, &c);
      sr += w * c;
      si += w * s;
      sn += w;
    }
  }
  sr = block_reduce(sr, sm, add_op);
  si = block_reduce(si, sm, add_op);
  sn = block_reduce(sn, sm, add_op);
  if (threadIdx.x == 0) {
    a.sums[3 * f] = sr;
    a.sums[3 * f + 1] = si;
    a.sums[3 * f + 2] = sn;
  }
}

// -------------------------------------------------------------- delta mask
__global__ __launch_bounds__(kDB) void k_delta_pass(const RoundArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long sm[kDB];
  unsigned long long size = 0, left = 0;
  const size_t i = (size_t)blockIdx.x * kDB + threadIdx.x;
  if (i < a.n) {
    bool in;
    if (a.only_centroid) {
      in = false;
    } else {
      const size_t f = i / a.L;
      const double th = a.theta[i], ph = a.phi[i];
      double s, c;
      sincos(ph, &s, &c);
      const double u0 = cos(th), st = sin(th);
      const double u1r = st * c, u1i = st * s;
      const double2 v1 = a.v1[f];
      // u0 * v0 + u1 * v1
      const double zr = u0 * a.v0 + (u1r * v1.x - u1i * v1.y);
      const double zi = u1r * v1.y + u1i * v1.x;
      const double dist = sqrt(2.0 * (1.0 - np_cabs(zr, zi)));
      double bound = (sqrt(a.var[i]) + a.sq_err) * kUBound;
      if (a.conf_c < a.conf[i]) bound = 0.0;
      in = dist < bound;
    }
    if ((long long)i == a.centroid) in = true;
    a.mask[i] = in ? 1 : 0;
    unsigned char r = a.rem[i];
    if (in && r) {
      r = 0;
      a.rem[i] = 0;
    }
    size = in ? 1 : 0;
    left = r ? 1 : 0;
  }
  auto uadd = [](unsigned long long x, unsigned long long y) { return x + y; };
  size = block_reduce(size, sm, uadd);
  left = block_reduce(left, sm, uadd);
  if (threadIdx.x == 0) {
    if (size) atomicAdd(a.cnt, size);
    if (left) atomicAdd(a.cnt + 1, left);
  }
}

// -------------------------------------------------------------- refinement
struct RefArgs {
  unsigned char *masks;  // [max_clusters][n]
  const int *slots;      // [nc]
  const double *thr;     // [nc]
  const double *conf, *theta, *var;
  unsigned long long *sizes;  // [nc]
  double *part;               // [nc][nblocks][4]
  double *out;                // [nc][4]
  size_t n;
  int nc, nblocks;
  double nm1, shift;  // neighbors - 1, uVarBound * sigma
};

__global__ __launch_bounds__(kDB) void k_exclusive(const RefArgs a) {
  const size_t i = (size_t)blockIdx.x * kDB + threadIdx.x;
  const bool live = i < a.n;
  int count = 0;
  for (int k = 0; k < a.nc; ++k) {
    bool m = false;
    if (live) {
      unsigned char *p = a.masks + (size_t)a.slots[k] * a.n + i;
      m = *p != 0;
      count += m ? 1 : 0;
      if (k > 0 && m && count != 1) {
        m = false;
        *p = 0;
      }
    }
    const unsigned long long b = __ballot(m);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.sizes + k, (unsigned long long)__popcll(b));
  }
}

__global__ __launch_bounds__(kDB) void k_csums1(const RefArgs a) {
#pragma clang fp contract(off)
  __shared__ double sm[kDB];
  const int k = blockIdx.y;
  const unsigned char *m = a.masks + (size_t)a.slots[k] * a.n;
  const double thr = a.thr[k];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (size_t i = (size_t)blockIdx.x * kDB + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kDB) {
    if (!m[i]) continue;
    const double conf = a.conf[i];
    if (!(conf >= thr)) continue;
    const double var = a.var[i];
    s0 += 1.0 / var;
    s1 += a.theta[i] / var;
    // estim_bound_var_theta(confidence, 'sup', uVarBound) (:514-529)
    const double cb = fmax(conf + -1.0 * a.shift, 0.0);
    s2 += 1.0 / dmx_var_theta(cb, a.nm1);
    s3 += 1.0;
  }
  double *o = a.part + ((size_t)k * a.nblocks + blockIdx.x) * 4;
  s0 = block_reduce(s0, sm, add_op);
  s1 = block_reduce(s1, sm, add_op);
  s2 = block_reduce(s2, sm, add_op);
  s3 = block_reduce(s3, sm, add_op);
  if (threadIdx.x == 0) {
    o[0] = s0;
    o[1] = s1;
    o[2] = s2;
    o[3] = s3;
  }
}

__global__ __launch_bounds__(kDB) void k_csums2(const RefArgs a) {
  __shared__ double sm[kDB];
  const int k = blockIdx.x;
  const double *p = a.part + (size_t)k * a.nblocks * 4;
  for (int j = 0; j < 4; ++j) {
    double s = 0.0;
    for (int i = threadIdx.x; i < a.nblocks; i += kDB) s += p[(size_t)i * 4 + j];
    s = block_reduce(s, sm, add_op);
    if (threadIdx.x == 0) a.out[(size_t)k * 4 + j] = s;
  }
}

// ----------------------------------------------------------------- host side
// HIP events around the kernels of one call (demix_last_ms); the two events
// belong to the context
static int dmx_start(const Events &tm) {
  FASST_HIP(hipEventRecord(tm.e[0], 0));
  return FASST_OK;
}
static int dmx_finish(const Events &tm, int n_kernels) {
  FASST_LAUNCH_CHECK();
  g_dmx_launches += n_kernels;
  return elapsed_ms(tm.e[0], tm.e[1], 0, &g_dmx_ms);
}

static int stage1_blocks(size_t n) {
  const size_t b = (n + kDB - 1) / kDB;
  return (int)(b < (size_t)kDmxMaxBlocks ? b : (size_t)kDmxMaxBlocks);
}

}  // namespace fasst

using namespace fasst;

struct demix_ctx {
  int device = 0, F = 0, N = 0, nb = 0, L = 0, maxc = 0;
  size_t n = 0;
  bool have_features = false;
  Events tm;
  DBuf<double> planes;  // [4][n]
  DBuf<unsigned char> rem, cand, masks;
  DBuf<AMax> apart;
  DBuf<double> aout, sums;
  DBuf<double2> v1;
  DBuf<unsigned long long> cnt;
  double *plane(int w) { return planes.p + (size_t)w * n; }
};

static bool ctx_ok(demix_ctx *c, const char *fn, bool need_features = true) {
  if (!c) {
    set_error("%s: null context", fn);
    return false;
  }
  if (need_features && !c->have_features) {
    set_error("%s: no feature planes yet (demix_features or demix_set_plane first)", fn);
    return false;
  }
  return true;
}

static void round_args(demix_ctx *c, RoundArgs &a) {
  a.conf = c->plane(0);
  a.theta = c->plane(1);
  a.phi = c->plane(2);
  a.var = c->plane(3);
  a.rem = c->rem.p;
  a.cand = c->cand.p;
  a.mask = nullptr;
  a.apart = c->apart.p;
  a.aout = c->aout.p;
  a.sums = c->sums.p;
  a.v1 = c->v1.p;
  a.cnt = c->cnt.p;
  a.n = c->n;
  a.F = c->F;
  a.L = c->L;
  a.nblocks = stage1_blocks(c->n);
  a.only_centroid = 0;
  a.centroid = -1;
  a.theta_c = a.bound = a.v0 = a.conf_c = a.sq_err = 0.0;
}

extern "C" {

int demix_last_ms(double *device_ms) {
  if (device_ms) *device_ms = g_dmx_ms;
  return FASST_OK;
}

int demix_launch_count(long *count) {
  if (count) *count = g_dmx_launches.load();
  return FASST_OK;
}

int demix_transfer_count(long *count) {
  if (count) *count = g_dmx_transfers.load();
  return FASST_OK;
}

int demix_create(int device, int F, int N, int neighbors, int max_clusters, demix_ctx **out) {
  if (!out) {
    set_error("demix_create: null argument");
    return FASST_ERR_SHAPE;
  }
  *out = nullptr;
  if (F < 1 || N < 1 || neighbors < 1 || neighbors > N || max_clusters < 1) {
    set_error("demix_create: bad shape (F %d, N %d, neighbors %d: 1 <= neighbors <= N, "
              "max_clusters %d)", F, N, neighbors, max_clusters);
    return FASST_ERR_SHAPE;
  }
  const size_t n = (size_t)F * (N - neighbors + 1);
  if ((n + kDB - 1) / kDB > (size_t)INT_MAX) {
    set_error("demix_create: %d bins x %d frames exceed the grid", F, N);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(device);
  demix_ctx *c = new demix_ctx;
  c->device = device;
  c->F = F;
  c->N = N;
  c->nb = neighbors;
  c->L = N - neighbors + 1;
  c->maxc = max_clusters;
  c->n = n;
  int st;
  if ((st = c->planes.alloc(4 * n)) || (st = c->rem.alloc(n)) || (st = c->cand.alloc(n)) ||
      (st = c->masks.alloc((size_t)max_clusters * n)) || (st = c->apart.alloc(kDmxMaxBlocks)) ||
      (st = c->aout.alloc(4)) || (st = c->sums.alloc((size_t)3 * F)) || (st = c->v1.alloc(F)) ||
      (st = c->cnt.alloc(2)) || (st = c->tm.create(2))) {
    delete c;
    return st;
  }
  *out = c;
  return FASST_OK;
}

int demix_destroy(demix_ctx *c) {
  if (!c) return FASST_OK;
  DeviceGuard g(c->device);
  delete c;
  return FASST_OK;
}

int demix_features_dev(demix_ctx *c, const double *x0, const double *x1) {
  if (!ctx_ok(c, "demix_features", false)) return FASST_ERR_SHAPE;
  if (!x0 || !x1) {
    set_error("demix_features: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  const size_t n = c->n;
  DBuf<double> lM, lm, vM, vm;
  DBuf<CMax> part;
  if ((st = lM.alloc_uninit(n)) || (st = lm.alloc_uninit(n)) || (st = vM.alloc_uninit(4 * n)) ||
      (st = vm.alloc_uninit(4 * n)) || (st = part.alloc(kDmxMaxBlocks + 1)))
    return st;
  int flags[2] = {0, 0};
  if ((st = sig_pca2d_dev(c->device, c->F, c->N, c->nb, x0, x1, lM.p, lm.p, vM.p, vm.p, flags)))
    return st;
  double pca_ms = 0.0;
  sig_last_ms(&pca_ms);
  FeatArgs a;
  a.x0 = (const double2 *)x0;
  a.x1 = (const double2 *)x1;
  a.lM = lM.p;
  a.lm = lm.p;
  a.vM = (const double2 *)vM.p;
  a.conf = c->plane(0);
  a.theta = c->plane(1);
  a.phi = c->plane(2);
  a.var = c->plane(3);
  a.part = part.p;
  a.F = c->F;
  a.N = c->N;
  a.L = c->L;
  a.nb = c->nb;
  a.nblocks = stage1_blocks(n);
  if ((st = dmx_start(c->tm))) return st;
  k_energy_max1<<<a.nblocks, kDB>>>(a);
  k_energy_max2<<<1, kDB>>>(a);
  k_features<<<(unsigned)((n + kDB - 1) / kDB), kDB>>>(a);
  if ((st = dmx_finish(c->tm, 3))) return st;
  g_dmx_ms += (float)pca_ms;
  c->have_features = true;
  return FASST_OK;
}

int demix_features(demix_ctx *c, const double *x0, const double *x1) {
  if (!ctx_ok(c, "demix_features", false)) return FASST_ERR_SHAPE;
  if (!x0 || !x1) {
    set_error("demix_features: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  const size_t nin = (size_t)2 * c->F * c->N;
  DBuf<double> d0, d1;
  if ((st = d0.upload(x0, nin)) || (st = d1.upload(x1, nin))) return st;
  return demix_features_dev(c, d0.p, d1.p);
}

int demix_get_plane(demix_ctx *c, int which, double *out) {
  if (!ctx_ok(c, "demix_get_plane")) return FASST_ERR_SHAPE;
  if (which < 0 || which > 3 || !out) {
    set_error("demix_get_plane: plane %d outside 0 .. 3, or a null pointer", which);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  FASST_TRY(c->planes.at(which * c->n, c->n).get(out, c->n));
  ++g_dmx_transfers;
  return FASST_OK;
}

int demix_set_plane(demix_ctx *c, int which, const double *in) {
  if (!ctx_ok(c, "demix_set_plane", false)) return FASST_ERR_SHAPE;
  if (which < 0 || which > 3 || !in) {
    set_error("demix_set_plane: plane %d outside 0 .. 3, or a null pointer", which);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  FASST_TRY(c->planes.at(which * c->n, c->n).put(in, c->n));
  c->have_features = true;
  return FASST_OK;
}

// the n bytes of mask `slot`; p == nullptr (and the error set) for a bad slot
static DSpan<unsigned char> mask_span(demix_ctx *c, int slot, const char *fn) {
  if (slot == DEMIX_MASK_SUBSET) return c->rem.at(0, c->n);
  if (slot == DEMIX_MASK_CANDIDATES) return c->cand.at(0, c->n);
  if (slot < 0 || slot >= c->maxc) {
    set_error("%s: mask %d outside 0 .. %d", fn, slot, c->maxc - 1);
    return {};
  }
  return c->masks.at((size_t)slot * c->n, c->n);
}

int demix_get_mask(demix_ctx *c, int slot, unsigned char *out) {
  if (!ctx_ok(c, "demix_get_mask", false)) return FASST_ERR_SHAPE;
  const DSpan<unsigned char> m = mask_span(c, slot, "demix_get_mask");
  if (!m.p || !out) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  FASST_TRY(m.get(out, c->n));
  ++g_dmx_transfers;
  return FASST_OK;
}

int demix_set_mask(demix_ctx *c, int slot, const unsigned char *in) {
  if (!ctx_ok(c, "demix_set_mask", false)) return FASST_ERR_SHAPE;
  const DSpan<unsigned char> m = mask_span(c, slot, "demix_set_mask");
  if (!m.p || !in) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  return m.put(in, c->n);
}

int demix_init_subset(demix_ctx *c) {
  if (!ctx_ok(c, "demix_init_subset", false)) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  FASST_HIP(hipMemset(c->rem.p, 1, c->n));   // (a fill with 1, not 0: no DSpan::zero)
  FASST_HIP(hipDeviceSynchronize());
  return FASST_OK;
}

int demix_argmax(demix_ctx *c, double *out) {
  if (!ctx_ok(c, "demix_argmax")) return FASST_ERR_SHAPE;
  if (!out) {
    set_error("demix_argmax: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  RoundArgs a;
  round_args(c, a);
  if ((st = dmx_start(c->tm))) return st;
  k_argmax1<<<a.nblocks, kDB>>>(a);
  k_argmax2<<<1, kDB>>>(a);
  if ((st = dmx_finish(c->tm, 2))) return st;
  return c->aout.get(out, 4);
}

int demix_theta_pass(demix_ctx *c, double theta_c, double dist_bound, double *sums) {
  if (!ctx_ok(c, "demix_theta_pass")) return FASST_ERR_SHAPE;
  if (!sums) {
    set_error("demix_theta_pass: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  RoundArgs a;
  round_args(c, a);
  a.theta_c = theta_c;
  a.bound = dist_bound;
  if ((st = dmx_start(c->tm))) return st;
  k_theta_pass<<<c->F, kDB>>>(a);
  if ((st = dmx_finish(c->tm, 1))) return st;
  return c->sums.get(sums, (size_t)3 * c->F);
}

int demix_delta_pass(demix_ctx *c, int slot, double theta_c, const double *v1, double conf_c,
                     double max_err, long centroid, int only_centroid, long *counts) {
  if (!ctx_ok(c, "demix_delta_pass")) return FASST_ERR_SHAPE;
  if (slot < 0 || slot >= c->maxc || !counts || (!only_centroid && !v1) || centroid < 0 ||
      (size_t)centroid >= c->n) {
    set_error("demix_delta_pass: mask %d outside 0 .. %d, centroid %ld outside the plane, or a "
              "null pointer", slot, c->maxc - 1, centroid);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  RoundArgs a;
  round_args(c, a);
  a.mask = c->masks.p + (size_t)slot * c->n;
  a.theta_c = theta_c;
  a.v0 = std::cos(theta_c);
  a.conf_c = conf_c;
  a.sq_err = std::sqrt(max_err);
  a.centroid = centroid;
  a.only_centroid = only_centroid;
  if (!only_centroid && (st = c->v1.put(v1, c->F))) return st;
  FASST_TRY(c->cnt.zero(2));
  if ((st = dmx_start(c->tm))) return st;
  k_delta_pass<<<(unsigned)((c->n + kDB - 1) / kDB), kDB>>>(a);
  if ((st = dmx_finish(c->tm, 1))) return st;
  unsigned long long h[2];
  if ((st = c->cnt.get(h, 2))) return st;
  counts[0] = (long)h[0];
  counts[1] = (long)h[1];
  return FASST_OK;
}

static int ref_args(demix_ctx *c, int n, const int *slots, const char *fn, RefArgs &a,
                    DBuf<int> &dslots) {
  if (n < 1 || n > c->maxc || !slots) {
    set_error("%s: %d clusters outside 1 .. %d, or a null pointer", fn, n, c->maxc);
    return FASST_ERR_SHAPE;
  }
  for (int k = 0; k < n; ++k)
    if (slots[k] < 0 || slots[k] >= c->maxc) {
      set_error("%s: mask %d outside 0 .. %d", fn, slots[k], c->maxc - 1);
      return FASST_ERR_SHAPE;
    }
  FASST_TRY(dslots.upload(slots, n));
  a.masks = c->masks.p;
  a.slots = dslots.p;
  a.thr = nullptr;
  a.conf = c->plane(0);
  a.theta = c->plane(1);
  a.var = c->plane(3);
  a.sizes = nullptr;
  a.part = a.out = nullptr;
  a.n = c->n;
  a.nc = n;
  a.nblocks = stage1_blocks(c->n);
  a.nm1 = (double)c->nb - 1.0;
  a.shift = kUBound * std::sqrt(1600.0 / ((double)c->nb - 1.0));
  return FASST_OK;
}

int demix_exclusive(demix_ctx *c, int n, const int *slots, long *sizes) {
  if (!ctx_ok(c, "demix_exclusive", false)) return FASST_ERR_SHAPE;
  if (!sizes) {
    set_error("demix_exclusive: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  RefArgs a;
  DBuf<int> dslots;
  DBuf<unsigned long long> dsizes;
  if ((st = ref_args(c, n, slots, "demix_exclusive", a, dslots)) || (st = dsizes.alloc(n)))
    return st;
  a.sizes = dsizes.p;
  if ((st = dmx_start(c->tm))) return st;
  k_exclusive<<<(unsigned)((c->n + kDB - 1) / kDB), kDB>>>(a);
  if ((st = dmx_finish(c->tm, 1))) return st;
  std::vector<unsigned long long> h(n);
  if ((st = dsizes.get(h.data(), n))) return st;
  for (int k = 0; k < n; ++k) sizes[k] = (long)h[k];
  return FASST_OK;
}

int demix_cluster_sums(demix_ctx *c, int n, const int *slots, const double *thresholds,
                       double *sums) {
  if (!ctx_ok(c, "demix_cluster_sums")) return FASST_ERR_SHAPE;
  if (!thresholds || !sums) {
    set_error("demix_cluster_sums: null argument");
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  int st;
  RefArgs a;
  DBuf<int> dslots;
  DBuf<double> dthr, part, out;
  if ((st = ref_args(c, n, slots, "demix_cluster_sums", a, dslots))) return st;
  if ((st = dthr.upload(thresholds, n)) || (st = part.alloc_uninit((size_t)n * a.nblocks * 4)) ||
      (st = out.alloc_uninit((size_t)n * 4)))
    return st;
  a.thr = dthr.p;
  a.part = part.p;
  a.out = out.p;
  if ((st = dmx_start(c->tm))) return st;
  k_csums1<<<dim3(a.nblocks, n), kDB>>>(a);
  k_csums2<<<n, kDB>>>(a);
  if ((st = dmx_finish(c->tm, 2))) return st;
  return out.get(sums, out.n);
}

}  // extern "C"
