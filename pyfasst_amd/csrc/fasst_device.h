// Device helpers shared by every kernel file of the engine (gfx950).  A helper
// with a numerical contract (np.abs bit for bit, a reciprocal within 1 ulp, a
// fixed summation order) lives here once, so a fix reaches every caller.
#pragma once
#include "fasst_common.h"
#include "fasst_esched.h"

namespace fasst {

// Device-side halt: once an iteration raises a flag (singular mixing solve,
// dead TW) every later kernel of the batch returns at entry, so a batch of
// iterations is enqueued without host round trips and the state stays the
// one the flagged iteration left (flags layout in fasst_ctx.h).
#define HALT_GUARD(h)                                   \
  do {                                                  \
    if ((h) && *(volatile const int *)(h)) return;      \
  } while (0)

// v_mfma_f64_16x16x4f64: D (16 x 16) = A (16 x 4) B (4 x 16) + C
__device__ __forceinline__ d4 mfma4(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// v_mfma_f64_4x4x4f64: four independent 4 x 4 blocks
__device__ __forceinline__ double mfma44(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// 1/x for finite normal x (the E-step's guarded det and max(V, eps), the
// NMF / SIMM ratios' max(hat, eps)): v_rcp_f64 + two Newton steps (<= 1 ulp)
// instead of the ~10-instruction IEEE division sequence.
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}

// np.abs(complex128): larger * sqrt(fma(r, r, 1)), r = smaller / larger
// (NumPy's SIMD loop for complex absolute)
__device__ __forceinline__ double np_cabs(double re, double im) {
#pragma clang fp contract(off)
  const double a = fabs(re), b = fabs(im);
  if (isinf(a) || isinf(b)) return INFINITY;
  if (a != a || b != b) return NAN;
  const double l = a > b ? a : b, s = a > b ? b : a;
  const double r = l == 0.0 ? 0.0 : s / l;
  return sqrt(fma(r, r, 1.0)) * l;
}

// x ** omega as NumPy gives it (omega == 1: the identity, exact)
__device__ __forceinline__ double pow_omega(double x, double omega) {
  return omega == 1.0 ? x : pow(x, omega);
}

// sum over the wave's 64 lanes in a fixed butterfly: every lane ends with the
// same value, whatever the grid
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// sum over the block in a fixed tree through s[blockDim.x] (blockDim.x a power
// of two); every thread returns the total and s is free again on return
__device__ __forceinline__ double block_sum(double x, double *s) {
  s[threadIdx.x] = x;
  __syncthreads();
  for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
    if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// medianFilter's output sample n of a row of N samples (tools/signalTools.py
// :13-24): the median of the window [max(n - length, 0), min(n + length, N - 1)),
// an even count averaging the two middle values; an empty window, one that
// holds a NaN, or a NaN mean (+inf and -inf in the middle) gives `self`, the
// sample itself.  Selection by rank counting, ties broken by index, so any
// window length works.  src is indexed by the sample's own index (the row, or
// an LDS stage of it offset by the stage's first sample); length <= N.
// A span of more than kMedLdsSpan doubles (48 KiB) is not staged by the callers
constexpr int kMedLdsSpan = 6144;
__device__ __forceinline__ double median_at(const double *src, double self, int n, int length, int N) {
#pragma clang fp contract(off)
  const int lo = max(n - length, 0);
  const int hi = (int)min((long)n + length, (long)N - 1);
  const int cnt = hi - lo;
  if (cnt <= 0) return self;
  bool has_nan = false;
  for (int i = lo; i < hi; ++i) has_nan |= src[i] != src[i];
  if (has_nan) return self;
  const int k1 = (cnt - 1) >> 1, k2 = cnt >> 1;
  double v1 = 0.0, v2 = 0.0;
  int found = 0;
  for (int i = lo; i < hi && found < 2; ++i) {
    const double xi = src[i];
    int rank = 0;
    for (int j = lo; j < hi; ++j) {
      const double xj = src[j];
      rank += (xj < xi) || (xj == xi && j < i);
    }
    if (rank == k1) { v1 = xi; ++found; }
    if (rank == k2) { v2 = xi; ++found; }
  }
  const double res = k1 == k2 ? v1 : (v1 + v2) / 2.0;
  return res != res ? self : res;
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) {
  return make_double2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ double2 csub(double2 a, double2 b) {
  return make_double2(a.x - b.x, a.y - b.y);
}
__device__ __forceinline__ double2 cscale(double2 a, double s) {
  return make_double2(a.x * s, a.y * s);
}

// raw-buffer access to streamed operands: a wave-uniform resource (SGPRs,
// formed on the scalar unit) + a 32-bit per-lane byte offset vo + a uniform
// byte offset so, so no 64-bit VALU address arithmetic per access and every
// load is issued unconditionally (AUX 2 = non-temporal).  The resource spans
// 2 GB from p: the callers keep their offsets inside their allocations.
typedef unsigned buf_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const double *p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(p), 0, 0x7fffffff, 0x00020000);
}
template <int AUX>
__device__ __forceinline__ double buf_ld(__amdgpu_buffer_rsrc_t r, unsigned vo, unsigned so) {
  const buf_u2 x = __builtin_amdgcn_raw_buffer_load_b64(r, (int)vo, (int)so, AUX);
  return __builtin_bit_cast(double, x);
}

// XCD-aware logical block: workgroups b, b + 8, ... of a launch share an XCD
// (dispatch is round-robin over the 8 XCDs, for speed only, never
// correctness); the bijective remap of cdna_hip_programming.md gives each XCD
// a contiguous run of the logical (x fastest, z slowest) sequence, so the
// blocks that re-read one operand slice (the E-step's TW chunk, the
// contractions' W / (FW H)^T slices) meet in one 4 MB L2.  At C3 it takes
// 9-14 % off the HBM fetch of the E-step and both contractions (rocprofv3
// FETCH_SIZE, profiles/r4_bench.txt vs the row-major order) at equal time.
__device__ __forceinline__ dim3 xcd_block() {
  const int nx = gridDim.x, ny = gridDim.y, n = nx * ny * gridDim.z;
  const int b = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
  const int q = n / 8, r = n % 8, x = b % 8;
  const int L = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
  return dim3(L % nx, (L / nx) % ny, L / (nx * ny));
}

// max(x, y) as ONE v_max_f64: fmax() lowers to llvm.maxnum, whose operands
// the backend first canonicalises (a second v_max_f64 each) unless it can
// prove them canonical, which it cannot for MFMA results.  For the finite
// operands it is used on the two forms agree.
__device__ __forceinline__ double vmax_f64(double x, double y) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}

// One element of the TW image [ntt][J][KP / 8][64]: piece (tt, j, u), lane l
// pairs the operands of the k-steps 2 u and 2 u + 1, TW[j][tq + 8 u][16 tt +
// fl] and TW[j][tq + 8 u + 4][16 tt + fl]; `row(k)` is row k of source j at
// frame 16 tt + fl
template <class Row>
__device__ __forceinline__ void tw_image_store(double2 *__restrict__ img, int tt, int j, int J,
                                               int KP, int e, Row &&row) {
  const int u = e >> 6, lane = e & 63, fl = lane & 15, tq = lane >> 4;
  img[((size_t)tt * J + j) * (KP / 8) * 64 + e] = make_double2(row(tq + 8 * u, fl), row(tq + 8 * u + 4, fl));
}

// sum of the E-step's loglik partials [slot][bin tile]: the live entries
// (slot < segments of the bin tile, fasst_esched.h) in index order, strided
// over the 256 threads (a fixed order)
__device__ __forceinline__ double ll_partial_sum(const double *__restrict__ llpart, const ESched es) {
  double x = 0.0;
  for (int i = threadIdx.x; i < es.nslot * es.nbt; i += 256) {
    const int sl = i / es.nbt, bt = i - sl * es.nbt;
    if (sl < es_segments(es, bt)) x += llpart[i];
  }
  return x;
}

// The slot buffer tb[j][b] of a spectral component with time blobs (H = TW TB,
// fasst_em_spectral.hip): its factor TW ("TWs", kbw block rows x L), TB
// (L x Tp) and the TW step's numerator / denominator
struct TBLayout {
  size_t tws, tb, num, den, n;   // offsets (doubles) in the slot buffer, total
};
__host__ __device__ inline TBLayout tb_layout(int kbw, int L, int Tp) {
  TBLayout o;
  o.tws = 0;
  o.tb = (size_t)kbw * L;
  o.num = o.tb + (size_t)L * Tp;
  o.den = o.num + (size_t)kbw * L;
  o.n = o.den + (size_t)kbw * L;
  return o;
}

// the time-blob kernels' halt test (iter: TBArgs::iter / TBRArgs::iter)
__device__ inline bool tb_halted(const int *halt, const int *flags, int iter) {
  if (!halt || !*(volatile const int *)halt) return false;
  return iter < 0 || *(volatile const int *)(flags + kFlagIter) < iter;
}

}  // namespace fasst
