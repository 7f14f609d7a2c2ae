// Shared definitions of the MI355X FASST engine (gfx950, HIP).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdarg>
#include <string>
#include <vector>

#include "../../include/fasst_hip.h"

namespace fasst {

// Kernel attribute: keep adjacent LDS reads / writes as separate ds_read_b64 /
// ds_write_b64 instead of ds_read2_b64 / ds_read2st64_b64 pairs, which take
// 8 LDS cycles for the 2 + 2 of two single reads (MI355X_MICROARCH.md §LDS).
// A device-code target feature: the host pass of the same source does not
// know it, so it is spelled only for the device pass.
#if defined(__HIP_DEVICE_COMPILE__)
#define FASST_NO_LDS_PAIRING __attribute__((target("no-load-store-opt")))
#else
#define FASST_NO_LDS_PAIRING
#endif

constexpr double kEps = 1e-10;  // audioModel.py:61, tools/signalTools.py:11
constexpr int kMaxJ = 16;       // sources (spatial components; > 8: the two-pass E-step)
constexpr int kMaxR = 32;       // total spatial rank (the GEM path; the step calls: kStepMaxR)
constexpr int kStepMaxR = 16;   // total spatial rank of fasst_suff_stat / fasst_mix_solve
constexpr int kMaxKP = 128;     // padded NMF components (K > 64: one spectral
                                // component per source, fixed FW, no lambdaCorr / TB)
constexpr int kFwFpc = 64;      // bins per block of the FW update's f-contraction
constexpr int kTile = 16;       // MFMA f64 16x16x4 tile edge
// several spectral components per spatial component: source j's NMF columns
// are cut into <= kMaxBlk blocks (one per spectral component); the blocks of
// all sources (the "slots") carry the TW restart flags
constexpr int kMaxBlk = 8, kMaxSlot = 16;
constexpr int kMaxTB = 64;  // time blobs per spectral component
constexpr int kFlagHalt = 1 + kMaxSlot, kFlagIter = 2 + kMaxSlot, kNFlags = 3 + kMaxSlot;
#ifndef FASST_FPW
#define FASST_FPW 2
#endif
#ifndef FASST_TPW
#define FASST_TPW 2
#endif
constexpr int kFPW = FASST_FPW;  // bin tiles per wave, FB contraction
constexpr int kTPW = FASST_TPW;  // frame tiles per wave, TW contraction

typedef double d4 __attribute__((ext_vector_type(4)));

void set_error(const char *fmt, ...);

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// blocks of 256 threads for a grid-stride loop over n elements, at most `cap`
// (kernels that fix their summation order by grid keep the cap they had)
inline int egrid(size_t n, size_t cap = 8192) {
  const size_t b = (n + 255) / 256;
  return (int)(b < cap ? b : cap);
}

#define FASST_HIP(call)                                                      \
  do {                                                                       \
    hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) {                                                  \
      ::fasst::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call,          \
                         hipGetErrorString(e_));                             \
      return e_ == hipErrorOutOfMemory ? FASST_ERR_OOM : FASST_ERR_DEVICE;   \
    }                                                                        \
  } while (0)

#define FASST_LAUNCH_CHECK()                                                 \
  do {                                                                       \
    hipError_t e_ = hipGetLastError();                                       \
    if (e_ != hipSuccess) {                                                  \
      ::fasst::set_error("%s:%d kernel launch: %s", __FILE__, __LINE__,      \
                         hipGetErrorString(e_));                             \
      return FASST_ERR_DEVICE;                                               \
    }                                                                        \
  } while (0)

// Scoped device selection (restores the caller's device).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A non-blocking stream of the current device owned by a call's scope: drained
// and destroyed with it, so every return after create() leaves nothing queued.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  int create() {
    FASST_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return FASST_OK;
  }
  ~Stream() {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
};

// Up to three HIP events owned by a call's scope or by a context and destroyed
// with it, so no error return after create() can leak them.
struct Events {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  Events() = default;
  Events(const Events &) = delete;
  Events &operator=(const Events &) = delete;
  int create(int n) {
    for (int i = 0; i < n; ++i) FASST_HIP(hipEventCreate(&e[i]));
    return FASST_OK;
  }
  // the timer of one call: create e[0] and e[1], record e[0] on `stream`
  int start(hipStream_t stream) {
    int st = create(2);
    if (st) return st;
    FASST_HIP(hipEventRecord(e[0], stream));
    return FASST_OK;
  }
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// Record `end` on `stream`, wait for it, *ms = the device time since `start`.
inline int elapsed_ms(hipEvent_t start, hipEvent_t end, hipStream_t stream, float *ms) {
  FASST_HIP(hipEventRecord(end, stream));
  FASST_HIP(hipEventSynchronize(end));
  FASST_HIP(hipEventElapsedTime(ms, start, end));
  return FASST_OK;
}

// Return a callee's non-zero status from the calling function.
#define FASST_TRY(expr)                                                      \
  do {                                                                       \
    int st_ = (expr);                                                        \
    if (st_) return st_;                                                     \
  } while (0)

// The bounds rule of every host transfer, in elements: `rows` rows of `width`,
// `host_pitch` apart on the host and `dev_pitch` apart on the device, lie in a
// device span of `n`.  A linear copy of `count` is one row of pitch `count`.
constexpr bool span_fits(size_t n, size_t rows, size_t width, size_t host_pitch,
                         size_t dev_pitch) {
  return rows == 0 || width == 0 ||
         (width <= host_pitch && width <= dev_pitch && width <= n &&
          rows - 1 <= (n - width) / dev_pitch);
}
static_assert(span_fits(12, 1, 12, 12, 12), "exact fit");
static_assert(!span_fits(12, 1, 13, 13, 13), "one element over");
static_assert(span_fits(0, 0, 5, 5, 16) && span_fits(0, 3, 0, 0, 0), "rows == 0, width == 0");
static_assert(!span_fits(0, 1, 1, 1, 1), "anything into an empty span");
static_assert(span_fits(48, 3, 16, 16, 16), "width == pitch");
static_assert(!span_fits(48, 3, 16, 16, 15) && !span_fits(48, 3, 16, 15, 16), "width > pitch");
static_assert(span_fits(37, 3, 5, 5, 16), "the last row ends exactly at n");
static_assert(!span_fits(36, 3, 5, 5, 16), "the last row ends one past n");
static_assert(span_fits(37, 3, 5, 7, 16), "host pitch above the width");
static_assert(!span_fits(47, 4, 5, 5, 16) && span_fits(53, 4, 5, 5, 16), "four rows");
static_assert(!span_fits(4, 2, 3, 3, 0), "zero device pitch");
static_assert(!span_fits(~(size_t)0, 3, 5, 5, ~(size_t)0 / 2 + 1), "no wrap-around in rows * pitch");

// Non-owning view of `n` elements of device memory, the one host transfer path:
// every count, width and pitch is in elements of T, checked with span_fits
// (FASST_ERR_SHAPE, nothing copied); an empty transfer does nothing.  Without a
// stream a call blocks (hipMemcpy, hipMemcpy2D, hipMemset); with one it is queued
// on it.  The host pointer is untyped: the C ABI passes double2 arrays as double *.
template <typename T>
struct DSpan {
  T *p = nullptr;
  size_t n = 0;
  // the part from `off` (of `count`); empty, so refusing a transfer, if outside
  DSpan at(size_t off) const { return off <= n ? DSpan{p + off, n - off} : DSpan{}; }
  DSpan at(size_t off, size_t count) const {
    return off <= n && count <= n - off ? DSpan{p + off, count} : DSpan{};
  }
  int fits(size_t rows, size_t width, size_t hp, size_t dp, const char *what) const {
    if (span_fits(n, rows, width, hp, dp)) return FASST_OK;
    set_error("DSpan::%s: %zu rows of %zu elements, pitch %zu (host %zu), the span holds %zu",
              what, rows, width, dp, hp, n);
    return FASST_ERR_SHAPE;
  }
  int put(const void *host, size_t count) const {
    FASST_TRY(fits(1, count, count, count, "put"));
    if (count) FASST_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return FASST_OK;
  }
  int put(const void *host, size_t count, hipStream_t stream) const {
    FASST_TRY(fits(1, count, count, count, "put"));
    if (count) FASST_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, stream));
    return FASST_OK;
  }
  int get(void *host, size_t count) const {
    FASST_TRY(fits(1, count, count, count, "get"));
    if (count) FASST_HIP(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost));
    return FASST_OK;
  }
  int get(void *host, size_t count, hipStream_t stream) const {
    FASST_TRY(fits(1, count, count, count, "get"));
    if (count) FASST_HIP(hipMemcpyAsync(host, p, count * sizeof(T), hipMemcpyDeviceToHost, stream));
    return FASST_OK;
  }
  // `rows` rows of `width` elements between a host matrix of row pitch `hp`
  // and a device image of row pitch `dp`
  int put_rows(const void *host, size_t rows, size_t width, size_t hp, size_t dp) const {
    FASST_TRY(fits(rows, width, hp, dp, "put_rows"));
    if (rows && width)
      FASST_HIP(hipMemcpy2D(p, dp * sizeof(T), host, hp * sizeof(T), width * sizeof(T), rows,
                            hipMemcpyHostToDevice));
    return FASST_OK;
  }
  int put_rows(const void *host, size_t rows, size_t width, size_t hp, size_t dp,
               hipStream_t stream) const {
    FASST_TRY(fits(rows, width, hp, dp, "put_rows"));
    if (rows && width)
      FASST_HIP(hipMemcpy2DAsync(p, dp * sizeof(T), host, hp * sizeof(T), width * sizeof(T), rows,
                                 hipMemcpyHostToDevice, stream));
    return FASST_OK;
  }
  int get_rows(void *host, size_t rows, size_t width, size_t hp, size_t dp) const {
    FASST_TRY(fits(rows, width, hp, dp, "get_rows"));
    if (rows && width)
      FASST_HIP(hipMemcpy2D(host, hp * sizeof(T), p, dp * sizeof(T), width * sizeof(T), rows,
                            hipMemcpyDeviceToHost));
    return FASST_OK;
  }
  int get_rows(void *host, size_t rows, size_t width, size_t hp, size_t dp,
               hipStream_t stream) const {
    FASST_TRY(fits(rows, width, hp, dp, "get_rows"));
    if (rows && width)
      FASST_HIP(hipMemcpy2DAsync(host, hp * sizeof(T), p, dp * sizeof(T), width * sizeof(T), rows,
                                 hipMemcpyDeviceToHost, stream));
    return FASST_OK;
  }
  int zero(size_t count) const {
    FASST_TRY(fits(1, count, count, count, "zero"));
    if (count) FASST_HIP(hipMemset(p, 0, count * sizeof(T)));
    return FASST_OK;
  }
  int zero(size_t count, hipStream_t stream) const {
    FASST_TRY(fits(1, count, count, count, "zero"));
    if (count) FASST_HIP(hipMemsetAsync(p, 0, count * sizeof(T), stream));
    return FASST_OK;
  }
};

// Device buffer owned by a context or a call's scope; freed in the destructor.
// put / get / zero go through the span over the whole buffer; a part of it, and
// every pitched copy, names its span: at(off).get(..), at(0).put_rows(..).
template <typename T>
struct DBuf {
  T *p = nullptr;
  size_t n = 0;
  DSpan<T> at(size_t off) const { return DSpan<T>{p, n}.at(off); }
  DSpan<T> at(size_t off, size_t count) const { return DSpan<T>{p, n}.at(off, count); }
  int put(const void *host, size_t count) { return at(0).put(host, count); }
  int put(const void *host, size_t count, hipStream_t stream) { return at(0).put(host, count, stream); }
  int get(void *host, size_t count) const { return at(0).get(host, count); }
  int get(void *host, size_t count, hipStream_t stream) const { return at(0).get(host, count, stream); }
  int zero(size_t count) const { return at(0).zero(count); }
  int zero(size_t count, hipStream_t stream) const { return at(0).zero(count, stream); }
  // a fresh buffer of exactly the uploaded elements: no zero fill, no sync
  int upload(const void *host, size_t count) {
    FASST_TRY(alloc_uninit(count));
    return put(host, count);
  }
  int upload(const void *host, size_t count, hipStream_t stream) {
    FASST_TRY(alloc_uninit(count));
    return put(host, count, stream);
  }
  int alloc(size_t count) {
    release();
    if (count == 0) return FASST_OK;
    FASST_HIP(hipMalloc(&p, count * sizeof(T)));
    n = count;
    // zero-fill and wait: the context stream is non-blocking, so a pending
    // null-stream memset could otherwise land after later stream work
    FASST_HIP(hipMemset(p, 0, count * sizeof(T)));
    FASST_HIP(hipDeviceSynchronize());
    return FASST_OK;
  }
  // scratch that every reader writes before it reads: no zero-fill, no sync
  int alloc_uninit(size_t count) {
    release();
    if (count == 0) return FASST_OK;
    FASST_HIP(hipMalloc(&p, count * sizeof(T)));
    n = count;
    return FASST_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DBuf() { release(); }
};

}  // namespace fasst
