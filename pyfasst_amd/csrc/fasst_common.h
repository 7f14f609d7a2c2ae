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

// Device buffer owned by a context or a call's scope; freed in the destructor.
// The one host transfer path: put / get / upload count elements of T, check
// the count against the allocation (FASST_ERR_SHAPE, nothing copied) and do
// nothing for a count of 0.  Without a stream the copy blocks (hipMemcpy);
// with one it is queued on it (hipMemcpyAsync).  The host pointer is untyped
// because the C ABI passes double2 arrays as double *.
template <typename T>
struct DBuf {
  T *p = nullptr;
  size_t n = 0;
  // FASST_OK when `count` elements lie inside the allocation
  int fits(size_t count, const char *what) const {
    if (count <= n) return FASST_OK;
    set_error("DBuf::%s: %zu elements, the buffer holds %zu", what, count, n);
    return FASST_ERR_SHAPE;
  }
  int put(const void *host, size_t count) {
    FASST_TRY(fits(count, "put"));
    if (count) FASST_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return FASST_OK;
  }
  int put(const void *host, size_t count, hipStream_t stream) {
    FASST_TRY(fits(count, "put"));
    if (count) FASST_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, stream));
    return FASST_OK;
  }
  int get(void *host, size_t count) const {
    FASST_TRY(fits(count, "get"));
    if (count) FASST_HIP(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost));
    return FASST_OK;
  }
  int get(void *host, size_t count, hipStream_t stream) const {
    FASST_TRY(fits(count, "get"));
    if (count) FASST_HIP(hipMemcpyAsync(host, p, count * sizeof(T), hipMemcpyDeviceToHost, stream));
    return FASST_OK;
  }
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
