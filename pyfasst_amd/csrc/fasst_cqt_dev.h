// Device-side seam between the model context (fasst_ctx) and the CQT / MinQT
// context (cqt_ctx): the batched rasterised transform reads and writes the
// model's frame-major planes in place, so no F x T array crosses to the host
// (fasst_set_audio_cqt, fasst_*_waveforms_cqt; include/fasst_cqt.h).
#pragma once
#include "fasst_common.h"

struct cqt_ctx;

namespace fasst {

// c = g0 x0 + g1 x1 (one row of a 2 x 2 gain applied to the two channels)
__device__ __forceinline__ double2 gain_apply(double2 g0, double2 g1, double2 x0, double2 x1) {
  return make_double2(g0.x * x0.x - g0.y * x0.y + (g1.x * x1.x - g1.y * x1.y),
                      g0.x * x0.y + g0.y * x0.x + (g1.x * x1.y + g1.y * x1.x));
}

// The B images a batched inverse reads, frame-major with row pitch ld:
//   G == nullptr  image b is S + b * plane (Wiener images [B][Tp][Fp], or the
//                 single [W][F] raster of cqt_inverse with B = 1);
//   G != nullptr  S is the resident channel pair X [2][plane] and image
//                 b = (n, channel) is G_n[channel][0] X0 + G_n[channel][1] X1,
//                 formed as it is loaded (G [J][2][2][gp], the time-invariant
//                 spatial filter): no image array exists.
struct CqtImages {
  const double2 *S = nullptr;
  size_t plane = 0;
  int ld = 0;
  const double2 *G = nullptr;
  int gp = 0;
};

__device__ __forceinline__ double2 image_at(const CqtImages &im, int b, long col, int row) {
  const size_t o = (size_t)col * im.ld + row;
  if (!im.G) return im.S[b * im.plane + o];
  const double2 *g = im.G + (size_t)(2 * b) * im.gp + row;
  return gain_apply(g[0], g[im.gp], im.S[o], im.S[im.plane + o]);
}

int cqt_ctx_device(const cqt_ctx *q);
// FASST_ERR_SHAPE unless q is on `device` and transforms L samples to F x T
int cqt_match_model(cqt_ctx *q, long L, int device, int F, int T, const char *fn);
// data [L][2] (host) -> both channel transforms into X [2][plane], row pitch
// ld, on stream s, in one batched forward chain; X must be zero where the
// transform leaves it unwritten (the caller clears it on s first).  Returns
// with s idle.
int cqt_forward_pair(cqt_ctx *q, hipStream_t s, const double *data, long L, double2 *X, int ld,
                     size_t plane);
// B images -> y [B][L] (host) on stream s, in one batched inverse chain.
// Returns with s idle.
int cqt_inverse_batch(cqt_ctx *q, hipStream_t s, const CqtImages &im, int B, long L, double *y);

}  // namespace fasst
