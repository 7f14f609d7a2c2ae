/*
 * fasst_nsgt.h -- C ABI of the non-stationary Gabor transform (libfasst_hip.so):
 * the reference's tftransforms/nsgt (nsgtf.py, nsigtf.py), whole-signal and
 * sliced (slicq.py), and the FFT of any length it stands on.
 *
 * Conventions: fasst_hip.h (status codes, the last-error text, complex128 as
 * interleaved doubles).  All arithmetic is FP64.  The overlap-add of the
 * inverse is a gather in ascending band order: two runs give the same bits.
 *
 * A plan holds the windows of all `nbands` bands (both halves of the
 * spectrum), their lengths M[k] (time channels), Lg[k] (window lengths),
 * start[k] (the first spectrum bin of the window, wins[k][0], in [0, nn)),
 * and the windows g / dual windows gd, real, packed band after band
 * (sum of Lg doubles each).  `real` and `reducedform` fix the bands a
 * transform uses, the reference's slice
 *     real == 0:  all nbands
 *     real != 0:  reducedform .. nbands/2 + 1 - reducedform
 * and the inverse then forms the mirrored bands on the fly.
 *
 * Coefficients are packed: channel c, used band j (in slice order) at
 *     c * coef_len + sum of M over the used bands before j,
 * M[k] complex values each; coef_len = the sum of M over the used bands.
 *
 *   forward:  x [nch][Ls] real  ->  coef [nch][coef_len] complex
 *   backward: coef              ->  y [nch][Ls], real when the plan is, else
 *                                   complex
 * With is_device != 0 both arrays are device pointers, the call runs on the
 * default stream and returns when the kernels have finished; nothing crosses
 * to the host.  A second call with the same nch allocates nothing.
 *
 * FFT lengths: a power of two up to 4096 is one FFT in LDS; a larger power of
 * two (up to 2^24) is the four-step method; any other length N is Bluestein's
 * convolution of size nextpow2(2N-1) on those two.  Hence the ceilings
 * Ls, nn, M[k] <= FASST_NSGT_MAX_N.
 *
 * Refused on the host, before any device call:
 *   FASST_ERR_SHAPE        nbands < 1 (or odd with real), Ls < 1, nn < Ls,
 *                          M[k] < 1, Lg[k] < 2 or > nn, start outside [0, nn),
 *                          a used band with M[k] < Lg[k]/2 (the inverse's
 *                          slices would not fit), nch < 1, a null pointer
 *   FASST_ERR_UNSUPPORTED  Ls, nn or M[k] above FASST_NSGT_MAX_N
 *
 * fasst_nsgt_fft: out[k] = sum_n in[n] exp(sign 2 pi i n k / N), sign = -1 or
 * +1, no scaling, host pointers, N <= FASST_NSGT_MAX_N (a power of two up to
 * 2^24).
 *
 * The sliced transform (the reference's slicq.py, slicing.py, unslicing.py): a
 * stream of any length is cut into half-overlapping slices of sl_len = 4 hhop
 * samples under a Tukey window whose transitions of tr_area samples are centred
 * on hhop and 3 hhop; every slice is one more channel of a plan with
 * Ls = sl_len, and the inverse adds the overlapping halves back.  A sliced
 * plan is a plan (fasst_nsgt_coef_len and fasst_nsgt_plan_destroy take it)
 * plus the slicing window slwnd [sl_len] and, optionally, the synthesis window
 * recwnd [sl_len] (null: the slices are added as they are), both in stream
 * order.
 *
 * The stream is counted in quarter-blocks of hhop samples: two zero blocks,
 * the signal (its last block zero-filled), zero blocks behind.  Slice s takes
 * blocks 2s .. 2s+3.  One call transforms `nslices` consecutive slices of
 * `nchan` channels from slice first_slice_index on (only its parity matters:
 * odd and even slices store their quarters, and rotate their bands, in
 * opposite ways).
 *   sliced_forward:  blocks: per channel the 2 nslices + 2 quarter-blocks
 *                    2 first .. 2 (first + nslices) + 1, channel c at
 *                    blocks + c * blocks_stride (in samples; host arrays are
 *                    packed: blocks_stride = (2 nslices + 2) hhop)
 *                    ->  coef [nslices][nchan][coef_len] complex
 *   sliced_backward: coef  ->  y: per channel the 2 nslices quarter-blocks
 *                    2 first .. 2 (first + nslices) - 1 of the stream, channel
 *                    c at y + c * y_stride samples (host: y_stride =
 *                    2 nslices hhop); real when the plan is, else complex.
 *                    carry_in_out [nchan][2 hhop] samples holds what the slice
 *                    before `first` adds to the first two blocks (zeros before
 *                    slice 0) and returns what slice first + nslices - 1 adds
 *                    to the two blocks after the last; after the last call it
 *                    is the stream's last two blocks.  The sums are formed
 *                    older slice first and each product and sum rounds on its
 *                    own, so the result does not depend on how the slices are
 *                    grouped into calls.
 * Each call launches the kernels of forward / backward plus one, whatever
 * nslices.  Refused on the host: FASST_ERR_SHAPE for sl_len not a multiple of
 * 4, tr_area odd, negative or >= sl_len / 2, an M[k] that is no multiple of 4,
 * a plan that is not sliced, nchan * nslices > 65535, a stride below the run.
 */
#ifndef FASST_NSGT_H
#define FASST_NSGT_H

#include "fasst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FASST_NSGT_MAX_N (1 << 23)

int fasst_nsgt_plan_create(int device, int Ls, int nn, int nbands, const int *M, const int *Lg,
                           const int *start, const double *g, const double *gd, int real,
                           int reducedform, void **plan);
int fasst_nsgt_plan_destroy(void *plan);
int fasst_nsgt_coef_len(void *plan, long *out);
int fasst_nsgt_forward(void *plan, int nch, const double *x, int is_device, double *coef);
int fasst_nsgt_backward(void *plan, int nch, const double *coef, int is_device, double *y);
int fasst_nsgt_fft(int device, int n, int sign, const double *in, double *out);

int fasst_nsgt_sliced_plan_create(int device, int sl_len, int tr_area, int nn, int nbands,
                                  const int *M, const int *Lg, const int *start, const double *g,
                                  const double *gd, int real, int reducedform, const double *slwnd,
                                  const double *recwnd, void **plan);
int fasst_nsgt_sliced_forward(void *plan, int nchan, int nslices, int first_slice_index,
                              const double *blocks, long blocks_stride, int is_device,
                              double *coef);
int fasst_nsgt_sliced_backward(void *plan, int nchan, int nslices, int first_slice_index,
                               const double *coef, double *carry_in_out, int is_device, double *y,
                               long y_stride);

/* Kernel launches of this unit since the library was loaded (all threads). */
int fasst_nsgt_launch_count(long *count);
/* Measurement only.  fasst_nsgt_set_timing(1) makes the calling thread's later
 * forward / backward calls record HIP events around their kernels;
 * fasst_nsgt_last_ms returns that thread's last call's device time: total,
 * and the share of the whole-signal FFT (forward: of length Ls; backward: of
 * length nn).  Off by default: no events are created. */
int fasst_nsgt_set_timing(int on);
int fasst_nsgt_last_ms(double *total_ms, double *fft_ms);

#ifdef __cplusplus
}
#endif

#endif /* FASST_NSGT_H */
