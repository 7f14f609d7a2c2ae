/*
 * fasst_filter.h -- C ABI of the fused STFT-domain filter (libfasst_hip.so):
 * the reference's tftransforms/stft.py filter_stft (:133-227) and
 * filter_conv_stft (:229-334).  Each frame is analysed, multiplied by the
 * M_out x M_in matrix of every bin and overlap-added; no spectrogram is kept.
 *
 * Stateless calls on a device index.  Conventions: fasst_hip.h (status codes,
 * the last-error text, complex128 as interleaved doubles, row-major).  All
 * arithmetic is FP64 and the overlap-add is a gather in frame order: two runs
 * give the same bits.
 *
 *   data   [L][M_in]       samples, channels fastest (NumPy [T, M] order)
 *   W      complex128, the filter of output channel o, input channel c:
 *            w_tv == 0                    [M_out][M_in][F]
 *            w_tv != 0, FILTER_W_NUMPY    [M_out][M_in][F][n_w_frames]
 *            w_tv != 0, FILTER_W_FRAMES   [M_out][M_in][n_w_frames][F]
 *          F = nfft/2 + 1.  The imaginary parts of bins 0 and nfft/2 of the
 *          product are dropped, as numpy.fft.irfft does.
 *   awin, swin [wlen]      analysis and synthesis windows
 *   y_out  [*len_out][M_out]
 *
 * Framing: n_frames = ceil(L / hop), frame 0 centred on sample 0 (wlen/2
 * leading zeros), *len_out = (n_frames-1) hop + wlen - wlen/2, which is in
 * general not L.  Each output sample is divided by the sum of swin*awin over
 * the frames that cover it (zeros -> 1).  A time-varying W needs
 * n_w_frames >= n_frames; the surplus is ignored.
 *
 * Refused on the host, before any device call:
 *   FASST_ERR_SHAPE        bad sizes, nfft < wlen or > 8192, too few W frames,
 *                          M_out or M_in * M_out above 65535,
 *                          a hop so large that wlen/2 + L passes the framed
 *                          length (the reference's negative tail padding)
 *   FASST_ERR_UNSUPPORTED  nfft not a power of two; the frame's LDS form past
 *                          FILTER_LDS_BYTES:  P = ceil(max(M_in, M_out)/2)
 *                          complex buffers of nfft when M_in <= FILTER_REG_M
 *                          (in place), ceil(M_in/2) + ceil(M_out/2) otherwise
 *
 * With y_out == NULL a call only validates and returns *len_out.
 * fasst_filter_stft takes host pointers (allocates, copies, runs, copies back).
 * fasst_filter_stft_dev takes device pointers for every array, runs on
 * `stream` (a hipStream_t, NULL for the default stream) and returns after the
 * kernels have finished; the FILTER_W_NUMPY layout of a time-varying W costs
 * one tiled transpose into FILTER_W_FRAMES (a read and a write of W), which a
 * producer on the device avoids by writing FILTER_W_FRAMES itself.
 */
#ifndef FASST_FILTER_H
#define FASST_FILTER_H

#include "fasst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FILTER_W_NUMPY 0
#define FILTER_W_FRAMES 1
#define FILTER_REG_M 8
#define FILTER_LDS_BYTES (160 * 1024)

int fasst_filter_stft(int device, const double *data, int L, int M_in, int M_out, const double *W,
                      int w_tv, int n_w_frames, const double *awin, const double *swin, int wlen,
                      int nfft, int hop, double *y_out, int *len_out);
int fasst_filter_stft_dev(int device, const double *data, int L, int M_in, int M_out,
                          const double *W, int w_tv, int n_w_frames, const double *awin,
                          const double *swin, int wlen, int nfft, int hop, double *y_out,
                          int *len_out, int w_layout, void *stream);

/* Measurement only (tools/bench_aux.py).  fasst_filter_set_timing(1) makes the
 * calling thread's later fasst_filter_stft* calls record HIP events around
 * their kernels; fasst_filter_last_ms then returns that thread's last call's
 * device time: total, and the share of the W transpose (0 when none ran).
 * Off by default: no events are created.  Flag and figures are per thread. */
int fasst_filter_set_timing(int on);
int fasst_filter_last_ms(double *total_ms, double *transpose_ms);

#ifdef __cplusplus
}
#endif

#endif /* FASST_FILTER_H */
