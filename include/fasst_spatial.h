/*
 * fasst_spatial.h -- C ABI of the spatial package (libfasst_hip.so): the
 * reference's spatial/steering_vectors.py and spatial/dirdiag.py.
 *
 * Conventions: fasst_hip.h (status codes, the last-error text, complex128 as
 * interleaved doubles, row-major).  All arithmetic is FP64 and every
 * reduction has a fixed order: two runs give the same bits.  The stateless
 * calls take host pointers and a device index; the two calls on a model
 * context read its resident observation where it lies.
 *
 * Far-field phase of sensor m of a uniform linear array, in the reference's
 * product order (steering_vectors.py:48-52):
 *     y(m, f, theta) = ((-2 pi * (m * freqs[f])) * k) * sin_theta,
 *     a = (cos y, sin y),      k = distanceInterMic / soundCelerity.
 * The callers pass k and sin(theta) as NumPy forms them on the host, so the
 * argument of the sine / cosine pair is the reference's own, bit for bit.
 *
 * steer_ula:     out [ntheta][nch][F] complex = a(m, f, theta).
 * steer_acous:   out [nch][F] complex = g[m] * exp(-2 pi i dist[m] freqs[f] / c),
 *                g[m] = 1 / (sqrt(4 pi) dist[m])  (steering_vectors.py:66-73).
 * cx_tmean:      mean [4][F] = the time means of Cx[0], Re Cx[1], Im Cx[1] and
 *                Cx[2] of the resident observation.  Frames are summed in
 *                chunks of 64 in ascending order, the chunks in ascending
 *                order, then divided by T: the order depends on T alone.
 * dir_diag:      dir_diag_stereo (steering_vectors.py:76-160) on the resident
 *                observation: cx_tmean, the clamped 2x2 Hermitian inverse
 *                (inv_herm_mat_2d), then
 *                  D[theta][f] = |a0^2| i00 + |a1^2| i11 + 2 Re(conj(a0) a1 i01).
 *                diagram [ntheta][F], det [F] (the clamped determinants: the
 *                caller raises the reference's ValueError where one is 0),
 *                mean [4][F] or NULL.
 * ula_response:  directivity_filter_diagram_ULA's loop (dirdiag.py:113-121):
 *                  diagram[theta][f] = |sum_m w[m][f] a(m, f, theta) / sqrt(n)|^2,
 *                m ascending, w [n][F] complex.  n <= FASST_SPATIAL_MAX_SENSORS,
 *                FASST_ERR_UNSUPPORTED above.
 * mvdr_target:   make_MVDR_filter_target (dirdiag.py:36-68) for stereo:
 *                target [F][2] complex, interf [n_interf][F][2] complex,
 *                w [2][F] complex.  No determinant floor (invHermMat2D).
 */
#ifndef FASST_SPATIAL_H
#define FASST_SPATIAL_H

#include "fasst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FASST_SPATIAL_MAX_SENSORS 64

/* slots of fasst_spatial_launch_count / fasst_spatial_last_ms */
#define FASST_SPATIAL_K_STEER_ULA 0
#define FASST_SPATIAL_K_STEER_ACOUS 1
#define FASST_SPATIAL_K_CX_TMEAN 2
#define FASST_SPATIAL_K_CAPON 3
#define FASST_SPATIAL_K_ULA_RESPONSE 4
#define FASST_SPATIAL_K_MVDR_TARGET 5
#define FASST_SPATIAL_NK 6

int fasst_steer_ula(int device, int nch, int F, int ntheta, const double *freqs,
                    const double *sin_theta, double k, double *out);
int fasst_steer_acous(int device, int nch, int F, const double *freqs, const double *dist,
                      double celerity, double *out);
int fasst_cx_tmean(fasst_ctx *c, double *mean);
int fasst_dir_diag(fasst_ctx *c, int ntheta, const double *freqs, const double *sin_theta,
                   double k, double *diagram, double *det, double *mean);
int fasst_ula_response(int device, int n, int F, int ntheta, const double *w, const double *freqs,
                       const double *sin_theta, double k, double *diagram);
int fasst_mvdr_target(int device, int F, int n_interf, const double *target, const double *interf,
                      double *w);

/* kernels launched from fasst_spatial.hip by this process so far, per slot
 * (the time mean counts its partial and its combine launch) */
int fasst_spatial_launch_count(long *counts);
/* device time (HIP events) of the last launch of each slot, without copies */
int fasst_spatial_last_ms(double *ms);
/* bytes these calls have copied between host and device so far */
int fasst_spatial_transfer_bytes(long *bytes);

#ifdef __cplusplus
}
#endif

#endif /* FASST_SPATIAL_H */
