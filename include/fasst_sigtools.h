/*
 * fasst_sigtools.h -- C ABI of the signal tools (libfasst_hip.so): the
 * reference's tools/signalTools.py prinComp2D (:26-118), medianFilter
 * (:13-24), f0detectionFunction (:198-318) and invHermMat2D (:120-131).
 *
 * Stateless calls on a device index.  Every call exists twice: `sig_x` takes
 * host pointers (allocates, copies, runs, copies back) and `sig_x_dev` takes
 * device pointers for EVERY array argument (planes already in HBM are used
 * where they lie; the call returns after the kernels have finished).  Small
 * scalar results (flags, counts) are always written to host memory.
 * Conventions: fasst_hip.h (status codes, the last-error text, complex128 as
 * interleaved doubles, row-major).  All arithmetic is FP64 and every
 * reduction has a fixed order: two runs give the same bits.
 *
 * sig_pca2d: 2x2 local PCA of two complex planes x0, x1 [F][N] over windows of
 *   neighbor_nb frames, L = N - neighbor_nb + 1 windows per bin:
 *     c0 = |sum |x0|^2| / (nb-1), c1 = |sum |x1|^2| / (nb-1),
 *     c01 = sum x0 conj(x1) / (nb-1)     (direct sums, ascending frame)
 *   then the reference's closed form: tra, det, delta = sqrt(tra^2 - 4 det),
 *   lambda_M/m = (tra +- delta)/2, v = (c01, lambda - c0) / den with
 *   v_M = (1, 0), v_m = (0, 1) where den == 0.
 *   lambda_M, lambda_m [F][L] real; v_M, v_m [2][F][L] complex128.
 *   flags[0] / flags[1] != 0: some lambda_M / lambda_m is negative.
 *   1 <= neighbor_nb <= min(N, SIG_PCA_MAX_NEIGHBORS).
 *
 * sig_median: rows in [R][N]; out[r][n] is the median of
 *   in[r][max(n-length,0) : min(n+length, N-1)] (end exclusive: the last
 *   sample is in no window), the mean of the two middle values for an even
 *   count; an empty window, a window holding a NaN or a NaN result gives
 *   out[r][n] = in[r][n].  length >= 0, no upper limit.
 *
 * sig_hsum: harmonic sum (prod == 0) or product (prod != 0) salience.
 *   tf [F][T] magnitudes, weights [F]; the bins of harmonic h of F0 number i
 *   are bin_idx[bin_ptr[i*n_harm + h] .. bin_ptr[i*n_harm + h + 1]) (a CSR
 *   list built on the host with the reference's own threshold test, so the
 *   selection is exact); bin_ptr has n_f0*n_harm + 1 entries, nnz = its last.
 *     hs[i][t] = sum or prod over the harmonics h that have bins of
 *                max_b(weights[b] tf[b][t]) / sum_f tf[f][t];   0 if none has.
 *   hs [n_f0][T].
 *
 * sig_invherm: element-wise inverse of n 2x2 Hermitian matrices,
 *   det = a00 a11 - |a01|^2 (no floor), i00 = a11/det, i01 = -a01/det,
 *   i11 = a00/det.  a00, a11 real [n]; a01 and i01 complex128 [n] when
 *   off_complex != 0, else real [n].  *n_zero_det counts det == 0.
 */
#ifndef FASST_SIGTOOLS_H
#define FASST_SIGTOOLS_H

#include "fasst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIG_PCA_MAX_NEIGHBORS 4096

int sig_pca2d(int device, int F, int N, int neighbor_nb, const double *x0, const double *x1,
              double *lambda_M, double *lambda_m, double *v_M, double *v_m, int *flags);
int sig_pca2d_dev(int device, int F, int N, int neighbor_nb, const double *x0, const double *x1,
                  double *lambda_M, double *lambda_m, double *v_M, double *v_m, int *flags);

int sig_median(int device, int R, int N, int length, const double *in, double *out);
int sig_median_dev(int device, int R, int N, int length, const double *in, double *out);

int sig_hsum(int device, int F, int T, int n_f0, int n_harm, const double *tf,
             const double *weights, const int *bin_ptr, const int *bin_idx, int prod, double *hs);
/* nnz: the length of bin_idx (the host call reads it from bin_ptr) */
int sig_hsum_dev(int device, int F, int T, int n_f0, int n_harm, const double *tf,
                 const double *weights, const int *bin_ptr, const int *bin_idx, int nnz, int prod,
                 double *hs);

int sig_invherm(int device, long n, int off_complex, const double *a00, const double *a01,
                const double *a11, double *i00, double *i01, double *i11, int *n_zero_det);
int sig_invherm_dev(int device, long n, int off_complex, const double *a00, const double *a01,
                    const double *a11, double *i00, double *i01, double *i11, int *n_zero_det);

/* device time (HIP events) of the kernels of the last sig_* call, without copies */
int sig_last_ms(double *device_ms);

/* kernels launched from fasst_sigtools.hip by this process so far */
int sig_launch_count(long *count);

#ifdef __cplusplus
}
#endif

#endif /* FASST_SIGTOOLS_H */
