/*
 * fasst_demix.h -- C ABI of DEMIX's device side (libfasst_hip.so): the
 * mixing-parameter clustering of the reference's demixTF.py (the feature
 * planes of comp_pcafeatures / comp_parameters :448-512, the passes of one
 * clustering round :248-388 / :556-564 and of the refinement :566-758).
 *
 * A demix_ctx keeps, for F bins and L = N - neighbors + 1 windows, the four
 * feature planes confidence, theta, phi, thetaVar (float64 [F][L]), the mask
 * of the points still to classify and up to max_clusters cluster masks (byte
 * planes [F][L], 0 / 1) in device memory.  A clustering round moves O(F)
 * numbers; a plane crosses to the host only through demix_get_plane /
 * demix_get_mask, which demix_transfer_count counts.
 * Conventions: fasst_hip.h (status codes, the last-error text, complex128 as
 * interleaved doubles, row-major).  All arithmetic is FP64, every
 * floating-point reduction has a fixed order (two runs give the same bits);
 * counts are integer sums.  The quirks of the reference that the kernels keep
 * are listed in DESIGN.md §7.9.
 *
 * demix_features: x0, x1 complex128 [F][N], the two channels' STFTs (host
 *   pointers; demix_features_dev: device pointers, used where they lie).
 *   Runs sig_pca2d_dev (fasst_sigtools.h) on the resident planes, the
 *   lexicographic complex maximum of mean(X**2) over [:, nb/2 : nb/2 + L]
 *   (two stages, fixed order), and one element-wise kernel for confidence,
 *   theta, phi and thetaVar.  The STFTs and the PCA outputs are freed.
 * demix_init_subset: every point is still to classify.
 * demix_argmax: out[4] = flat index, confidence, theta, phi of the first
 *   maximum of the confidence with classified points counted as 0.
 * demix_theta_pass: the candidate mask (|theta - theta_c| < dist_bound, still
 *   to classify; a NaN bound gives an empty mask) and, per bin,
 *   sums[f][0..2] = sum_t mask/var cos(phi), sum_t mask/var sin(phi),
 *   sum_t mask/var with var == 0 -> eps (compute_temporal, :352-368).
 * demix_delta_pass: cluster mask number `slot` of getTFPointsNearDelta
 *   (:320-350): dist = sqrt(2 (1 - |cos(theta) v0 + sin(theta) e^{j phi}
 *   v1[f]|)) < (sqrt(var) + sqrt(max_err)) * 2.33, the bound 0 where
 *   conf_c < confidence, the centroid's own point forced in; v1 complex128
 *   [F] (host).  only_centroid != 0: the mask is the centroid's point alone.
 *   Clears the mask's points from the set still to classify.
 *   counts[0] = the cluster's size, counts[1] = points still to classify.
 * demix_exclusive: create_exclusive_clusters (:639-667) over the masks
 *   slots[0..n), in that order; sizes[n] out.
 * demix_cluster_sums: for each of the masks slots[0..n) thresholded by
 *   confidence >= thresholds[k]: sums[k][0..3] = sum 1/var, sum theta/var,
 *   sum 1/varBound (estim_bound_var_theta of each point's confidence), count.
 */
#ifndef FASST_DEMIX_H
#define FASST_DEMIX_H

#include "fasst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct demix_ctx demix_ctx;

#define DEMIX_PLANE_CONFIDENCE 0
#define DEMIX_PLANE_THETA 1
#define DEMIX_PLANE_PHI 2
#define DEMIX_PLANE_VAR 3
#define DEMIX_MASK_SUBSET (-1) /* demix_get_mask / demix_set_mask: the set still to classify */
#define DEMIX_MASK_CANDIDATES (-2) /* the candidate mask of the last demix_theta_pass */

int demix_create(int device, int F, int N, int neighbors, int max_clusters, demix_ctx **out);
int demix_destroy(demix_ctx *ctx);

int demix_features(demix_ctx *ctx, const double *x0, const double *x1);
int demix_features_dev(demix_ctx *ctx, const double *x0, const double *x1);

int demix_get_plane(demix_ctx *ctx, int which, double *out);
int demix_set_plane(demix_ctx *ctx, int which, const double *in);
int demix_get_mask(demix_ctx *ctx, int slot, unsigned char *out);
int demix_set_mask(demix_ctx *ctx, int slot, const unsigned char *in);

int demix_init_subset(demix_ctx *ctx);
int demix_argmax(demix_ctx *ctx, double *out);
int demix_theta_pass(demix_ctx *ctx, double theta_c, double dist_bound, double *sums);
int demix_delta_pass(demix_ctx *ctx, int slot, double theta_c, const double *v1, double conf_c,
                     double max_err, long centroid, int only_centroid, long *counts);
int demix_exclusive(demix_ctx *ctx, int n, const int *slots, long *sizes);
int demix_cluster_sums(demix_ctx *ctx, int n, const int *slots, const double *thresholds,
                       double *sums);

/* device time (HIP events) of the kernels of the last demix_* call, without copies */
int demix_last_ms(double *device_ms);
/* kernels launched from fasst_demix.hip by this process so far */
int demix_launch_count(long *count);
/* [F][L] planes and masks copied to the host by this process so far */
int demix_transfer_count(long *count);

#ifdef __cplusplus
}
#endif

#endif /* FASST_DEMIX_H */
