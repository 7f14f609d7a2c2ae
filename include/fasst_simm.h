/*
 * fasst_simm.h -- C ABI of the SIMM source/filter engine (libfasst_hip.so).
 *
 * Replaces the multiplicative-update loops of the reference's
 * SeparateLeadStereo/SIMM/SIMM.py:
 *   Stereo_SIMM (SIMM.py:397-943)  -> simm_create(stereo=1) + simm_run
 *   SIMM        (SIMM.py:46-395)   -> simm_create(stereo=0) + simm_run
 * The random initialisation stays on the host (it draws from NumPy's global
 * stream in the reference, SIMM.py:200-255 / :525-576), so the Python host
 * side (pyfasst_amd/SeparateLeadStereo/SIMM/SIMM.py) reproduces it exactly
 * and hands the initial parameters over with simm_set_params.
 *
 * Conventions are those of fasst_hip.h: float64, C order, host arrays copied
 * in and out, status codes FASST_*, message in fasst_last_error().
 *   SXR, SXL : [F][N]   power spectrograms (mono: SXR only, SXL NULL)
 *   WF0      : [F][NF0] source comb dictionary
 *   WGAMMA   : [F][P]   smooth filter atoms
 *   HGAMMA [P][K], HPHI [K][N], HF0 [NF0][N], HM [R][N], WM [F][R]
 *   alpha [2] = (alphaR, alphaL), betaR/betaL [R] (the diagonals the
 *   reference returns as np.diag matrices, SIMM.py:943)
 */
#ifndef FASST_SIMM_H
#define FASST_SIMM_H

#include "fasst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct simm_ctx simm_ctx;

/* sizes of SIMM.py:498-504 / :147-153; K <= 8, P*K <= 512.  Mono needs
 * R == 1 or R == N (quirk N7, SIMM.py:388), else FASST_ERR_SHAPE.        */
int simm_create(int device, int F, int N, int NF0, int P, int K, int R, int stereo,
                simm_ctx **out);
int simm_destroy(simm_ctx *ctx);

/* the data to be fitted and the fixed dictionaries (SIMM.py:397-403);
 * SXR / SXL may be NULL when only simm_separate is wanted                  */
int simm_set_data(simm_ctx *ctx, const double *SXR, const double *SXL, const double *WF0,
                  const double *WGAMMA);

/* initial parameters (SIMM.py:525-576); alpha and betaR / betaL are read for
 * stereo only (alpha = (0.5, 0.5) in the reference; betaL NULL means
 * 1 - betaR, :575-576).
 * Builds WPHI, SF0, SPHI and the model spectrograms (:578-585).           */
int simm_set_params(simm_ctx *ctx, const double *HGAMMA, const double *HPHI, const double *HF0,
                    const double *HM, const double *WM, const double *alpha,
                    const double *betaR, const double *betaL);

/* n_iter iterations of the reference loop body (:613-941 / :278-393);
 * omega = updateRulePower; update_hgamma = updateHGAMMA (stereo only).
 * reco_err (may be NULL): [2*n_iter] Itakura-Saito errors after the HF0 and
 * the HPHI update of each iteration (computeError=True, :676-683, :721-728). */
int simm_run(simm_ctx *ctx, int n_iter, double omega, int update_hgamma, double *reco_err);

/* ISDistortion(SXR, hatSXR) [+ ISDistortion(SXL, hatSXL)] of the current
 * model (SIMM.py:34-44, :602-603)                                          */
int simm_reco_error(simm_ctx *ctx, double *out);

/* writeSeparatedSignals masks (SeparateLeadStereo/SeparateLeadStereoTF.py:
 * 1762-1846) from the current parameters: XR, XL complex128 [F][N] mixture
 * STFTs -> lead VR, VL and accompaniment MR, ML complex128 [F][N] (stereo). */
int simm_separate(simm_ctx *ctx, const double *XR, const double *XL, double *VR, double *VL,
                  double *MR, double *ML);

/* current parameters; any pointer may be NULL (alpha/beta: stereo only) */
int simm_get_params(simm_ctx *ctx, double *HGAMMA, double *HPHI, double *HF0, double *HM,
                    double *WM, double *alpha, double *betaR, double *betaL);

/* NF0-sized products (SF0 = WF0 HF0 and WF0^T [num | den], SIMM.py:623-674,
 * :799) dispatched since the library was loaded, per kernel: the
 * hand-written k_dgemm2 (the default) and the generic k_gemm
 * (FASST_SIMM_GEMM=2); either pointer may be NULL */
int simm_nf0_product_counts(long *dgemm2_launches, long *kgemm_launches);

/*
 * stereo_NMF (SIMM.py:945-1104): the accompaniment model on its own,
 *   SXR ~ WM diag(betaR^2) HM,  SXL ~ WM diag(betaL^2) HM,  betaL = 1 - betaR,
 * a stereo Itakura-Saito NMF with one panning gain per component.  The
 * initial draw stays on the host (pyfasst_amd/SeparateLeadStereo/SIMM/SIMM.py
 * stereo_NMF); the loop body (:1009-1102) runs on the device with no model
 * plane stored (pyfasst_amd/csrc/fasst_snmf.hip).
 *   SXR, SXL [F][N], WM [F][R], HM [R][N], betaR / betaL [R] (the diagonals)
 */
typedef struct snmf_ctx snmf_ctx;

/* 1 <= R <= 128, else FASST_ERR_UNSUPPORTED */
int snmf_create(int device, int F, int N, int R, snmf_ctx **out);
int snmf_destroy(snmf_ctx *ctx);
int snmf_set_data(snmf_ctx *ctx, const double *SXR, const double *SXL);
/* initial parameters (SIMM.py:968-991); betaL = 1 - betaR */
int snmf_set_params(snmf_ctx *ctx, const double *WM, const double *HM, const double *betaR);
/* n_iter iterations; omega = updateRulePower.  reco_err (may be NULL):
 * [3 * n_iter + 1], ISDistortion(SXR, hatSXR) + ISDistortion(SXL, hatSXL)
 * before the loop and after the HM, WM and beta step of each iteration
 * (:1001, :1036, :1065, :1095), computed on the device only when asked for */
int snmf_run(snmf_ctx *ctx, int n_iter, double omega, double *reco_err);
/* current parameters; any pointer may be NULL */
int snmf_get_params(snmf_ctx *ctx, double *WM, double *HM, double *betaR, double *betaL);

#ifdef __cplusplus
}
#endif

#endif /* FASST_SIMM_H */
