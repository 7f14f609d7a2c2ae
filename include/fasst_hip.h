/*
 * fasst_hip.h -- C ABI of the MI355X FASST EM engine (libfasst_hip.so).
 *
 * The reference (s-ben/pyfasst) has no FFI layer: its seam is the Python
 * class surface of audioModel.py operating on NumPy state.
 * Each entry point below replaces one reference routine; the Python host
 * side (pyfasst_amd/audioModel.py) binds them with ctypes and keeps the
 * reference's class surface, argument meaning and exceptions.
 *
 * Conventions
 *   - all arrays are host arrays, C (row-major) order, caller-owned, copied in
 *     and out; the library owns every device allocation;
 *   - real data is float64; complex data is complex128 == interleaved
 *     (re, im) float64 pairs, exactly NumPy's memory layout;
 *   - one context = one GPU + one HIP stream; calls on a context are
 *     serialised by the caller; distinct contexts may live on distinct threads;
 *   - every function returns a status code (FASST_OK == 0); the message of
 *     the last failure of the calling thread is in fasst_last_error().
 */
#ifndef FASST_HIP_H
#define FASST_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define FASST_OK               0
#define FASST_ERR_SHAPE        1  /* -> AttributeError / ValueError          */
#define FASST_ERR_SINGULAR     2  /* -> np.linalg.LinAlgError('Singular Matrix'),
                                     audioModel.py:855-863                    */
#define FASST_ERR_DEVICE       3  /* HIP runtime / kernel failure             */
#define FASST_ERR_OOM          4  /* device allocation failed                 */
#define FASST_TW_RESTART       5  /* renormalize_parameters found sum(TW)<eps
                                     (audioModel.py:2023-2028): the host must
                                     draw the random restart and resume       */
#define FASST_ERR_UNSUPPORTED  6  /* model structure outside the HIP path     */

typedef struct fasst_ctx fasst_ctx;

/* ABI revision of this header.  A caller compares fasst_abi_version() with
 * the FASST_ABI_VERSION it was built against and refuses a mismatch (the
 * Python loader does, pyfasst_amd/_lib.py).  Revision 2: fasst_source_powers
 * and fasst_sigma_comp take 128-bit column sets (two 64-bit words per
 * spatial component; revision 1 read one word, and fasst_sigma_comp took its
 * mask by value), so a revision-1 caller would pass too short an array.
 * Revision 3 adds the time-invariant spatial filter (fasst_spatial_filter_*)
 * and fasst_gcc_phat.  Revision 4 adds the discrete-state time weights
 * (fasst_set_tw_constr / fasst_get_tw_constr).  Revision 5 adds the two-factor
 * (source / filter) spectral components (fasst_sf_* and fasst_set_factors /
 * fasst_get_factors).  Revision 6 adds fasst_estep_partition.  Revision 7 adds
 * the source / filter IS-NMF (sfnmf_*, fasst_nmf.h).  Revision 8 adds the
 * stereo accompaniment IS-NMF (snmf_*, fasst_simm.h).  Revision 9 adds the
 * GEMM layer's test entry points (fasst_gemm_plan, fasst_gemm_probe,
 * fasst_dgemm2_probe).  Revision 10 adds the sparsity reweighting
 * (fasst_sf_set_sparsity / fasst_sf_reweigh / fasst_sf_run_sparse).  Revision
 * 11 adds the spatial package (fasst_spatial.h). */
#define FASST_ABI_VERSION 11
int fasst_abi_version(void);

/* The E-step's balanced schedule, host arithmetic only (no device call;
 * pyfasst_amd/csrc/fasst_esched.h).  nbt bin tiles x Q quad-steps are the units
 * u = bin_tile Q + q; block b of nb owns [lo[b], lo[b + 1]).  Fills lo[nb + 1],
 * first[nbt] (the first block that meets each bin tile), nseg[nbt] (how many
 * do: the bin tile's partial slots 0 .. nseg - 1) and *max_slots (the slots
 * the context allocates for the E-step partials); a null pointer is skipped.
 * Needs 1 <= nb <= nbt Q < 2^30. */
int fasst_estep_partition(int nbt, int Q, int nb, long long *lo, int *first, int *nseg,
                          int *max_slots);

/* The FP64 MFMA GEMM layer (pyfasst_amd/csrc/fasst_gemm.h, fasst_dgemm2.h),
 * exported so that tests can pin it directly.
 *
 * fasst_gemm_plan: host arithmetic only (no device call).  What gemm<.., NB>
 * does with an M x N x K product: the split-K count *nz it runs when given a
 * workspace, the K range *kchunk of one split, the k_gemm tile shape
 * (*wgm, *wtm, *wtn: a wgm x 4/wgm wave grid of wtm x wtn MFMA tiles) and the
 * workspace *work_doubles it needs (0: no split).  A null pointer is skipped.
 * Needs M, N, K >= 1 and NB in {1, 2, 4}. */
int fasst_gemm_plan(int M, int N, int K, int NB, int *nz, int *kchunk, int *wgm, int *wtm,
                    int *wtn, long long *work_doubles);
/* One gemm<ta, tb, nb> call, C_b = opA opB_b for b < nb, on host operands.
 * A is [M][lda] (ta: [K][lda]); B holds the nb operands back to back, each
 * [K][ldb] (tb: [N][ldb]); C holds the nb outputs back to back, each [M][ldc].
 * Every array is uploaded whole with the given leading dimensions (C too:
 * elements the product does not own come back as they went in) and the call
 * runs on a stream of its own.  use_work bit 0: pass a workspace of
 * fasst_gemm_plan's work_doubles followed by a guard tail (otherwise none is
 * passed and the product runs unsplit); bit 1 (tb == 0 only): B is one
 * [K][ldb] array and operand b is its column block b N .. b N + N - 1.
 * *nz_ran: the split count that ran.  *guard_ok: the guard tails behind the
 * operands, outputs and workspace are bit-intact.  (ta, tb, nb) outside the
 * instantiated forms (0,0,1) (1,0,1) (1,0,2) (1,0,4) (0,1,1) (0,1,2) returns
 * FASST_ERR_UNSUPPORTED; a split product with ldc != N FASST_ERR_SHAPE. */
int fasst_gemm_probe(int device, int ta, int tb, int nb, int M, int N, int K, const double *A,
                     int lda, const double *B, int ldb, double *C, int ldc, int use_work,
                     int *nz_ran, int *guard_ok);
/* One dgemm2 call, C [M][ldc] = A^T B with A [K][lda] and B [K][ldb], in the
 * same way.  a_skew / b_skew in {0, 1} put the device operand one double past
 * a 16-byte boundary (the 4-byte-piece arms with an even leading dimension);
 * A == B with equal lda / ldb and skews runs on one device buffer.  flat = 1
 * keeps the 16-byte form on flat-address pieces.  *arm: 0 D2Prod raw-buffer
 * pieces, 1 D2Prod flat pieces, 2 D2Odd with B in 4-byte pieces, 3 D2Odd with
 * A, 4 D2Odd with both.  A damaged guard tail returns FASST_ERR_DEVICE. */
int fasst_dgemm2_probe(int device, int M, int N, int K, const double *A, int lda, int a_skew,
                       const double *B, int ldb, int b_skew, double *C, int ldc, int flat,
                       int *arm);

const char *fasst_last_error(void);
int fasst_device_count(int *n);

/* ---- model context ------------------------------------------------------
 * Replaces the NumPy state of FASST (audioModel.py:159-248,2349-2393).
 * fasst_create allocates the observation (F freq bins x T frames, stereo:
 * the reference GEM is stereo-only, audioModel.py:394,418-420,605-607);
 * fasst_configure (re)allocates the model: J spatial components (= sources),
 * rank[J] spatial ranks, K[J] NMF components, mix_conv 0 = 'inst' (params
 * C x r), 1 = 'conv' (params r x C x F).  Reconfiguring keeps Cx / X.       */
int fasst_create(int device, int F, int T, fasst_ctx **out);
int fasst_configure(fasst_ctx *ctx, int J, const int *rank, const int *K, int mix_conv);
/* The same with the mixing type per spatial component (mix_conv[J], the
 * reference's per-component 'mix_type', retrieve_subsrc_params
 * audioModel.py:546-576).  In a model with both types, the mixing update
 * (update_mix_matrix :766-889) runs the 'inst' update over the free 'inst'
 * components with every other component held fixed; the reference's 'conv'
 * solve (:854-863) can only run when no other component exists, so its
 * free 'conv' components in a mixed model are rejected by the host layer. */
int fasst_configure_types(fasst_ctx *ctx, int J, const int *rank, const int *K,
                          const int *mix_conv);
int fasst_destroy(fasst_ctx *ctx);

/* comp_transf_Cx (audioModel.py:250-302) on the device: data[L][2] float64
 * (already scaled as AudioObject, audioObject.py:124-127), Hann or any
 * window[wlen], nfft (== fsize), hop.  Keeps the channel STFTs resident for
 * the Wiener images and builds Cx.  T must equal ceil(L/hop)+2.            */
int fasst_set_audio(fasst_ctx *ctx, const double *data, int L, const double *window,
                    int wlen, int nfft, int hop);
/* mix_psd[F] = mean_t over the channel PSDs / 2 (audioModel.py:304-319).   */
int fasst_mix_psd(fasst_ctx *ctx, double *mix_psd);

/* Cx: complex128 [3][F][T], packed upper triangle {X0 X0*, X0 X1*, X1 X1*}
 * exactly as FASST.Cx (audioModel.py:293-302).                              */
int fasst_set_cx(fasst_ctx *ctx, const double *cx);
int fasst_get_cx(fasst_ctx *ctx, double *cx);
/* X: complex128 [2][F][T] channel STFTs kept resident for the Wiener images
 * (replaces the per-source STFT recomputation of audioModel.py:1188-1192);
 * Cx is rebuilt from them on the device (audioModel.py:293-302).           */
int fasst_set_stft(fasst_ctx *ctx, const double *X);

/* Spatial component j: params in the reference layout (complex128; for
 * 'inst' the C x r matrix, for 'conv' r x C x F); free = frdm_prior=='free'.*/
int fasst_set_spatial(fasst_ctx *ctx, int j, const double *params, int free_);
int fasst_get_spatial(fasst_ctx *ctx, int j, double *params);
/* Spectral component of source j (single NMF factor, TB empty):
 * FB F x K, FW K x K, TW K x T (float64).                                    */
int fasst_set_spectral(fasst_ctx *ctx, int j, const double *FB, const double *FW,
                       const double *TW, int fb_free, int tw_free);
int fasst_get_spectral(fasst_ctx *ctx, int j, double *FB, double *FW, double *TW);
/* FW_frdm_prior of source j ('free' = 1): the FW multiplicative update of
 * update_spectral_components (audioModel.py:1578-1631) runs between the FB
 * and TW updates.  Default after fasst_configure: fixed.                     */
int fasst_set_fw_prior(fasst_ctx *ctx, int j, int fw_free);

/* Several spectral components on spatial component j (comp_spat_comp_power's
 * sum over spec_comps, audioModel.py:430-498; sequential per-component
 * update, :1479-1727): source j's FB / FW / TW (set by fasst_set_spectral)
 * hold the nblk components side by side, component b in columns / rows
 * [kb[b], kb[b + 1]) (kb[0] = 0, kb[nblk] = K_j, FW block diagonal), in the
 * reference's spec_comps key order; fb_free[b] / fw_free[b] / tw_free[b] are
 * component b's priors.  Restart flags (fasst_run / fasst_renormalize
 * restart_mask) then count one bit per component: bit (sum of nblk of the
 * sources before j) + b.                                                      */
int fasst_set_blocks(fasst_ctx *ctx, int j, int nblk, const int *kb, const int *fb_free,
                     const int *fw_free, const int *tw_free);

/* lambdaCorr (audioModel.py:1484-1507 and the corrPen terms of :1544-1719):
 * the inter-source correlation penalty of the spectral updates.  With
 * lambda > 0 the components are updated one at a time in the reference's
 * spec_comps key order: component q is block seq_b[q] of spatial component
 * seq_j[q] (fasst_set_blocks layout; nseq = every component, once).
 * lambda = 0 (the default after fasst_configure) switches it off.           */
int fasst_set_corr(fasst_ctx *ctx, double lambda, int nseq, const int *seq_j, const int *seq_b);

/* Time blobs of component b of source j (H = TW.TB, audioModel.py:486-487;
 * set through setComponentParameter(..., 'TB', ...), :2082): TW is the
 * component's factor TW (rows x L, rows = its fasst_set_blocks width), TB the
 * L x T time blobs, tb_free = TB_frdm_prior == 'free'.  The device keeps both
 * and writes H into the component's rows of the source's TW (whatever
 * fasst_set_spectral put there); TW then updates through TB (:1665-1691), TB
 * by :1931-1978, renormalisation :2029-2033.  L = 0 removes them; call after
 * fasst_set_blocks (which drops the time blobs of the source it changes).
 * A restart bit of such a component means sum(TW) < eps: the caller redraws
 * TW and performs the TB renormalisation (fasst_get_tb's TB is then not yet
 * divided by its row means).                                                 */
int fasst_set_tb(fasst_ctx *ctx, int j, int b, int L, const double *TW, const double *TB,
                 int tb_free);
int fasst_get_tb(fasst_ctx *ctx, int j, int b, double *TW, double *TB);

/* Discrete-state time weights of source j's spectral component (TW_constr,
 * update_spectral_components audioModel.py:1728-1928): kind 0 = 'NMF' (the
 * default after fasst_configure), 1 = 'GSMM', 2 = 'SHMM'.  With kind > 0 and
 * a free TW, the TW step of fasst_run / fasst_spectral_update re-estimates,
 * per state k alone, the weight TW_all[k, t], takes the Itakura-Saito
 * divergence of hat_W to that single-state power, decodes one state per frame
 * (GSMM: argmin with the state priors; SHMM: the reference's Viterbi with the
 * transition matrix) and leaves TW = TW_all at the decoded state, 0 elsewhere.
 * TW_all float64 [K][T], or NULL: every row = max_k TW[k, t] of the TW
 * uploaded by fasst_set_spectral (call it first).  dp float64 [K] (GSMM) or
 * [K][K] (SHMM), or NULL: 1 / K.  dp_free = TW_DP_frdm_prior == 'free': dp
 * becomes the decoded state (transition) frequencies after each iteration.
 * The source must have one spectral component without time blobs, the
 * context at most 4096 frequency bins (the step keeps a frame tile of hat_W
 * and a basis column in LDS; FASST_ERR_UNSUPPORTED from this call), and
 * lambdaCorr must be 0 when the iteration runs (FASST_ERR_UNSUPPORTED).
 * fasst_configure, fasst_set_blocks with several components and fasst_set_tb
 * with time blobs on the source drop the constraint.  renormalize_parameters rescales TW, never TW_all.
 * fasst_get_tw_constr: TW_all [K][T], dp [K] or [K][K], state int [T] (the
 * last decoded sequence; zeros before the first TW step); any may be NULL. */
int fasst_set_tw_constr(fasst_ctx *ctx, int j, int kind, const double *TW_all,
                        const double *dp, int dp_free);
int fasst_get_tw_constr(fasst_ctx *ctx, int j, double *TW_all, double *dp, int *state);

/* renormalize_parameters (audioModel.py:1980-2040).  restart_mask bit j (or
 * bit per spectral component, fasst_set_blocks) is set when sum(TW) < eps:
 * the caller draws the restart (host RNG order).                            */
int fasst_renormalize(fasst_ctx *ctx, int *restart_mask);

/* n_iter GEM iterations (GEM_iteration, audioModel.py:384-428), with the
 * annealed noise PSD rows psd[n_iter][F] (audioModel.py:364-373) and the NMF
 * exponent omega (nmfUpdateCoeff).  logliks[n_iter] receives the loglik of
 * each iteration.  On FASST_TW_RESTART, *iters_done iterations are complete
 * (the last one ended in the restart condition reported in restart_mask).   */
int fasst_run(fasst_ctx *ctx, int n_iter, const double *psd, double omega,
              double *logliks, int *restart_mask, int *iters_done);

/* Per-source STFT-domain Wiener images (separate_comps,
 * audioModel.py:1088-1217 up to the iSTFT; compute_sigma_comp_2d :1327,
 * compute_inv_sigma_mix_2d :1374, compute_Wiener_gain_2d :1396).  psd[F] is
 * the last annealed PSD; X complex128 [2][F][T] or NULL to use the resident
 * STFT; S out complex128 [J][2][F][T].                                       */
int fasst_wiener_images(fasst_ctx *ctx, const double *psd, const double *X, double *S);

/* Separation sources for fasst_wiener_images / fasst_separate_waveforms
 * (separate_comps' spec_comp_ind, audioModel.py:1130-1164): source n sums the
 * terms [term_off[n], term_off[n + 1]); term i is the spectral components in
 * columns term_mask[2 i .. 2 i + 1] (a 128-bit column set: bit k of word
 * k / 64 = column k, fasst_set_blocks layout; K <= 128) of spatial
 * component term_j[i] (compute_sigma_comp_2d, :1327-1372).  Sigma_x is the
 * sum over the sources plus the PSD (compute_inv_sigma_mix_2d, :1374-1394).
 * nsrc = 0 (the default): one source per spatial component, all columns.
 * The outputs then hold nsrc sources instead of J.                          */
int fasst_set_sources(fasst_ctx *ctx, int nsrc, const int *term_off, const int *term_j,
                      const unsigned long long *term_mask);

/* separate_comps up to the waveforms it writes (audioModel.py:1088-1233):
 * the Wiener images above, then the per-source, per-channel iSTFT
 * (tftransforms/stft.py:71-131, window / analysis_window as STFT's
 * synthWindow / window) of each image without leaving device memory.  Needs
 * the resident STFT (fasst_set_audio / fasst_set_stft) and nfft/2+1 == F.
 * y out float64 [J][2][len], len = hop*(T-1) + wlen - wlen/2 (istft's length
 * before the caller's [:datalen] trim).                                      */
int fasst_separate_waveforms(fasst_ctx *ctx, const double *psd, const double *window,
                             const double *analysis_window, int wlen, int nfft, int hop,
                             double *y);

/* Time-invariant spatial filter (separate_spatial_filter_comp,
 * audioModel.py:891-1061): per bin R_n = sum_r a_r a_r^H of every 'conv'
 * spatial component, R_aa their mean over n, WG_n = R_n inv(R_aa)
 * (inv_herm_mat_2d with its determinant clamp, tools/signalTools.py:182-196;
 * compute_Wiener_gain_2d timeInvariant, audioModel.py:1453-1465) divided by
 * Re(WG_n[0,0] + WG_n[1,1]).  The spectral parameters and the noise PSD play
 * no part, and neither does fasst_set_sources: there is one output per spatial
 * component.  All three need a configured context whose components are all
 * 'conv' (the reference raises NotImplementedError('Mixing params not
 * convolutive...') on an 'inst' one): otherwise FASST_ERR_UNSUPPORTED.
 *   gains      WG out complex128 [J][2][2][F]
 *   images     S out complex128 [J][2][F][T], S[n][c] = sum_c2 WG_n[c][c2] X[c2]
 *              of the resident STFT (any transform's: fasst_set_stft)
 *   waveforms  the iSTFT of each image, the gain applied as each frame is
 *              loaded (the images are never stored); arguments, y layout
 *              [J][2][len] and len as fasst_separate_waveforms              */
int fasst_spatial_filter_gains(fasst_ctx *ctx, double *WG);
int fasst_spatial_filter_images(fasst_ctx *ctx, double *S);
int fasst_spatial_filter_waveforms(fasst_ctx *ctx, const double *window,
                                   const double *analysis_window, int wlen, int nfft, int hop,
                                   double *y);

/* gcc_phat_tdoa_2d (audioModel.py:1316-1324): out float64 [nfft][T] =
 * irfft(Cx01 / |Cx01|, n = nfft, axis = 0) of the context's observation
 * (fasst_set_audio / fasst_set_stft / fasst_set_cx); needs nfft/2+1 == F.  A
 * bin whose cross-spectrum is zero is 0/0 = NaN, as in the reference.        */
int fasst_gcc_phat(fasst_ctx *ctx, int nfft, double *out);

/* ---- two-factor (source / filter) spectral components --------------------
 * A model whose spectral components have one or two factors, V_j = prod_i
 * (FB_i.FW_i).TW_i (comp_spat_comp_power, audioModel.py:430-498; the reference's
 * multiChanSourceF0Filter, :2551-2900), runs on a state of its own beside the
 * single-factor model above (fasst_sf.hip): the powers are held as F x T
 * planes on the device and no F x T array crosses to the host during
 * fasst_sf_run.  Every spatial component has exactly one spectral component;
 * every factor is TW_constr 'NMF' without time blobs; lambdaCorr is 0.
 *
 * fasst_sf_configure replaces any model of the context (fasst_configure* drops
 * it again): J spatial components, rank[J] (sum <= 16, the explicit-V E-step),
 * mix_conv[J] (0 'inst', 1 'conv'), nfac[J] in {1, 2}, and per (j, i) at index
 * 2 j + i: Kb, Kw (FB F x Kb, FW Kb x Kw -- not square in general -- TW Kw x T)
 * and priors[3 (2 j + i) + {0, 1, 2}] = FB / FW / TW 'free';
 * alias[3 (2 j + i) + {0, 1, 2}] = -1, or the index 2 j' + i' of an earlier
 * factor whose FB / FW / TW this factor shares (the reference's source
 * dictionary is one array in every component and is rescaled in place by
 * each of them, audioModel.py:2679-2680,2003-2021): one device buffer.
 * fasst_sf_set_spatial / fasst_sf_get_spatial: params as fasst_set_spatial.
 * fasst_set_factors / fasst_get_factors: the three matrices of factor i of
 * component j, row-major float64, caller-owned (get: any may be NULL).
 * fasst_sf_renormalize / fasst_sf_run: as fasst_renormalize / fasst_run; bit
 * 2 j + i of restart_mask is factor i of component j: the caller redraws TW,
 * and for a factor that is not the last divides it by its mean and performs
 * the whole renormalisation of the next factor with that mean as its energy
 * (the device left that factor alone; audioModel.py:2003-2036 hands
 * `global_energy` from factor to factor).
 * fasst_sf_wiener_images / fasst_sf_separate_waveforms: as fasst_wiener_images
 * (resident STFT only) / fasst_separate_waveforms with the sources given here:
 * source n sums the spatial components j with src_of[j] == n (-1: in none);
 * S out complex128 [nsrc][2][F][T], y out float64 [nsrc][2][len].
 *
 * Sparsity reweighting (reweigh_sparsity_constraint, audioModel.py:2981-3014).
 * fasst_sf_set_sparsity: length[J], the median filter length of component j's
 * barycentre track (0: the component is not reweighed); cleared by
 * fasst_sf_configure.  fasst_sf_reweigh(sigma > 0): for j = 0 .. J-1 in order,
 * where length[j] > 0 and factor 0 has Kw > 2, TW of factor 0 (the buffer in
 * use: one shared by two components is multiplied twice) is multiplied in
 * place by the Gaussian mask of width sigma around the median-filtered
 * barycentre of its columns (k_sf_bary, then k_sf_sparsify).
 * fasst_sf_run_sparse: fasst_sf_run with fasst_sf_reweigh(sigma[it]) after
 * every iteration it whose flags are clean.  An iteration that flags a dead TW
 * returns FASST_TW_RESTART with *iters_done = it + 1 WITHOUT that iteration's
 * reweigh: the reference redraws TW inside GEM_iteration (:2023-2028), before
 * the reweigh of the same loop pass (:2966-2977), so the caller redraws,
 * uploads, calls fasst_sf_reweigh(sigma[it]) and resumes at it + 1.          */
int fasst_sf_configure(fasst_ctx *ctx, int J, const int *rank, const int *mix_conv, const int *nfac,
                       const int *Kb, const int *Kw, const int *priors, const int *alias);
int fasst_sf_set_spatial(fasst_ctx *ctx, int j, const double *params, int free_);
int fasst_sf_get_spatial(fasst_ctx *ctx, int j, double *params);
int fasst_set_factors(fasst_ctx *ctx, int j, int i, const double *FB, const double *FW,
                      const double *TW);
int fasst_get_factors(fasst_ctx *ctx, int j, int i, double *FB, double *FW, double *TW);
int fasst_sf_renormalize(fasst_ctx *ctx, int *restart_mask);
int fasst_sf_run(fasst_ctx *ctx, int n_iter, const double *psd, double omega, double *logliks,
                 int *restart_mask, int *iters_done);
int fasst_sf_set_sparsity(fasst_ctx *ctx, const int *length);
int fasst_sf_reweigh(fasst_ctx *ctx, double sigma);
int fasst_sf_run_sparse(fasst_ctx *ctx, int n_iter, const double *psd, double omega,
                        const double *sigma, double *logliks, int *restart_mask, int *iters_done);
int fasst_sf_wiener_images(fasst_ctx *ctx, const double *psd, int nsrc, const int *src_of, double *S);
int fasst_sf_separate_waveforms(fasst_ctx *ctx, const double *psd, int nsrc, const int *src_of,
                                const double *window, const double *analysis_window, int wlen,
                                int nfft, int hop, double *y);

/* Per-kernel timing with HIP events (used by bench.py for the roofline of
 * the dominant kernel), in the timed loop's own schedule: each pair is
 * recorded on the stream its kernel runs on (the side stream stays forked),
 * in a ring of 32 iterations between host syncs.  fasst_kernel_times
 * returns the number of kernel slots and fills the mean duration in ms of
 * each slot over the profiled iterations (a side-stream slot measures its
 * kernel while the main stream's kernels run beside it).                   */
int fasst_set_profiling(fasst_ctx *ctx, int on);
int fasst_kernel_times(fasst_ctx *ctx, double *avg_ms, long *counts, int nk);
const char *fasst_kernel_name(int i);

/* ---- stateless kernels --------------------------------------------------
 * stft (tftransforms/stft.py:3-69): x[L] float64, window[wlen], nfft a power
 * of two >= wlen, hop; X out complex128 [nfft/2+1][n_frames] with
 * n_frames = ceil(L/hop)+2 (query with X == NULL).                           */
int fasst_stft(int device, const double *x, int L, const double *window, int wlen,
               int nfft, int hop, double *X, int *n_frames);
/* istft (tftransforms/stft.py:71-131): X complex128 [nfft/2+1][n_frames];
 * y out float64 [hop*(n_frames-1)+wlen - wlen/2].                           */
int fasst_istft(int device, const double *X, int n_frames, const double *window,
                const double *analysis_window, int wlen, int nfft, int hop, double *y);
/* istft of the SIMM pipeline (SeparateLeadStereo/separateLeadFunctions.py:
 * 163-233): no half-window trim, edge normalisation copied from the
 * neighbouring window; y out float64 [hop*(n_frames-1)+wlen] (>= 2 wlen). */
int fasst_istft_simm(int device, const double *X, int n_frames, const double *window,
                     const double *analysis_window, int wlen, int nfft, int hop, double *y);
/* inv_herm_mat_2d (tools/signalTools.py:132-196) on n matrices:
 * diag[2][n], off complex128[n] -> inv_diag[2][n], inv_off complex128[n], det[n]. */
int fasst_inv_herm_mat_2d(int device, int n, const double *diag, const double *off,
                          double *inv_diag, double *inv_off, double *det);

/* ---- GEM step methods (fasst_steps.hip) ---------------------------------
 * The FASST methods GEM_iteration (audioModel.py:384-428) is made of, as
 * device calls on the reference's own arrays, for scripts that drive an
 * iteration piecewise or inspect its intermediates (fasst_run fuses them and
 * never materialises these arrays).  complex128 = interleaved (re, im).
 *
 * retrieve_subsrc_params (:514-578), the powers half: V out [nj][F][T], the
 * power of spatial components j0 .. j0+nj-1 from the context's parameters
 * (colmask[2 jj .. 2 jj + 1]: the NMF columns to include, a 128-bit set,
 * bit k of word k / 64 = column k; NULL: all).                             */
int fasst_source_powers(fasst_ctx *ctx, int j0, int nj, const unsigned long long *colmask,
                        double *V);
/* compute_suff_stat (:580-764) on the context's Cx: V [R][F][T] per-rank
 * powers, mix complex128 [R][2][F], psd [F] -> rxx complex128 [3][F]
 * (hat_Rxx: mean of Cx00, Cx01, Cx11), rxs complex128 [F][2][R],
 * rss complex128 [F][R][R], ws [R][F][T] (hat_Ws), loglik.  R <= 16.      */
int fasst_suff_stat(fasst_ctx *ctx, int R, const double *V, const double *mix, const double *psd,
                    double *rxx, double *rxs, double *rss, double *ws, double *loglik);
/* update_mix_matrix (:766-889), the solve: kind[r] = 0 fixed, 1 free
 * 'inst', 2 free 'conv' per rank; mix complex128 [R][2][F] in/out.  Free
 * 'conv' ranks next to other ranks: FASST_ERR_SHAPE (the reference's solve
 * raises); a singular system: FASST_ERR_SINGULAR, mix untouched.           */
int fasst_mix_solve(int device, int F, int R, const double *rss, const double *rxs, double *mix,
                    const int *kind);
/* update_spectral_components (:1469-1978): hat_W [J][F][T] -> the
 * context's FB / FW / TW (TB) updated in place (read back with
 * fasst_get_spectral); no renormalisation (fasst_renormalize).            */
int fasst_spectral_update(fasst_ctx *ctx, const double *hat_W, double omega);
/* compute_sigma_comp_2d (:1327-1372): spatial component j, NMF columns
 * colmask[0 .. 1] (128-bit set, bit k of word k / 64 = column k) ->
 * diag [2][F][T], off complex128 [F][T].                                   */
int fasst_sigma_comp(fasst_ctx *ctx, int j, const unsigned long long *colmask, double *diag,
                     double *off);
/* compute_inv_sigma_mix_2d (:1374-1394): n components' diag [n][2][F][T],
 * off complex128 [n][F][T], psd [F] -> inverse of their sum + PSD I:
 * idiag [2][F][T], ioff complex128 [F][T].                                 */
int fasst_inv_sigma_mix(int device, int n, int F, int T, const double *diag, const double *off,
                        const double *psd, double *idiag, double *ioff);
/* compute_Wiener_gain_2d (:1396-1467): one component's sigma (sdiag
 * [2][n], soff complex128 [n]) and the inverse mixture covariance
 * (idiag [2][n], ioff complex128 [n]) -> WG complex128 [2][2][n].         */
int fasst_wiener_gain(int device, long n, const double *sdiag, const double *soff,
                      const double *idiag, const double *ioff, double *WG);

#ifdef __cplusplus
}
#endif
#endif /* FASST_HIP_H */
