// Two-factor (source / filter) spectral components: the "planar" GEM path of
// fasst_sf.hip.  A model of this kind keeps its own device state beside the
// single-factor state of fasst_ctx.h, which it never touches: every spatial
// component has one spectral component of one or two factors, each factor
// FB [F][Kb], FW [Kb][Kw], TW [Kw][T] (dense row-major, FW not square), and the
// powers are held as F x T planes.
#pragma once
#include "fasst_ctx.h"

namespace fasst {

constexpr int kSfMaxFac = 2;
constexpr int kSfWideK = 128;     // Kb above this: a wide candidate
constexpr int kSfWideRows = 64;   // FB rows per column-max partial
constexpr int kSfWidePart = 1024; // blocks (= partial sums) of the TW reduction

struct SfFactor {
  int Kb = 0, Kw = 0, fb_free = 0, fw_free = 0, tw_free = 0;
  DBuf<double> FB, FW, TW, W, P;   // W = FB.FW [F][Kw], P = W.TW [F][T]
  // the matrices in use: this factor's own buffers, or those of an earlier
  // factor it shares a matrix with (fasst_sf_configure's alias)
  double *fb = nullptr, *fw = nullptr, *tw = nullptr;
  // the wide arm (fasst_sf.hip, "wide factors"): cand = Kb > kSfWideK with FB
  // and FW fixed and FW square (fasst_sf_configure); wide = cand and the FW
  // last uploaded is diagonal (fasst_set_factors).  A wide factor holds
  // W = FB.diag(FW) [F][ldw] and its transpose WT [Kb][ldwt], both leading
  // dimensions even (the 16-byte row loads of k_dgemm2)
  int cand = 0, wide = 0, ldw = 0, ldwt = 0;
  DBuf<double> WT;
};

}  // namespace fasst

struct fasst_sf_model {
  int J = 0, R = 0;
  int rank[fasst::kMaxJ] = {0}, roff[fasst::kMaxJ + 1] = {0}, conv[fasst::kMaxJ] = {0};
  int spat_free[fasst::kMaxJ] = {0}, nfac[fasst::kMaxJ] = {0};
  int shared[fasst::kMaxJ] = {0};   // source j has a matrix in common with another factor
  fasst::SfFactor fac[fasst::kMaxJ][fasst::kSfMaxFac];
  // planes: V [J][F][T] source powers, ws [R][F][T] hat_Ws, hatW [J][F][T],
  // other / rn / rd [F][T] of the factor being updated
  fasst::DBuf<double> V, ws, hatW, other, rn, rd;
  fasst::DBuf<double2> mix, rss, rxs, rxx;   // mix [R][2][F] (canonical mixing parameters)
  fasst::DBuf<double> psd, llb, ll, energy, scal;
  // energy [j] the spatial energies, [kMaxJ + j] mean(TW) handed to the next factor
  fasst::DBuf<int> droff, dconv;             // roff / conv on the device
  fasst::DBuf<int> kind, flags;              // flags [0] singular, [1 + 2 j + i] TW restart
  // contraction outputs and the split-K workspace of the MFMA GEMM
  fasst::DBuf<double> cn, cd, xn, xd, fwh, work;
  int psd_cap = 0;
  // sparsity reweighting (fasst_sf_set_sparsity): the median length of
  // component j's barycentre track (0: none) and the track itself, mu [T]
  int sparsity[fasst::kMaxJ] = {0};
  fasst::DBuf<double> mu;
  // wide factors only: rnd [F][2 T] = [rn | rd], cnd [Kb][2 T] = [num | den],
  // wcmax [ceil(F / kSfWideRows)][Kb] column-max partials, wm / ww2 [Kb] the
  // column maxima of FB and the column means of FW, wpart the block sums of TW
  fasst::DBuf<double> rnd, cnd, wcmax, wm, ww2, wpart;
};

namespace fasst {
void sf_release(fasst_ctx *c);
// device-pointer forms of compute_suff_stat and update_mix_matrix's solve
// (fasst_steps.hip): every array already on the device, launched on `s`.
// vmap[r] = the plane of V that rank r reads (V holds one plane per source)
int suff_stat_device(fasst_ctx *c, hipStream_t s, int R, const double *dV, const int *vmap,
                     const double2 *dmix, const double *dpsd, double2 *drxx, double2 *drxs,
                     double2 *drss, double *dws, double *dllb, double *dll);
int mix_solve_device(hipStream_t s, int F, int R, const double2 *drss, const double2 *drxs,
                     double2 *dmix, const int *dkind, int nconv, int *dsing);
}  // namespace fasst
