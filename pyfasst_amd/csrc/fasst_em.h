// Internal interface of the EM engine's translation units: fasst_em.hip
// (model configuration, gem_iteration, the C ABI; no kernel) and one unit per
// phase, fasst_em_estep.hip, fasst_em_mix.hip, fasst_em_spectral.hip and
// fasst_em_renorm.hip.  The E-step's single-pass kernel is instantiated in
// eight further units, fasst_em_estep_j1.hip .. _j8.hip, one per source count,
// which only fasst_em_estep.hip calls (fasst_em_estep_mx.h).  Each kernel, and
// each of its instantiations, is named in exactly one unit, which launches it
// and queries or sets its attributes; the others reach it through the host
// functions declared here.  Argument structs stay private to their unit (the
// E-step's to its units).
#pragma once
#include "fasst_ctx.h"

namespace fasst {

enum KernelId {
  KW = 0, KFWH, KINSTA, KESTEP, KLL, KMIX, KMIXI, KFBC, KFBU, KTWC, KREN, KTWU, KFWU, KROWS, KRTAIL, KTWD, KTWV
};

// per-kernel timing: an event pair around the launch on the stream it runs on
// (s = nullptr: the main stream), slot = the iteration's place in the ring
inline void prof_begin(fasst_ctx *c, int id, hipStream_t s = nullptr) {
  if (c->prof) {
    (void)hipEventRecord(c->ev0[id][c->pslot], s ? s : c->stream);
    c->used[id][c->pslot] = 1;
  }
}
inline void prof_end(fasst_ctx *c, int id, hipStream_t s = nullptr) {
  if (c->prof) (void)hipEventRecord(c->ev1[id][c->pslot], s ? s : c->stream);
}

// the E-step's default schedule and the fewest quad-steps a balanced block
// takes by default (fasst_configure)
constexpr bool kEsBalancedDefault = true;
constexpr int kEsMinUnits = 10;
// k_tw_contract_lds's schedule when FASST_TWC_SCHED is unset
constexpr bool kTwcBalancedDefault = true;

// bins per block of the FW update's f-contraction (k_fw_reduce holds three
// [fpc][KP] tiles in LDS: 96 KB at KP = 128 with 32 bins)
inline int fw_fpc(const fasst_ctx *c) { return c->KP > 64 ? 32 : kFwFpc; }

// ---- fasst_em_estep.hip
int estep_lds_limits();                    // the dynamic-LDS ceilings of k_egen_stats / _fused
int estep_occupancy(const fasst_ctx *c);   // resident E-step blocks per CU
bool estep_cxi(const fasst_ctx *c);        // the single-pass E-step reads the Cx image
bool estep_twi(const fasst_ctx *c);        // ... and the TW image
// the model's E-step on c->stream; tw_fresh: the previous iteration's fused
// k_tw_update wrote the TW image
int launch_estep_phase(fasst_ctx *c, const double *psd_dev, bool tw_fresh);
int launch_loglik(fasst_ctx *c, double *ll_dev);   // k_loglik over the E-step's partials

// ---- fasst_em_mix.hip (build_inst_A: fasst_ctx.h)
int mix_lds_limits();                        // the dynamic-LDS ceiling of k_mix's R > 16 arm
int launch_mix(fasst_ctx *c, hipStream_t s);   // update_mix_matrix on stream s

// ---- fasst_em_renorm.hip
int launch_renorm(fasst_ctx *c, int iter);   // the unfused renormalisation on c->stream
// the fused tail's k_renorm_scales (then ev_scales) and k_renorm_rows on the
// side stream, inside launch_tail_side's fork
int launch_renorm_side(fasst_ctx *c, hipStream_t side);
// the fused tail's last launch, k_renorm_tail, after the side stream's ev_rows
int launch_renorm_tail(fasst_ctx *c, double *ll_dev, int iter, bool prep);

// ---- fasst_em_spectral.hip (launch_w_old: fasst_ctx.h)
int spectral_lds_limits();   // the dynamic-LDS ceilings of k_fw_reduce / k_fwh_t
// resident k_tw_contract_lds blocks per CU (bal: of its balanced form; sets its
// LDS ceiling), its frame-tile groups (units) and the frame tiles of one
int twl_occupancy(const fasst_ctx *c, bool bal, int *units, int *group_tiles);
int contract_occupancy(const fasst_ctx *c);   // resident k_fb_contract waves per CU
int launch_spectral_prep(fasst_ctx *c, bool fork);   // (FW.TW)^T and the TW row sums
int spectral_update(fasst_ctx *c, double omega, bool tail = false);
int launch_tb_refresh(fasst_ctx *c, int iter);   // launch_renorm: H = TWs TB of every time blob
int launch_tb_set(fasst_ctx *c, int j, int b);   // fasst_set_tb: H of block b of source j
// fasst_spectral_update: k_rho_from_hatw from a caller's hat_W [J][F][T] on the device
int launch_rho_from_hatw(fasst_ctx *c, const double *hat_W_dev);

}  // namespace fasst
