// Internal interface of the EM engine's translation units: fasst_em.hip (model
// configuration, gem_iteration, the phases not yet moved out, the C ABI) and
// fasst_em_estep.hip (the E-step).  Each kernel is named in exactly one unit,
// which launches it and queries or sets its attributes; the other reaches it
// through the host functions declared here.  Argument structs stay private to
// their unit.
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

// ---- fasst_em_estep.hip
int estep_lds_limits();                    // the dynamic-LDS ceilings of k_egen_stats / _fused
int estep_occupancy(const fasst_ctx *c);   // resident E-step blocks per CU
bool estep_cxi(const fasst_ctx *c);        // the single-pass E-step reads the Cx image
bool estep_twi(const fasst_ctx *c);        // ... and the TW image
// the model's E-step on c->stream; tw_fresh: the previous iteration's fused
// k_tw_update wrote the TW image
int launch_estep_phase(fasst_ctx *c, const double *psd_dev, bool tw_fresh);
int launch_loglik(fasst_ctx *c, double *ll_dev);   // k_loglik over the E-step's partials

}  // namespace fasst
