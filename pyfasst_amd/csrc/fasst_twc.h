// Launchers of the discrete-state TW step (fasst_twc.hip), called by the
// spectral update of fasst_em_spectral.hip for the sources fasst_set_tw_constr marked:
// c->Wkf = W of the pre-update factors, c->Wkf_new = W after the FB / FW
// updates, c->TW still the previous time weights, c->hatW the E-step's rho
// = hat_W / max(V_old, eps), or (plane_is_hatw, the multi-component path after
// its first k_multi_prep) hat_W itself.
#pragma once
#include "fasst_ctx.h"

namespace fasst {
int launch_tw_statediv(fasst_ctx *c, double omega, bool plane_is_hatw);
int launch_tw_decode(fasst_ctx *c);
}  // namespace fasst
