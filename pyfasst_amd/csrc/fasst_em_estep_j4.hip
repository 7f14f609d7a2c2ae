// The k_estep_mx<4, ...> instantiations: the single-pass E-step of a model of
// 4 sources, with its launch and occupancy query (fasst_em_estep_mx.h).
#include "fasst_em_estep_mx.h"

template int fasst::estep_mx_j<4>(const fasst_ctx *, const fasst::EArgs *, int);
