// The k_estep_mx<2, ...> instantiations: the single-pass E-step of a model of
// 2 sources, with its launch and occupancy query (fasst_em_estep_mx.h).
#include "fasst_em_estep_mx.h"

template int fasst::estep_mx_j<2>(const fasst_ctx *, const fasst::EArgs *, int);
