// The k_estep_mx<1, ...> instantiations: the single-pass E-step of a model of
// 1 source, with its launch and occupancy query (fasst_em_estep_mx.h).
#include "fasst_em_estep_mx.h"

template int fasst::estep_mx_j<1>(const fasst_ctx *, const fasst::EArgs *, int);
