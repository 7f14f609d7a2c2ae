// The k_estep_mx<8, ...> instantiations: the single-pass E-step of a model of
// 8 sources, with its launch and occupancy query (fasst_em_estep_mx.h).
#include "fasst_em_estep_mx.h"

template int fasst::estep_mx_j<8>(const fasst_ctx *, const fasst::EArgs *, int);
