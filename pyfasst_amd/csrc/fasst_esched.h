// The E-step's balanced schedule: integer partition of the flattened
// (bin tile, quad-step) work list over NB blocks.  One formula, used by the
// host (launch shape, buffer size), by k_estep_mx (its own range and partial
// slot) and by the consumers of the partials (segments per bin tile), so the
// layout of epart / llpart is decided here and nowhere else.
//
// A quad-step is one 16-bin tile x 4 consecutive frame tiles (one per wave).
// With Q quad-steps per bin tile the units are u = bin_tile * Q + q, U = nbt * Q
// of them, and block b owns [b U / NB, (b + 1) U / NB) (floor division).  The
// part of a block's range inside one bin tile is a segment; the segments of a
// bin tile are numbered from 0 (its slot) in block order, and a partial lives
// at [slot][bin] (statistics) or [slot][bin tile] (loglik).  1 <= NB <= U, so
// no block is empty and the blocks first(bt) .. first(bt) + nseg(bt) - 1 all
// meet bin tile bt: the slots are dense.
//
// Plain C++ (no HIP types): tools/esched_check.cpp compiles it on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FASST_ES_HD __host__ __device__ __forceinline__
#else
#define FASST_ES_HD inline
#endif

namespace fasst {

// how the E-step partials are laid out (a value argument of the kernels that
// write or sum them).  bal == 0: the (bin tile, frame chunk) grid, every bin
// tile has nslot = frame chunks segments.
struct ESched {
  int bal;    // 1: balanced schedule
  int nb;     // balanced: blocks
  int Q;      // balanced: quad-steps per bin tile
  int nbt;    // bin tiles
  int nslot;  // slots of the partial buffers (max segments per bin tile)
};

// first unit of block b
FASST_ES_HD long long es_lo(int b, long long U, int nb) { return (long long)b * U / nb; }
// the block that owns unit u: the largest b with b U / NB <= u
FASST_ES_HD int es_owner(long long u, long long U, int nb) {
  return (int)(((u + 1) * nb - 1) / U);
}
// first block that meets bin tile bt, and how many do
FASST_ES_HD int es_first(int bt, int Q, int nbt, int nb) {
  return es_owner((long long)bt * Q, (long long)nbt * Q, nb);
}
FASST_ES_HD int es_nseg(int bt, int Q, int nbt, int nb) {
  const long long U = (long long)nbt * Q;
  return es_owner((long long)bt * Q + Q - 1, U, nb) - es_owner((long long)bt * Q, U, nb) + 1;
}
// segments of bin tile bt under either schedule
FASST_ES_HD int es_segments(const ESched &s, int bt) {
  return s.bal ? es_nseg(bt, s.Q, s.nbt, s.nb) : s.nslot;
}

// max over the bin tiles of nseg: sizes the partial buffers
inline int es_max_slots(int nbt, int Q, int nb) {
  int m = 1;
  for (int bt = 0; bt < nbt; ++bt) {
    const int n = es_nseg(bt, Q, nbt, nb);
    if (n > m) m = n;
  }
  return m;
}

}  // namespace fasst
