// The TW contraction's balanced schedule (k_tw_contract_lds): integer
// partition of the flattened (source, frame group, bin step) work list over NB
// persistent blocks, on fasst_esched.h's formulas.  Used by the host (launch
// shape, buffer size), by the kernel (its range and partial slots) and by
// k_tw_update (slots per unit), so the layout of tnum / tden is decided here
// and nowhere else.
//
// A frame group is the NW x TPW frame tiles one block works on together; with
// G groups, J sources and nft bin steps the units are u = j G + g and the
// steps s = u nft + f, U = J G nft of them.  Block b owns [b U / NB,
// (b + 1) U / NB).  The part of a block's range inside one unit is a segment;
// a unit's segments are numbered from 0 (the slot) in block order, and a
// partial lives at [slot][j][t][k].  1 <= NB <= U: no block is empty and a
// unit's slots are dense.  A unit whose source has no free TW keeps its
// steps (the list does not depend on the step's free flags); its segments are
// skipped by the whole block.
//
// Plain C++ (no HIP types): tools/twsched_check.cpp compiles it on the host.
#pragma once

#include "fasst_esched.h"

namespace fasst {

// how the TW partials are laid out (a value argument of the kernels that
// write or sum them).  bal == 0: the static bin split, every (source, frame)
// has nslot = bin chunks partials.
struct TwSched {
  int bal;    // 1: balanced schedule
  int nb;     // balanced: blocks
  int G;      // balanced: frame groups per source
  int gf;     // balanced: frames per group (16 NW TPW)
  int nft;    // balanced: bin steps per unit
  int nu;     // balanced: units (J G)
  int nslot;  // slots of tnum / tden (max segments per unit)
};

FASST_ES_HD long long tws_steps(const TwSched &s) { return (long long)s.nu * s.nft; }
// the unit of (source j, frame t)
FASST_ES_HD int tws_unit(const TwSched &s, int j, int t) { return j * s.G + t / s.gf; }
// first block that meets unit u, and how many do
FASST_ES_HD int tws_first(const TwSched &s, int u) { return es_first(u, s.nft, s.nu, s.nb); }
FASST_ES_HD int tws_nseg(const TwSched &s, int u) { return es_nseg(u, s.nft, s.nu, s.nb); }
// partials of (source j, frame t) under either layout
FASST_ES_HD int tws_segments(const TwSched &s, int j, int t) {
  return s.bal ? tws_nseg(s, tws_unit(s, j, t)) : s.nslot;
}

// One segment of a block's walk.
struct TwSeg {
  int u, f0, nf, slot;   // unit, first bin step, bin steps, partial slot
};
// the segment of block b that starts at step s (lo(b) <= s < end = lo(b + 1)),
// up to the unit's or the range's end
FASST_ES_HD TwSeg tws_segment(const TwSched &sc, int b, long long s, long long end) {
  TwSeg g;
  g.u = (int)(s / sc.nft);
  g.f0 = (int)(s - (long long)g.u * sc.nft);
  const long long left = end - s;
  g.nf = left < sc.nft - g.f0 ? (int)left : sc.nft - g.f0;
  g.slot = b - tws_first(sc, g.u);   // (0 where the block starts the unit)
  return g;
}

// the balanced schedule of J sources x G groups of gf frames x nft bin steps
// on nb blocks (clamped to [1, U])
inline TwSched tws_make(int J, int G, int gf, int nft, long long nb) {
  TwSched s{};
  s.bal = 1;
  s.G = G;
  s.gf = gf;
  s.nft = nft;
  s.nu = J * G;
  const long long U = tws_steps(s);
  s.nb = (int)(nb < 1 ? 1 : nb > U ? U : nb);
  s.nslot = es_max_slots(s.nu, s.nft, s.nb);
  return s;
}

}  // namespace fasst
