// Host check of the TW contraction's balanced partition
// (pyfasst_amd/csrc/fasst_twsched.h), stand-alone so it can run under the host
// sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/twsched_check.cpp -o twsched_check
//   ./twsched_check            (the sweep)
//   ./twsched_check J G nft NB (one schedule; prints "nb nslot")
// For J sources x G frame groups x nft bin steps on NB blocks it walks every
// block's range the way k_tw_contract_lds<BAL> does (tws_segment after
// tws_segment) and checks that every step is owned exactly once, that no block
// is empty, that a unit's slots are dense from 0 in block order, that nslot is
// the largest count found, that k_tw_update's count (tws_segments of any frame
// of the unit) is the unit's, and that the owner formula inverts the range
// formula.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pyfasst_amd/csrc/fasst_twsched.h"

using namespace fasst;

static int check(int J, int G, int nft, long long nb_asked, TwSched *out = nullptr) {
  const int gf = 128;
  const TwSched sc = tws_make(J, G, gf, nft, nb_asked);
  if (out) *out = sc;
  const long long U = tws_steps(sc);
  if (U != (long long)J * G * nft) return 1;
  if (sc.nb != (int)std::max(1ll, std::min(nb_asked, U))) return 2;   // clamped to [1, U]
  std::vector<int> owned(U, 0);
  std::vector<std::vector<int>> slots(sc.nu);
  for (int b = 0; b < sc.nb; ++b) {
    const long long lo = es_lo(b, U, sc.nb), end = es_lo(b + 1, U, sc.nb);
    if (end <= lo) return 3;                                  // no empty block
    // the owner formula inverts the range formula at both ends of the range
    if (es_owner(lo, U, sc.nb) != b || es_owner(end - 1, U, sc.nb) != b) return 4;
    for (long long s = lo; s < end;) {
      const TwSeg g = tws_segment(sc, b, s, end);
      if (g.nf < 1 || g.u < 0 || g.u >= sc.nu || g.f0 < 0 || g.f0 + g.nf > nft) return 5;
      if ((long long)g.u * nft + g.f0 != s) return 6;
      if (g.slot < 0 || g.slot >= sc.nslot) return 7;         // inside the buffers
      for (int f = g.f0; f < g.f0 + g.nf; ++f) ++owned[(size_t)g.u * nft + f];
      slots[g.u].push_back(g.slot);
      s += g.nf;
    }
  }
  for (long long s = 0; s < U; ++s)
    if (owned[s] != 1) return 8;
  int mx = 1;
  for (int u = 0; u < sc.nu; ++u) {
    const int n = tws_nseg(sc, u), j = u / G, g = u % G;
    if ((int)slots[u].size() != n) return 9;
    for (int i = 0; i < n; ++i)
      if (slots[u][i] != i) return 10;                        // dense, in block order
    // every 64-frame block of the group sees the unit's count
    for (int t = g * gf; t < (g + 1) * gf; t += 64)
      if (tws_unit(sc, j, t) != u || tws_segments(sc, j, t) != n) return 11;
    mx = std::max(mx, n);
  }
  return sc.nslot == mx ? 0 : 12;
}

int main(int argc, char **argv) {
  if (argc == 5) {
    TwSched sc;
    const int e = check(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoll(argv[4]), &sc);
    if (e) {
      std::printf("FAIL %d\n", e);
      return 1;
    }
    std::printf("%d %d\n", sc.nb, sc.nslot);
    return 0;
  }
  long n = 0;
  for (int J = 1; J <= 4; ++J)
    for (int G = 1; G <= 9; ++G)
      for (int nft = 1; nft <= 9; ++nft)
        for (int nb = 1; nb <= J * G * nft; ++nb, ++n)
          if (int e = check(J, G, nft, nb)) {
            std::printf("FAIL %d: J=%d G=%d nft=%d nb=%d\n", e, J, G, nft, nb);
            return 1;
          }
  // the benchmark's shape and its neighbours, the clamps, a large list
  const long long big[][4] = {{4, 79, 129, 512},  {4, 79, 129, 511}, {4, 79, 129, 1024},
                              {4, 79, 129, 683},  {4, 79, 129, 256}, {4, 79, 129, 1},
                              {4, 79, 129, 40764}, {4, 79, 129, 0},  {4, 79, 129, 1 << 20},
                              {8, 313, 257, 2048}, {3, 2, 5, 7}};
  for (const auto &c : big) {
    ++n;
    if (int e = check((int)c[0], (int)c[1], (int)c[2], c[3])) {
      std::printf("FAIL %d: J=%lld G=%lld nft=%lld nb=%lld\n", e, c[0], c[1], c[2], c[3]);
      return 1;
    }
  }
  std::printf("twsched_check: %ld schedules ok\n", n);
  return 0;
}
