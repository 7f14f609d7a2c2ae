// Host check of the E-step's balanced partition (pyfasst_amd/csrc/fasst_esched.h),
// stand-alone so it can run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/esched_check.cpp -o esched_check
//   ./esched_check
// For a grid of (bin tiles, quad-steps per bin tile, blocks) it walks every
// block's range the way k_estep_mx does (first segment from the formula, then
// whole bin tiles at slot 0) and checks that every unit is owned once, that a
// bin tile's slots are dense from 0, that nseg and the buffer size agree.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../pyfasst_amd/csrc/fasst_esched.h"

using namespace fasst;

static int check(int nbt, int Q, int nb) {
  const long long U = (long long)nbt * Q;
  std::vector<int> owned(U, 0);
  std::vector<std::vector<int>> slots(nbt);
  for (int b = 0; b < nb; ++b) {
    const int wu = (int)es_lo(b, U, nb), wend = (int)es_lo(b + 1, U, nb);
    if (wend <= wu) return 1;                      // no empty block (nb <= U)
    int bt = wu / Q, q0 = wu - bt * Q, nq = std::min(Q - q0, wend - wu);
    int slot = b - es_first(bt, Q, nbt, nb), left = wend - wu - nq;
    for (;;) {
      if (slot < 0 || es_owner((long long)bt * Q + q0, U, nb) != b) return 2;
      for (int q = q0; q < q0 + nq; ++q) ++owned[(size_t)bt * Q + q];
      slots[bt].push_back(slot);
      if (left <= 0) break;
      ++bt, q0 = 0, slot = 0, nq = std::min(Q, left), left -= nq;
    }
  }
  for (long long u = 0; u < U; ++u)
    if (owned[u] != 1) return 3;
  int mx = 1;
  for (int bt = 0; bt < nbt; ++bt) {
    const int n = es_nseg(bt, Q, nbt, nb);
    if ((int)slots[bt].size() != n) return 4;
    for (int i = 0; i < n; ++i)
      if (slots[bt][i] != i) return 5;             // dense, in block order
    mx = std::max(mx, n);
  }
  return es_max_slots(nbt, Q, nb) == mx ? 0 : 6;
}

int main() {
  long n = 0;
  for (int nbt = 1; nbt <= 20; ++nbt)
    for (int Q = 1; Q <= 20; ++Q)
      for (int nb = 1; nb <= nbt * Q; ++nb, ++n)
        if (int e = check(nbt, Q, nb)) {
          std::printf("FAIL %d: nbt=%d Q=%d nb=%d\n", e, nbt, Q, nb);
          return 1;
        }
  const int big[][3] = {{129, 157, 512}, {129, 157, 1024}, {129, 157, 256}, {129, 157, 1},
                        {129, 157, 129 * 157}, {4096, 4001, 2048}, {3, 3, 2}};
  for (const auto &c : big) {
    ++n;
    if (int e = check(c[0], c[1], c[2])) {
      std::printf("FAIL %d: nbt=%d Q=%d nb=%d\n", e, c[0], c[1], c[2]);
      return 1;
    }
  }
  std::printf("esched_check: %ld partitions ok\n", n);
  return 0;
}
