// Tile tables of the persistent Gram kernels (host only, no HIP call: the Python module binds gram_tile_order so
// a CPU test can walk it).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace dpsvm {
namespace launch {

// Workgroup L of a persistent kernel runs on XCD L % 8 and walks entries L, L + G, ...: chunks of CH consecutive
// tiles of `order` are dealt round-robin to the 8 XCDs (XCD x takes chunks x, x + 8, ...), so that the tiles an
// XCD's CUs run at one time share operand panels in its L2.  The tail that fills no whole round of chunks stays
// in order.
inline std::vector<uint32_t> xcd_deal(const std::vector<uint32_t>& order, int64_t CH) {
  const int64_t total = (int64_t)order.size(), full = total / (8 * CH) * (8 * CH);
  std::vector<uint32_t> tab((size_t)total);
  for (int64_t L = 0; L < total; ++L) {
    int64_t T = L;
    if (L < full) {
      const int64_t xcd = L % 8, local = L / 8;
      T = ((local / CH) * 8 + xcd) * CH + local % CH;
    }
    tab[(size_t)L] = order[(size_t)T];
  }
  return tab;
}

// The one-product pass's table of 256 x 256 tiles for a Gram of tm 256-row tiles by tn 128-COLUMN tiles (the unit
// the hot-tile pass and gram_adapt_last count in): entry (tx << 16) | u is the pair of 256 x 128 tiles (tx, 2 u)
// and (tx, 2 u + 1); with tn odd the last u has a left half only.  Symmetric: tile (tx, u) is needed iff u >= tx
// (its halves are the 256 x 128 tiles with ty >= 2 tx).  Order: groups of GM = 8 tile rows, column by column,
// rows inside a column, dealt to the XCDs in chunks of CH = 32 (8 A panels x 4 B panels of 256 rows: the area of
// the 256 x 128 pass's 8 / 64; 8 / 64, 4 / 32 and 16 / 32 measured within 1% of it,
// profiles/gram_tile256/tile_order_sweep.txt).
inline std::vector<uint32_t> gram_tile_order(int64_t tm, int64_t tn, bool sym) {
  constexpr int64_t GM = 8, CH = 32;
  const int64_t tu = (tn + 1) / 2;
  std::vector<uint32_t> order;
  for (int64_t g0 = 0; g0 < tm; g0 += GM) {
    const int64_t gm = std::min(GM, tm - g0);
    for (int64_t u = 0; u < tu; ++u)
      for (int64_t tx = g0; tx < g0 + gm; ++tx)
        if (!sym || u >= tx) order.push_back((uint32_t)((tx << 16) | u));
  }
  return xcd_deal(order, CH);
}

}  // namespace launch
}  // namespace dpsvm
