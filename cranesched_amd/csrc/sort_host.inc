// The arithmetic of the stable pair sort (sort_kernels.inc, driven by sort_call.inc): how many passes a key range needs, how many tiles
// n elements make, how large the histogram is.  No HIP in here: engine.hip includes it (as csr_host.inc), tests/cpp/sort_host_test.cpp
// compiles it with g++.
#pragma once
#include <cstdint>

namespace cns_sort {

constexpr uint32_t kDigitBits = 8;   // one pass of k_sort_hist / k_sort_rowscan / k_sort_scatter sorts by this many bits

// the least number of passes whose digits hold every key in 0 .. max_key: 0 for max_key == 0 (nothing to tell apart), at most 8
inline uint32_t key_passes(uint64_t max_key) {
  uint32_t p = 0;
  while (p * kDigitBits < 64 && (max_key >> (p * kDigitBits)) != 0) ++p;
  return p;
}

// the tiles of `tile` consecutive elements that n elements make (tile: kSortTile)
inline uint32_t tiles(uint32_t n, uint32_t tile) { return (uint32_t)(((uint64_t)n + tile - 1) / tile); }

// the [digit][tile] table of one pass and, behind it, the 256 row totals
inline uint64_t hist_bytes(uint32_t ntiles) { return ((uint64_t)256 * ntiles + 256) * 4; }

}  // namespace cns_sort
