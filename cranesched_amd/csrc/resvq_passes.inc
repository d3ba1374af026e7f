// How many 8-bit radix passes the segment half of cns_resvq_run's sort needs.  No HIP in here: engine.hip includes it for
// resvq_host.inc (as csr_host.inc), tests/cpp/resvq_passes_test.cpp compiles it with g++.
#pragma once
#include <cstdint>

namespace cns_resvq {

constexpr uint32_t kDigitBits = 8;       // one pass of k_sort_hist / k_sort_rowscan / k_sort_scatter sorts by this many bits
constexpr uint32_t kMaxSegPasses = 4;    // the segment is a 32-bit number

// A call of Q queries (1 <= Q <= 2^31 - 1) has the segments 0 .. 2 Q - 1: q for a query's plus times, Q + q for its minus times.
// -> the least number of passes p in 1 .. 4 with 2^(8 p) > 2 Q - 1, i.e. every segment number fits in p digits.
inline uint32_t seg_passes(uint64_t num_queries) {
  const uint64_t last = 2 * num_queries - 1;
  uint32_t p = 1;
  while (p < kMaxSegPasses && (last >> (kDigitBits * p))) ++p;
  return p;
}

}  // namespace cns_resvq
