// How many 8-bit radix passes the segment half of cns_resvq_run's sort needs: the pass count of the shared sort (sort_host.inc) over the
// call's largest segment number.  No HIP in here: engine.hip includes it for resvq_host.inc (as csr_host.inc),
// tests/cpp/resvq_passes_test.cpp compiles it with g++.
#pragma once
#include <cstdint>

#include "sort_host.inc"

namespace cns_resvq {

constexpr uint32_t kDigitBits = 8;       // the digit the segment passes are counted in: the sort's own (below)
constexpr uint32_t kMaxSegPasses = 4;    // the segment is a 32-bit number
static_assert(kDigitBits == cns_sort::kDigitBits, "the segment passes are passes of the shared sort: one digit width");

// A call of Q queries (1 <= Q <= 2^31 - 1) has the segments 0 .. 2 Q - 1: q for a query's plus times, Q + q for its minus times.
// -> the least number of passes p in 1 .. 4 with 2^(8 p) > 2 Q - 1, i.e. every segment number fits in p digits.
inline uint32_t seg_passes(uint64_t num_queries) { return cns_sort::key_passes(2 * num_queries - 1); }

}  // namespace cns_resvq
