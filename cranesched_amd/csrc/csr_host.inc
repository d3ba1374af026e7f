// The CSR rules of the callers' lists, checked on the host: an offsets array [n + 1] starts at 0 and never decreases; a node list is
// sorted here and then names no node twice and — where the caller gives a bound — no node at or above it.  No HIP in here: engine.hip
// includes it, tests/cpp/csr_host_test.cpp compiles it with g++.  The callers form their own messages from what comes back.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace cns_csr {

// the first i in [0, n) with off[i + 1] < off[i]; n: none
template <class Off>
uint64_t first_decrease(const Off* off, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return i;
  return n;
}

enum class Offsets : uint8_t { Ok, FirstNot0, Decreases };
struct OffsetsVerdict {
  Offsets what;
  uint64_t index;   // Decreases: the first i with off[i + 1] < off[i]
};
// offsets [n + 1]: the first offset before any decrease
template <class Off>
OffsetsVerdict check_offsets(const Off* off, uint64_t n) {
  if (off[0] != 0) return {Offsets::FirstNot0, 0};
  const uint64_t i = first_decrease(off, n);
  return i < n ? OffsetsVerdict{Offsets::Decreases, i} : OffsetsVerdict{Offsets::Ok, 0};
}

constexpr uint64_t kNoBound = ~0ull;
enum class Lists : uint8_t { Ok, Repeated, OutOfBound };
struct ListsVerdict {
  Lists what;
  uint64_t list;    // the offending list ...
  uint32_t value;   // ... and the value it repeats, or names at or above the bound
};
// The lists [beg, end) of a CSR whose offsets do not decrease there: each copied from src to dst (the same positions; src != dst) and
// sorted in dst, then walked in ascending order — the first value >= bound or equal to its predecessor ends the pass.  The entries of
// dst outside these lists are not touched, so chunks of the lists can run on threads of their own.
template <class Off>
ListsVerdict sort_lists(const Off* off, const uint32_t* src, uint32_t* dst, uint64_t beg, uint64_t end, uint64_t bound = kNoBound) {
  for (uint64_t l = beg; l < end; ++l) {
    const Off b = off[l], e = off[l + 1];
    if (e == b) continue;
    memcpy(dst + b, src + b, (size_t)(e - b) * 4);
    std::sort(dst + b, dst + e);
    for (Off x = b; x < e; ++x) {
      if (dst[x] >= bound) return {Lists::OutOfBound, l, dst[x]};
      if (x > b && dst[x] == dst[x - 1]) return {Lists::Repeated, l, dst[x]};
    }
  }
  return {Lists::Ok, 0, 0};
}

}  // namespace cns_csr
