// Lookups in a CSR (offsets [n + 1] over one flat array) and in a sorted range, usable from HIP device code (gfx950) and — for the
// CPU unit test of these helpers (tests/cpp/test_dev_helpers.cpp) — from plain host C++.
#pragma once
#include "res_dev.h"

namespace cns {

// the list of flat index i: the last e with off[e] <= i, for n >= 1 lists (off[n] > i; empty lists repeat an offset and are skipped)
template <class Off, class Idx>
CNS_HD u32 csr_owner(const Off* __restrict__ off, u32 n, Idx i) {
  u32 lo = 0, hi = n;   // answer in [lo, hi)
  while (hi - lo > 1) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// is x in the ascending a[b, e)?
template <class Off>
CNS_HD bool sorted_contains(const u32* __restrict__ a, Off b, Off e, u32 x) {
  while (b < e) {
    const Off mid = b + ((e - b) >> 1);
    const u32 v = a[mid];
    if (v == x) return true;
    if (v < x) b = mid + 1; else e = mid;
  }
  return false;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void k_fill_i64(i64* __restrict__ p, u32 n, i64 v) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
#endif

}  // namespace cns
