// CPU test of the pass count of cns_resvq_run's segment sort (cranesched_amd/csrc/resvq_passes.inc): on both sides of every Q at
// which it changes, at the ends of the range, and over a sweep held to the definition (the least p whose digits hold 2 Q - 1).
// Build: g++ -O1 -std=c++17 -Wall -Werror tests/cpp/resvq_passes_test.cpp -o resvq_passes_test
#include <cstdio>

#include "../../cranesched_amd/csrc/resvq_passes.inc"

using cns_resvq::seg_passes;
typedef uint32_t u32;
typedef uint64_t u64;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

// 256^p > 2 Q - 1 (p <= 4: 256^p fits in 64 bits)
static bool holds(u64 Q, u32 p) { return ((u64)1 << (8 * p)) > 2 * Q - 1; }

int main() {
  static_assert(cns_resvq::kDigitBits == 8 && cns_resvq::kMaxSegPasses == 4, "the cases below are written for 8-bit digits of a 32-bit segment");
  const struct { u64 Q; u32 want; } cases[] = {
      {1, 1},          {2, 1},          {128, 1},        {129, 2},           {32768, 2},
      {32769, 3},      {8388608, 3},    {8388609, 4},    {0x7FFFFFFFull, 4},
  };
  for (const auto& c : cases) {
    const u32 p = seg_passes(c.Q);
    if (p != c.want) { printf("FAIL: seg_passes(%llu) = %u, expected %u\n", (unsigned long long)c.Q, p, c.want); ++g_fail; }
    CHECK(holds(c.Q, p));
    CHECK(p == 1 || !holds(c.Q, p - 1));               // ... and no pass more than needed
  }
  // every Q near a power of two and a coarse sweep of the whole range: the least p that holds, never above 4
  u64 checked = 0;
  auto one = [&](u64 Q) {
    if (Q < 1 || Q > 0x7FFFFFFFull) return;
    const u32 p = seg_passes(Q);
    CHECK(p >= 1 && p <= 4);
    CHECK(holds(Q, p));
    CHECK(p == 1 || !holds(Q, p - 1));
    ++checked;
  };
  for (u32 b = 0; b < 31; ++b)
    for (int d = -3; d <= 3; ++d) one(((u64)1 << b) + (u64)(int64_t)d);
  for (u64 Q = 1; Q <= 0x7FFFFFFFull; Q += 104729) one(Q);
  for (u64 Q = 1; Q <= 70000; ++Q) one(Q);
  CHECK(checked > 90000);
  // monotone: more queries never need fewer passes
  for (u64 Q = 1; Q + 65521 <= 0x7FFFFFFFull; Q += 65521) CHECK(seg_passes(Q) <= seg_passes(Q + 1) && seg_passes(Q + 1) <= seg_passes(Q + 65521));
  if (g_fail) { printf("%d failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
