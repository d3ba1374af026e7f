// CPU test of the arithmetic of the shared pair sort (cranesched_amd/csrc/sort_host.inc): the pass count against its definition on both
// sides of every power of 256 and against the loop the callers used to write out, the segment pass count of cns_resvq_run against it,
// the tile count and the histogram's size on both sides of a tile and of a scan span.
// Build: g++ -O1 -std=c++17 -Wall -Werror tests/cpp/sort_host_test.cpp -o sort_host_test
#include <cstdio>

#include "../../cranesched_amd/csrc/sort_host.inc"
#include "../../cranesched_amd/csrc/resvq_passes.inc"

using cns_resvq::seg_passes;
using cns_sort::hist_bytes;
using cns_sort::key_passes;
using cns_sort::tiles;
typedef uint32_t u32;
typedef uint64_t u64;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

// the definition: p digits of 8 bits hold every key up to m (p >= 8: all 64 bits)
static bool holds(u64 m, u32 p) { return p >= 8 || (m >> (8 * p)) == 0; }

// the loop that limits_host.inc, submit_host.inc, usage_host.inc and running_host.inc each wrote out before key_passes, kept here as the definition
// (m < 2^63: above, the loop's last shift would be by 64 bits, which C++ leaves undefined; no caller came near, the counts are 32-bit)
static u32 written_out(u64 m) {
  u32 bits = 0;
  while ((m >> bits) != 0) ++bits;
  u32 pass = 0;
  for (; pass * 8 < bits; ++pass) {}
  return pass;
}

static void one(u64 m) {
  const u32 p = key_passes(m);
  CHECK(p <= 8);
  CHECK(holds(m, p));
  CHECK(p == 0 || !holds(m, p - 1));                   // ... and no pass more than needed
  if ((m >> 63) == 0) CHECK(p == written_out(m));
}

int main() {
  static_assert(cns_sort::kDigitBits == 8, "the cases below are written for 8-bit digits");
  // ---- key_passes: the ends, both sides of every 2^(8 p) ----
  CHECK(key_passes(0) == 0);
  CHECK(key_passes(1) == 1);
  CHECK(key_passes(255) == 1);
  CHECK(key_passes(UINT64_MAX) == 8);
  one(0); one(1); one(UINT64_MAX);
  for (u32 p = 1; p <= 7; ++p) {
    const u64 edge = (u64)1 << (8 * p);
    CHECK(key_passes(edge - 1) == p);
    CHECK(key_passes(edge) == p + 1);
    one(edge - 2); one(edge - 1); one(edge); one(edge + 1);
  }
  for (u32 b = 0; b < 64; ++b)
    for (int d = -3; d <= 3; ++d) one(((u64)1 << b) + (u64)(int64_t)d);
  for (u64 m = 0; m <= 70000; ++m) one(m);
  // a strided sweep of the whole range: the definition, the written-out loop, and monotone
  {
    const u64 stride = 0x0000FFF1FFFFFFF1ull;            // odd, about 2^48: some 65 000 steps
    u64 steps = 0;
    u32 prev = 0;
    for (u64 m = 0;; m += stride) {
      one(m);
      CHECK(key_passes(m) >= prev);
      prev = key_passes(m);
      ++steps;
      if (m > UINT64_MAX - stride) break;
    }
    CHECK(steps > 60000 && prev == 8);
  }

  // ---- seg_passes(Q) == key_passes(2 Q - 1): both sides of every Q at which either side changes, the ends, a sweep ----
  {
    auto same = [](u64 Q) {
      if (Q < 1 || Q > 0x7FFFFFFFull) return;
      CHECK(seg_passes(Q) == key_passes(2 * Q - 1));
    };
    same(1); same(2); same(0x7FFFFFFFull);
    for (u32 p = 1; p <= 4; ++p) {
      const u64 last = ((u64)1 << (8 * p)) / 2;          // the largest Q of p passes: 128, 32 768, 8 388 608, 2^31
      same(last - 1); same(last); same(last + 1); same(last + 2);
    }
    for (u32 b = 0; b < 31; ++b)
      for (int d = -3; d <= 3; ++d) same(((u64)1 << b) + (u64)(int64_t)d);
    for (u64 Q = 1; Q <= 70000; ++Q) same(Q);
    for (u64 Q = 1; Q <= 0x7FFFFFFFull; Q += 104729) same(Q);
    CHECK(seg_passes(128) == 1 && seg_passes(129) == 2 && seg_passes(32768) == 2 && seg_passes(32769) == 3);
    CHECK(seg_passes(8388608) == 3 && seg_passes(8388609) == 4 && seg_passes(0x7FFFFFFFull) == cns_resvq::kMaxSegPasses);
  }

  // ---- tiles and hist_bytes, a tile of 4096: around one tile, around the 256 tiles of one scan step ----
  {
    const struct { u32 n, want; } cases[] = {
        {0, 0}, {1, 1}, {4095, 1}, {4096, 1}, {4097, 2}, {256u * 4096u, 256}, {256u * 4096u + 1, 257},
    };
    for (const auto& c : cases) {
      const u32 t = tiles(c.n, 4096);
      if (t != c.want) { printf("FAIL: tiles(%u, 4096) = %u, expected %u\n", c.n, t, c.want); ++g_fail; }
      CHECK(t == (c.n + 4096 - 1) / 4096);                // as every site wrote it
      CHECK((u64)t * 4096 >= c.n && (t == 0 || (u64)(t - 1) * 4096 < c.n));
      CHECK(hist_bytes(t) == ((u64)256 * t + 256) * 4);   // the [digit][tile] table and the 256 row totals, in 32-bit words
      CHECK(hist_bytes(t) == (u64)256 * (t + 1) * 4);     // (as priority_host.inc wrote it)
    }
    CHECK(hist_bytes(0) == 1024 && hist_bytes(1) == 2048 && hist_bytes(256) == 263168 && hist_bytes(257) == 264192);
    CHECK(tiles(0xFFFFFFEFu, 4096) == 1048576);           // the largest n a caller passes: no 32-bit wrap in n + tile - 1
    CHECK(hist_bytes(1048576) == 1073742848ull);
  }
  if (g_fail) { printf("%d failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
