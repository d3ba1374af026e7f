// CPU test of the launch plan of k_probe (cranesched_amd/csrc/probe_plan_host.inc): the grid, the heap stride and the scratch bytes
// against their definition — written out here a second time, as properties and not as the routine's own expression — on both sides of
// every min and max: Jg around the resident workgroups, node_num around the widest partition, the cap binding and not, the cap below
// one stride.  And CNS_PROBE_SCRATCH_CAP: it lowers the cap, never raises it, and is ignored where it does not begin with a digit.
// Build: g++ -O1 -std=c++17 -Wall -Werror tests/cpp/probe_plan_test.cpp -o probe_plan_test
#include <cstdio>

#include "../../cranesched_amd/csrc/probe_plan_host.inc"

using cns_probe_plan::kScratchCap;
using cns_probe_plan::Plan;
using cns_probe_plan::plan;
typedef uint32_t u32;
typedef uint64_t u64;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

// The definition, as properties of the answer.
static void one(u64 resident, u64 Jg, u32 max_np, u32 pkmax, u32 ent, u64 cap) {
  ++g_cases;
  const Plan p = plan(resident, Jg, max_np, pkmax, ent, cap);
  bool ok = true;
  // stride: one more than the smaller of the two (a heap of node_num entries takes the push before the pop; no partition has more candidates than slots)
  ok = ok && p.stride >= 1 && p.stride - 1 <= max_np && p.stride - 1 <= pkmax && (p.stride - 1 == max_np || p.stride - 1 == pkmax);
  const u64 per = (u64)p.stride * ent;
  ok = ok && p.bytes == p.grid * per;
  ok = ok && p.grid >= 1;                                                     // a call always has one heap
  ok = ok && (p.grid == 1 || (p.grid <= Jg && p.grid <= resident && p.bytes <= cap));   // more than one only where probes, residency and the cap all allow it
  // ... and no smaller than they allow: one workgroup more would break one of the three
  const u64 next = p.grid + 1;
  ok = ok && (next > Jg || next > (resident ? resident : 1) || next * per > cap);
  if (!ok) { printf("FAIL: plan(%llu, %llu, %u, %u, %u, %llu) = grid %llu stride %u bytes %llu\n", (unsigned long long)resident, (unsigned long long)Jg, max_np, pkmax, ent,
                    (unsigned long long)cap, (unsigned long long)p.grid, p.stride, (unsigned long long)p.bytes); ++g_fail; }
}

int main() {
  const u32 ent = 80;   // (any size: the routine takes it as an argument; the engine hands over sizeof(HeapEnt), which cns_probe_shape names)
  // ---- literal answers: each min and max on both sides ----
  {
    const u64 R = 1024;
    // Jg against the resident workgroups
    CHECK(plan(R, 0, 129, 1, ent, kScratchCap).grid == 1);
    CHECK(plan(R, 1, 129, 1, ent, kScratchCap).grid == 1);
    CHECK(plan(R, R - 1, 129, 1, ent, kScratchCap).grid == R - 1);
    CHECK(plan(R, R, 129, 1, ent, kScratchCap).grid == R);
    CHECK(plan(R, R + 1, 129, 1, ent, kScratchCap).grid == R);
    CHECK(plan(0, 5, 129, 1, ent, kScratchCap).grid == 1);     // no occupancy figure: one workgroup
    // node_num against the widest partition
    for (u32 np : {3u, 65u, 129u}) {
      CHECK(plan(R, 7, np, np - 1, ent, kScratchCap).stride == np);
      CHECK(plan(R, 7, np, np, ent, kScratchCap).stride == np + 1);
      CHECK(plan(R, 7, np, np + 1, ent, kScratchCap).stride == np + 1);
      CHECK(plan(R, 7, np, 0xFFFFFFFEu, ent, kScratchCap).stride == np + 1);
    }
    CHECK(plan(R, 7, 129, 1, ent, kScratchCap).stride == 2 && plan(R, 7, 129, 1, ent, kScratchCap).bytes == 7ull * 2 * ent);
    // the cap: stride 130 -> 10400 bytes a workgroup
    const u64 per = 130ull * ent;
    CHECK(plan(R, 201, 129, 129, ent, 201 * per).grid == 201);          // exactly enough: not binding
    CHECK(plan(R, 201, 129, 129, ent, 201 * per - 1).grid == 200);      // one byte short: binding
    CHECK(plan(R, 201, 129, 129, ent, 2 * per).grid == 2);
    CHECK(plan(R, 201, 129, 129, ent, 2 * per - 1).grid == 1);
    CHECK(plan(R, 201, 129, 129, ent, per).grid == 1);
    CHECK(plan(R, 201, 129, 129, ent, per / 2).grid == 1);              // below one stride: the grid stays 1 ...
    CHECK(plan(R, 201, 129, 129, ent, per / 2).bytes == per);           // ... and that workgroup has its whole heap
    CHECK(plan(R, 201, 129, 129, ent, 0).grid == 1 && plan(R, 201, 129, 129, ent, 0).bytes == per);
    // the shipped cap: thousands of probes over thousands of nodes
    CHECK(plan(8192, 8192, 262144, 4000, ent, kScratchCap).grid == kScratchCap / (4001ull * ent));
    CHECK(plan(8192, 8192, 262144, 100, ent, kScratchCap).grid == 8192);
    // the widest input: nothing wraps in 64 bits
    const Plan w = plan(~0ull, ~0ull, 0xFFFFFFFEu, 0xFFFFFFFEu, ent, kScratchCap);
    CHECK(w.stride == 0xFFFFFFFFu && w.grid == 1 && w.bytes == 0xFFFFFFFFull * ent);
  }
  // ---- the definition over a grid of inputs around every edge ----
  {
    const u64 residents[] = {0, 1, 2, 255, 256, 1024, 8192};
    const u32 nps[] = {1, 3, 63, 64, 65, 129, 4096};
    for (u64 R : residents)
      for (u32 np : nps) {
        const u32 ks[] = {1, 2, np > 1 ? np - 1 : 1, np, np + 1, 1000000};
        for (u32 k : ks) {
          const u64 Jgs[] = {0, 1, 2, R ? R - 1 : 0, R, R + 1, 3 * R + 7};
          for (u64 Jg : Jgs) {
            const u64 per = ((u64)(np < k ? np : k) + 1) * ent;
            const u64 g0 = Jg < R ? Jg : R;
            const u64 caps[] = {0, 1, per / 2, per - 1, per, per + 1, 2 * per - 1, 2 * per, g0 * per - 1 + (g0 == 0), g0 * per, g0 * per + 1, kScratchCap};
            for (u64 cap : caps) one(R, Jg, np, k, ent, cap);
          }
        }
      }
    CHECK(g_cases > 20000);
  }
  // ---- resident(): the occupancy figure x the compute units, each at least 1 ----
  CHECK(cns_probe_plan::resident(0, 0) == 1 && cns_probe_plan::resident(-3, 256) == 256 && cns_probe_plan::resident(8, 0) == 8 && cns_probe_plan::resident(8, 256) == 2048);
  CHECK(cns_probe_plan::resident(0x7FFFFFFF, 0xFFFFFFFFu) == 0x7FFFFFFFull * 0xFFFFFFFFull);
  // ---- the environment variable lowers the cap, never raises it ----
  unsetenv("CNS_PROBE_SCRATCH_CAP");
  CHECK(cns_probe_plan::scratch_cap() == kScratchCap && kScratchCap == (1ull << 30));
  setenv("CNS_PROBE_SCRATCH_CAP", "", 1);
  CHECK(cns_probe_plan::scratch_cap() == kScratchCap);
  setenv("CNS_PROBE_SCRATCH_CAP", "20800", 1);
  CHECK(cns_probe_plan::scratch_cap() == 20800);
  setenv("CNS_PROBE_SCRATCH_CAP", "0", 1);
  CHECK(cns_probe_plan::scratch_cap() == 0);
  setenv("CNS_PROBE_SCRATCH_CAP", "1073741823", 1);
  CHECK(cns_probe_plan::scratch_cap() == kScratchCap - 1);
  setenv("CNS_PROBE_SCRATCH_CAP", "1073741825", 1);
  CHECK(cns_probe_plan::scratch_cap() == kScratchCap);
  setenv("CNS_PROBE_SCRATCH_CAP", "99999999999999999999999", 1);
  CHECK(cns_probe_plan::scratch_cap() == kScratchCap);
  for (const char* junk : {"abc", "-1", " 5", "+7", "x20800", "k"}) {      // no leading digit: ignored, not read as 0
    setenv("CNS_PROBE_SCRATCH_CAP", junk, 1);
    CHECK(cns_probe_plan::scratch_cap() == kScratchCap);
  }
  setenv("CNS_PROBE_SCRATCH_CAP", "20800abc", 1);                          // digits first: their value
  CHECK(cns_probe_plan::scratch_cap() == 20800);
  if (g_fail) { printf("%d failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
