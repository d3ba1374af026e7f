// The launch plan of k_probe (probe_kernel.inc, launched by probe_host.inc): how many persistent one-wave workgroups, how many HeapEnt
// each of them owns, how many bytes of scratch that makes.  No HIP in here: engine.hip includes it (as sort_host.inc),
// tests/cpp/probe_plan_test.cpp compiles it with g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace cns_probe_plan {

constexpr uint64_t kScratchCap = 1ull << 30;   // at most 1 GiB of heap scratch (a probe over thousands of nodes of a giant partition)

struct Plan {
  uint64_t grid;     // workgroups: as many as are resident at once, never more than there are probes, never more than the cap pays for, never 0
  uint32_t stride;   // HeapEnt per workgroup: min(widest partition, widest node_num of the call) + 1 (the push before the pop)
  uint64_t bytes;    // grid * stride * heap_ent_bytes
};

// resident: workgroups of k_probe the device holds at once | Jg: probes that reach a walk (>= 1 where a launch is planned; 0 plans one
// workgroup that finds nothing to take) | max_np: slots of the widest partition | pkmax: the widest node_num of the call | cap: bytes.
// A cap below one stride leaves one workgroup: a probe needs its whole heap, and one heap is what a call may always have.
inline Plan plan(uint64_t resident, uint64_t Jg, uint32_t max_np, uint32_t pkmax, uint32_t heap_ent_bytes, uint64_t cap) {
  Plan p;
  p.stride = std::min<uint32_t>(max_np, pkmax) + 1u;   // (max_np, pkmax < 2^32 - 1: node counts)
  const uint64_t per = (uint64_t)p.stride * heap_ent_bytes;
  uint64_t grid = std::min<uint64_t>(Jg, std::max<uint64_t>(resident, 1));
  grid = std::max<uint64_t>(1, std::min<uint64_t>(grid, cap / per));
  p.grid = grid;
  p.bytes = grid * per;
  return p;
}

// the workgroups of k_probe the device holds at once: the runtime's occupancy figure (0 where it gave none) x the compute units
inline uint64_t resident(int per_cu, uint32_t num_cus) { return (uint64_t)std::max(per_cu, 1) * std::max<uint32_t>(num_cus, 1); }

// CNS_PROBE_SCRATCH_CAP (bytes) lowers the cap (tests: the cap binding without thousands of wide probes); it never raises it.  A value
// that does not begin with a digit is ignored: a typing error must not put every probe call on one workgroup.
inline uint64_t scratch_cap() {
  const char* e = getenv("CNS_PROBE_SCRATCH_CAP");
  if (!e || *e < '0' || *e > '9') return kScratchCap;
  return std::min<uint64_t>(kScratchCap, strtoull(e, nullptr, 10));
}

}  // namespace cns_probe_plan
