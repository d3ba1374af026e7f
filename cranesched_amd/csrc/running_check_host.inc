// The input rules of include/crane_gpu_running/running.h, checked on the host before anything is uploaded: the rules of cns_set_running
// (snapshot_host.inc: build_running) for the set a ledger is seeded from, offsets that cover [0, num_allocs) once, distinct job ids,
// the sizes the kernels' 32-bit indices hold; for a cycle boundary the retire list (sorted here: the device bisects it), the state the
// admit step needs and what it must match.  No HIP in here: engine.hip includes it (running_host.inc calls it first),
// tests/cpp/running_host_test.cpp compiles it with g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/crane_gpu_running/running.h"

namespace cns_running {

constexpr uint64_t kMaxJobs = 0xFFFFFE00ull;     // 2^32 - 512: a workgroup's last lane index stays a uint32
constexpr uint64_t kMaxAllocs = 0xFFFFFF00ull;   // 2^32 - 256 allocations, and (slot, allocation) pairs

struct Verdict {
  int code = 0;   // CNS_OK, CNS_ERR_INVALID_ARG, CNS_ERR_UNSUPPORTED or CNS_ERR_STATE
  std::string msg;
  explicit operator bool() const { return code != 0; }
};
inline Verdict refuse(int code, std::string msg) {
  Verdict v;
  v.code = code; v.msg = std::move(msg);
  return v;
}

// the first value that stands twice in `sorted`, or none
inline bool first_repeat(const std::vector<uint32_t>& sorted, uint32_t* value) {
  for (size_t i = 1; i < sorted.size(); ++i)
    if (sorted[i] == sorted[i - 1]) { *value = sorted[i]; return true; }
  return false;
}

// cns_running_seed.  N: nodes of the snapshot.  *jobs / *allocs: the sizes of the set (0 / 0 for rn == nullptr or no job).
inline Verdict check_seed(const cns_running_soa* rn, const uint32_t* job_ids, uint32_t N, uint64_t* jobs, uint64_t* allocs) {
  *jobs = *allocs = 0;
  if (!rn || !rn->num_jobs) return {};
  const uint64_t R = rn->num_jobs, A = rn->num_allocs;
  if (R > kMaxJobs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_seed: more than 2^32 - 512 jobs");
  if (A > kMaxAllocs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_seed: more than 2^32 - 256 allocations");
  if (!rn->end_sec || !rn->alloc_offsets || !rn->alloc_node || !rn->alloc_cpu_raw || !rn->alloc_mem || !rn->alloc_core_lo)
    return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed: missing array");
  if (!job_ids) return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed: missing array: job_ids");
  if (rn->alloc_offsets[R] != rn->num_allocs) return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed: num_allocs mismatch");
  if (rn->alloc_offsets[0] != 0) return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed: alloc_offsets[0] != 0");
  for (uint64_t j = 0; j < R; ++j)
    if (rn->alloc_offsets[j + 1] < rn->alloc_offsets[j]) return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed: alloc_offsets decrease at job " + std::to_string(j));
  for (uint64_t a = 0; a < A; ++a)
    if (rn->alloc_node[a] >= N) return refuse(CNS_ERR_INVALID_ARG, "running allocation on node >= num_nodes");
  std::vector<uint32_t> ids(job_ids, job_ids + R);
  std::sort(ids.begin(), ids.end());
  uint32_t twice = 0;
  if (first_repeat(ids, &twice)) return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed: job id " + std::to_string(twice) + " stands twice in job_ids");
  *jobs = R; *allocs = A;
  return {};
}

// what cns_running_advance needs to know about the handle
struct Facts {
  bool have_ledger = false;      // a cns_running_seed succeeded and no cns_set_running / change of num_nodes dropped it
  bool have_cycle = false;       // a cycle finished on this handle and its results stand
  bool preempt_cycle = false;    // ... and it was a cns_select_preempt
  uint64_t cycle_jobs = 0;       // its queue length
  int64_t cycle_now = 0;         // its now
  uint64_t ledger_jobs = 0, ledger_allocs = 0, cycle_places = 0;
};

// cns_running_advance.  *sorted_ids: the retire ids ascending; *order: sorted position -> position in retire_ids.
inline Verdict check_step(const Facts& F, const cns_running_step* in, const cns_running_step_out* out, std::vector<uint32_t>* sorted_ids,
                          std::vector<uint32_t>* order) {
  sorted_ids->clear(); order->clear();
  if (!F.have_ledger) return refuse(CNS_ERR_STATE, "cns_running_advance before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)");
  const uint64_t K = in->num_retire, J = in->num_jobs;
  if (K > kMaxAllocs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_advance: more than 2^32 - 256 retire ids");
  if (K) {
    if (!in->retire_ids) return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: missing array: retire_ids");
    if (!out || !out->found) return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: missing array: out->found");
    order->resize(K);
    for (uint64_t i = 0; i < K; ++i) (*order)[i] = (uint32_t)i;
    std::sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) { return in->retire_ids[a] < in->retire_ids[b]; });
    sorted_ids->resize(K);
    for (uint64_t i = 0; i < K; ++i) (*sorted_ids)[i] = in->retire_ids[(*order)[i]];
    uint32_t twice = 0;
    if (first_repeat(*sorted_ids, &twice)) return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: job id " + std::to_string(twice) + " stands twice in retire_ids");
  }
  if (J) {
    if (!F.have_cycle) return refuse(CNS_ERR_STATE, "cns_running_advance: the admit step needs the results of a successful cycle");
    if (F.preempt_cycle) return refuse(CNS_ERR_STATE, "cns_running_advance: the admit step is not served after cns_select_preempt");
    if (J != F.cycle_jobs)
      return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: num_jobs " + std::to_string(J) + " is not the last cycle's " + std::to_string(F.cycle_jobs));
    if (in->now_sec != F.cycle_now)
      return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: now_sec " + std::to_string(in->now_sec) + " is not the last cycle's " + std::to_string(F.cycle_now));
    if (!in->job_id) return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: missing array: job_id");
    if (F.ledger_jobs + J > kMaxJobs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_advance: more than 2^32 - 512 jobs in the ledger");
    if (F.ledger_allocs + F.cycle_places > kMaxAllocs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_advance: more than 2^32 - 256 allocations in the ledger");
  }
  return {};
}

// the (slot, allocation) pairs of a rebuild are at most allocs x the widest node's slots: they must fit the sort's 32-bit indices
inline Verdict check_pairs(uint64_t allocs, uint64_t widest_node_slots) {
  if (allocs * (widest_node_slots ? widest_node_slots : 1) > kMaxAllocs)
    return refuse(CNS_ERR_UNSUPPORTED, "the running set's allocations times the slots of the node in most partitions exceed 2^32 - 256");
  return {};
}

}  // namespace cns_running
