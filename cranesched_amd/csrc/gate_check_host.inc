// The input rules of include/crane_gpu_gate/pending_gate.h, checked on the host in one pass over the caller's arrays: missing arrays,
// job_id strictly ascending, the CSR rules of the dependency lists (csr_host.inc) and every list strictly ascending by dep_job, the
// ap_flags bits, the sizes the kernels' 32-bit indices hold.  No HIP in here: engine.hip includes it (gate_host.inc calls it before
// anything is uploaded), tests/cpp/gate_host_test.cpp compiles it with g++.  What passes here is everything the kernels rely on:
// a bisection over job_id, one over a job's list, offsets that cover [0, D) once.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/crane_gpu_gate/pending_gate.h"
#include "csr_host.inc"

namespace cns_gate {

constexpr uint64_t kMaxJobs = 0xFFFFFE00ull;     // 2^32 - 512: a workgroup's last lane index stays a uint32
constexpr uint64_t kMaxEntries = 0xFFFFFF00ull;  // 2^32 - 256 dependency entries
constexpr uint64_t kMaxEvents = 0xFFFFFF00ull;   // 2^32 - 256 events: an event's index is below first_ev's "unclaimed" 0xFFFFFFFF

struct Verdict {
  int code = 0;   // CNS_OK, CNS_ERR_INVALID_ARG or CNS_ERR_UNSUPPORTED
  std::string msg;
  explicit operator bool() const { return code != 0; }
};
struct Sizes {
  uint64_t J = 0, D = 0, E = 0;
  bool has_deps = false;    // dep_is_or / dep_ready_sec are given
  bool has_array = false;   // array_parent and the ap_ arrays are given
};

inline Verdict refuse(int code, std::string msg) {
  Verdict v;
  v.code = code; v.msg = "cns_gate_pending: " + std::move(msg);
  return v;
}

inline Verdict check(const cns_gate_jobs* jb, const cns_gate_events* ev, const cns_gate_out* out, Sizes* sz) {
  Sizes S;
  S.J = jb->num_jobs;
  S.E = ev ? ev->num_events : 0;
  if (S.J > kMaxJobs) return refuse(CNS_ERR_UNSUPPORTED, "more than 2^32 - 512 jobs");
  if (S.E > kMaxEvents) return refuse(CNS_ERR_UNSUPPORTED, "more than 2^32 - 256 events");
  if (S.E && (!ev->dependent_job_id || !ev->dependee_job_id || !ev->event_sec)) return refuse(CNS_ERR_INVALID_ARG, "events with a missing array");
  if (!out->num_pending) return refuse(CNS_ERR_INVALID_ARG, "missing array: out->num_pending");
  if (S.J == 0) { *sz = S; return {}; }
  if (!jb->job_id) return refuse(CNS_ERR_INVALID_ARG, "missing array: job_id");
  if (!out->code || !out->pending) return refuse(CNS_ERR_INVALID_ARG, "missing array: out->code or out->pending");
  if ((jb->dep_is_or == nullptr) != (jb->dep_ready_sec == nullptr)) return refuse(CNS_ERR_INVALID_ARG, "dep_is_or and dep_ready_sec come together");
  S.has_deps = jb->dep_is_or != nullptr;
  for (uint64_t j = 1; j < S.J; ++j)                                                            // the btree order of m_pending_job_map_, :1377
    if (jb->job_id[j] <= jb->job_id[j - 1]) return refuse(CNS_ERR_INVALID_ARG, "job_id is not strictly ascending at row " + std::to_string(j));
  if (jb->dep_offsets) {
    const auto o = cns_csr::check_offsets(jb->dep_offsets, S.J);
    if (o.what == cns_csr::Offsets::FirstNot0) return refuse(CNS_ERR_INVALID_ARG, "dep_offsets[0] != 0");
    if (o.what == cns_csr::Offsets::Decreases) return refuse(CNS_ERR_INVALID_ARG, "dep_offsets decrease at job " + std::to_string(o.index));
    S.D = jb->dep_offsets[S.J];
    if (S.D > kMaxEntries) return refuse(CNS_ERR_UNSUPPORTED, "more than 2^32 - 256 dependency entries");
    if (S.D && (!S.has_deps || !jb->dep_job || !jb->dep_delay_sec))
      return refuse(CNS_ERR_INVALID_ARG, "dependency entries with a missing array (dep_is_or, dep_ready_sec, dep_job, dep_delay_sec)");
    for (uint64_t j = 0; j < S.J; ++j)                                                          // deps is a map: distinct keys, sorted by the packer
      for (uint64_t x = jb->dep_offsets[j] + 1; x < jb->dep_offsets[j + 1]; ++x)
        if (jb->dep_job[x] <= jb->dep_job[x - 1])
          return refuse(CNS_ERR_INVALID_ARG, "the dependency list of row " + std::to_string(j) + " is not strictly ascending at entry " + std::to_string(x));
  }
  if (jb->array_parent) {
    if (!jb->ap_flags || !jb->ap_deadline_sec || !jb->ap_running || !jb->ap_run_limit) return refuse(CNS_ERR_INVALID_ARG, "array_parent with a missing ap_ array");
    S.has_array = true;
    for (uint64_t j = 0; j < S.J; ++j)
      if (jb->ap_flags[j] & ~CNS_GATE_AP_ALL) return refuse(CNS_ERR_INVALID_ARG, "ap_flags[" + std::to_string(j) + "] has a bit outside CNS_GATE_AP_*");
  }
  *sz = S;
  return {};
}

}  // namespace cns_gate
