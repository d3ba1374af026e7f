// The input rules of include/crane_gpu_running/running_preempt.h, checked on the host before anything is uploaded: null arguments, the
// call order (a ledger, per-slot tables that are the ledger's), the arrays a cycle with preemption reads and writes, the sizes a
// reference of cns_preempt_out holds, the preempting ids as the device bisects them (ascending, each once), and what the admit step of
// cns_running_advance asks for behind such a cycle.  No HIP in here: engine.hip includes it (running_preempt_host.inc calls it first),
// tests/cpp/running_preempt_host_test.cpp compiles it with g++.  A sibling of running_check_host.inc, whose entry points and
// messages stay as they are.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/crane_gpu_running/running_preempt.h"
#include "preempt_host.inc"   // the rules this call shares with cns_select_preempt, formed under this call's name
#include "running_check_host.inc"

namespace cns_running {

constexpr uint64_t kMaxPreemptRefs = 0x80000000ull;   // a reference of cns_preempt_out carries bit 31 for a pending job: rows and queue indices stay below it

// what cns_running_select_preempt needs to know about the handle
struct PreemptFacts {
  bool have_nodes = false;      // a cns_set_nodes succeeded
  bool have_ledger = false;     // a cns_running_seed succeeded and no cns_set_running / change of num_nodes dropped it
  bool tables_are_ledgers = false;   // the per-slot running tables were built from it and no snapshot call emptied them since
  uint64_t ledger_jobs = 0;
};

// cns_running_select_preempt with preemption enabled (preempt != nullptr, preempt->enabled != 0: the caller has looked)
inline Verdict check_select_preempt(const PreemptFacts& F, const cns_job_soa* jobs, const cns_preempt_soa* pre, const cns_placement_soa* out,
                                    const cns_preempt_out* pout) {
  const char* who = "cns_running_select_preempt";
  if (const Verdict v = cns_preempt::check_order(who, F.have_nodes, jobs, pre, out, pout)) return v;
  if (!F.have_ledger) return refuse(CNS_ERR_STATE, "cns_running_select_preempt before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)");
  if (!F.tables_are_ledgers)
    return refuse(CNS_ERR_STATE, "cns_running_select_preempt: the per-slot running tables are not the ledger's (cns_set_nodes / cns_set_reservations emptied them: call cns_running_advance first)");
  const uint64_t J = jobs->num_jobs, R = F.ledger_jobs;
  if (J >= kMaxPreemptRefs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_select_preempt: 2^31 pending jobs or more (bit 31 of a reference marks a pending job)");
  if (R >= kMaxPreemptRefs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_select_preempt: 2^31 ledger rows or more (bit 31 of a reference marks a pending job)");
  if (const Verdict v = cns_preempt::check_pending(who, J, pre)) return v;
  if (const Verdict v = cns_preempt::check_running(who, R, pre)) return v;
  if (!pre->qos_preempt_offsets || (!pre->qos_preempt && pre->qos_preempt_offsets[pre->num_qos])) return refuse(CNS_ERR_INVALID_ARG, "cns_running_select_preempt: missing array: the QoS preempt lists");
  if (pre->num_preempting && !pre->preempting_job_ids) return refuse(CNS_ERR_INVALID_ARG, "cns_running_select_preempt: missing array: preempting_job_ids");
  return cns_preempt::check_output(who, pout);
}

// m_preempting_set_ as the device bisects it: ascending, each id once
inline std::vector<uint32_t> preempting_sorted(const uint32_t* ids, uint32_t n) {
  std::vector<uint32_t> v(ids, ids + (ids ? n : 0));
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// the row whose rn_job_id is not the ledger's
inline Verdict refuse_row_id(uint64_t row, uint32_t given, uint32_t ledger) {
  return refuse(CNS_ERR_INVALID_ARG, "cns_running_select_preempt: rn_job_id[" + std::to_string(row) + "] is " + std::to_string(given) + ", ledger row " + std::to_string(row) +
                                         " carries job id " + std::to_string(ledger) + " (the running-job arrays are in ledger order)");
}

// cns_running_advance behind check_step, when the last cycle was a cns_running_select_preempt with preemption enabled: only the caller's
// mask tells a job that started from one the commit loop held back ("Waiting for Preemption")
inline Verdict check_step_after_preempt(bool resident_preempt_cycle, const cns_running_step* in) {
  if (resident_preempt_cycle && in->num_jobs && !in->admit)
    return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance: missing array: admit (required after cns_running_select_preempt: the commit loop holds a job that preempted a running job back)");
  return {};
}

}  // namespace cns_running
