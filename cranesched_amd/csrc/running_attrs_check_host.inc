// The input rules of include/crane_gpu_running/running_attrs.h, checked on the host before anything is uploaded: the attribute arrays
// of a seed and of a cycle boundary, the state the consumers need (a ledger, columns on it), the pending side of
// cns_priority_order_resident as cns_priority_order checks it, the arrays cns_running_select_preempt_attrs must NOT be handed, and the
// two refusals that start from a device flag word: the least row whose account is out of range, the least row whose sums are.  No HIP
// in here: engine.hip includes it (running_attrs_host.inc calls it first), tests/cpp/running_attrs_host_test.cpp compiles it with g++.
// A sibling of running_check_host.inc and running_preempt_check_host.inc, whose entry points and messages stay as they are.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/crane_gpu_running/running_attrs.h"
#include "running_preempt_check_host.inc"

namespace cns_running {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;   // a flag word no row was recorded in

inline const char* no_columns_hint() {
  return "the ledger carries no attribute columns (a plain cns_running_seed / cns_running_advance drops them: seed with cns_running_seed_attrs)";
}

inline bool attrs_complete(const cns_running_attrs* a, bool need_start) {
  return a && (!need_start || a->start_sec) && a->qos && a->qos_priority && a->partition_priority && a->account;
}

// cns_running_seed_attrs, behind check_seed.  jobs: rows of the set.
inline Verdict check_seed_attrs(uint64_t jobs, const cns_running_attrs* attrs) {
  if (jobs && !attrs_complete(attrs, true)) return refuse(CNS_ERR_INVALID_ARG, "cns_running_seed_attrs: missing attribute array");
  return {};
}

// cns_running_advance_attrs, behind check_step and check_step_after_preempt
inline Verdict check_step_attrs(bool have_columns, const cns_running_step* in, const cns_running_attrs* queue_attrs) {
  if (!have_columns) return refuse(CNS_ERR_STATE, std::string("cns_running_advance_attrs: ") + no_columns_hint());
  if (in->num_jobs && !attrs_complete(queue_attrs, false))
    return refuse(CNS_ERR_INVALID_ARG, "cns_running_advance_attrs: missing attribute array of the queue (qos, qos_priority, partition_priority, account)");
  return {};
}

// cns_running_get_attrs
inline Verdict check_get_attrs(bool have_ledger, bool have_columns, const cns_running_attrs_out* o, uint64_t ledger_jobs) {
  if (!o) return refuse(CNS_ERR_INVALID_ARG, "cns_running_get_attrs: null argument");
  if (!have_ledger) return refuse(CNS_ERR_STATE, "cns_running_get_attrs before cns_running_seed_attrs (cns_set_running and a changed num_nodes drop the ledger)");
  if (!have_columns) return refuse(CNS_ERR_STATE, std::string("cns_running_get_attrs: ") + no_columns_hint());
  const bool any = o->start_sec || o->qos || o->qos_priority || o->partition_priority || o->account || o->node_num || o->alloc_cpu_raw || o->alloc_mem;
  if (any && o->capacity_jobs < ledger_jobs) return refuse(CNS_ERR_INVALID_ARG, "cns_running_get_attrs: the arrays are smaller than the ledger");
  return {};
}

// cns_priority_order_resident: the arguments and the state
inline Verdict check_order_resident(bool have_ledger, bool have_columns, const cns_priority_config* cfg, const cns_prio_pending_soa* pd, const uint32_t* order_out,
                                    const double* priority_out, const uint64_t* num_ordered) {
  if (!cfg || !pd || !num_ordered) return refuse(CNS_ERR_INVALID_ARG, "cns_priority_order_resident: null argument");
  if (pd->num_jobs && (!pd->submit_sec || !pd->qos_priority || !pd->partition_priority || !pd->node_num || !pd->total_cpu_raw || !pd->total_mem || !pd->account ||
                       !order_out || !priority_out))
    return refuse(CNS_ERR_INVALID_ARG, "cns_priority_order_resident: missing pending array");
  if (!have_ledger) return refuse(CNS_ERR_STATE, "cns_priority_order_resident before cns_running_seed_attrs (cns_set_running and a changed num_nodes drop the ledger)");
  if (!have_columns) return refuse(CNS_ERR_STATE, std::string("cns_priority_order_resident: ") + no_columns_hint());
  return {};
}

// ... its pending side, by the rules and the messages of cns_priority_order
inline Verdict check_order_pending(const cns_prio_pending_soa* pd, uint32_t num_accounts) {
  for (uint32_t i = 0; i < pd->num_jobs; ++i) {
    if (pd->account[i] >= num_accounts) return refuse(CNS_ERR_INVALID_ARG, "pending job account >= num_accounts");
    if (pd->total_cpu_raw[i] < 0) return refuse(CNS_ERR_INVALID_ARG, "negative cpu request");
  }
  return {};
}

// ... and what the device recorded of the running side: the least row with an account >= num_accounts, with a negative cpu sum, with a
// sum that leaves its type (kNoRow: none).  The least row decides; on one row the account goes first, then the range, then the sign.
enum { kRowFine = 0, kRowAccount, kRowSumRange, kRowCpuNegative };
inline int worst_row(uint32_t account_row, uint32_t negative_row, uint32_t range_row, uint32_t* row) {
  const uint32_t least = account_row < negative_row ? (account_row < range_row ? account_row : range_row) : (negative_row < range_row ? negative_row : range_row);
  *row = least;
  if (least == kNoRow) return kRowFine;
  return least == account_row ? kRowAccount : least == range_row ? kRowSumRange : kRowCpuNegative;
}
inline Verdict refuse_account_row(uint32_t row, uint32_t account, uint32_t num_accounts) {
  return refuse(CNS_ERR_INVALID_ARG, "cns_priority_order_resident: ledger row " + std::to_string(row) + " carries account " + std::to_string(account) +
                                         ", num_accounts is " + std::to_string(num_accounts) + " (running job account >= num_accounts)");
}
inline Verdict refuse_sum_row(uint32_t row, int kind) {
  if (kind == kRowCpuNegative)
    return refuse(CNS_ERR_INVALID_ARG, "cns_priority_order_resident: the cpu of ledger row " + std::to_string(row) + "'s allocations sums to a negative value (negative cpu allocation)");
  return refuse(CNS_ERR_UNSUPPORTED, "cns_priority_order_resident: the allocations of ledger row " + std::to_string(row) + " sum to a cpu value outside int64 or a memory value outside uint64");
}

// cns_running_select_preempt_attrs with preemption enabled (preempt != nullptr, preempt->enabled != 0: the caller has looked)
inline Verdict check_select_preempt_attrs(const PreemptFacts& F, bool have_columns, const cns_job_soa* jobs, const cns_preempt_soa* pre, const cns_placement_soa* out,
                                          const cns_preempt_out* pout) {
  const char* who = "cns_running_select_preempt_attrs";
  if (const Verdict v = cns_preempt::check_order(who, F.have_nodes, jobs, pre, out, pout)) return v;
  if (!F.have_ledger) return refuse(CNS_ERR_STATE, "cns_running_select_preempt_attrs before cns_running_seed_attrs (cns_set_running and a changed num_nodes drop the ledger)");
  if (!have_columns) return refuse(CNS_ERR_STATE, std::string("cns_running_select_preempt_attrs: ") + no_columns_hint());
  if (!F.tables_are_ledgers)
    return refuse(CNS_ERR_STATE, "cns_running_select_preempt_attrs: the per-slot running tables are not the ledger's (cns_set_nodes / cns_set_reservations emptied them: call cns_running_advance_attrs first)");
  const uint64_t J = jobs->num_jobs, R = F.ledger_jobs;
  if (J >= kMaxPreemptRefs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_select_preempt_attrs: 2^31 pending jobs or more (bit 31 of a reference marks a pending job)");
  if (R >= kMaxPreemptRefs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_select_preempt_attrs: 2^31 ledger rows or more (bit 31 of a reference marks a pending job)");
  if (pre->rn_job_id || pre->rn_qos || pre->rn_qos_priority || pre->rn_start_sec)
    return refuse(CNS_ERR_INVALID_ARG, "cns_running_select_preempt_attrs: rn_job_id, rn_qos, rn_qos_priority and rn_start_sec must be NULL: the call reads the ledger's columns, not the caller's arrays");
  if (const Verdict v = cns_preempt::check_pending(who, J, pre)) return v;
  if (!pre->qos_preempt_offsets || (!pre->qos_preempt && pre->qos_preempt_offsets[pre->num_qos])) return refuse(CNS_ERR_INVALID_ARG, "cns_running_select_preempt_attrs: missing array: the QoS preempt lists");
  if (pre->num_preempting && !pre->preempting_job_ids) return refuse(CNS_ERR_INVALID_ARG, "cns_running_select_preempt_attrs: missing array: preempting_job_ids");
  return cns_preempt::check_output(who, pout);
}

}  // namespace cns_running
