// The host side of a cycle with preemption (include/crane_gpu/preempt.h), stated once: which pending jobs may preempt, the flattened QoS
// lists, the size plan of the cycle's work buffers, the running side of cns_select_preempt (marks, set_in, the job -> entries CSR, the
// end patch), the fold of the device's (pending job, reference) pairs into cns_preempt_out with its refusals, the two endings that only
// write the preempting set out, and the input rules of cns_select_preempt.  Plain pointers, vectors and the ABI structs: no HIP, no
// handle.  engine.hip (pre_cycle, cns_select_preempt, run_resident_once) ensures, uploads, resets and downloads from these values;
// tests/cpp/preempt_host_test.cpp compiles this file with g++ (tests/test_preempt_host.py: hand rows, the running side against
// tests/running_preempt_pyref.py, the fold against the oracle).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/crane_gpu/preempt.h"
#include "jobs_host.inc"            // align16, kNoPart
#include "running_check_host.inc"   // Verdict, refuse

namespace cns_preempt {

using cns_running::Verdict;
using cns_running::refuse;
using cns_jobs_host::align16;
using u32 = uint32_t;
using u64 = uint64_t;
using i64 = int64_t;

// ---- the input rules of cns_select_preempt; the calls of running_preempt.h / running_attrs.h form the same messages under their names ----
inline Verdict check_order(const std::string& who, bool have_nodes, const cns_job_soa* jobs, const cns_preempt_soa* pre, const cns_placement_soa* out,
                           const cns_preempt_out* pout) {
  if (!jobs || !pre || !out || !pout) return refuse(CNS_ERR_INVALID_ARG, who + ": null argument");
  if (!have_nodes) return refuse(CNS_ERR_STATE, who + " before cns_set_nodes");
  return {};
}
inline Verdict check_pending(const std::string& who, u64 J, const cns_preempt_soa* pre) {
  if (J && (!pre->pd_qos || !pre->pd_qos_priority || !pre->pd_priority)) return refuse(CNS_ERR_INVALID_ARG, who + ": missing pending-job array");
  return {};
}
inline Verdict check_running(const std::string& who, u64 R, const cns_preempt_soa* pre) {
  if (R && (!pre->rn_job_id || !pre->rn_qos || !pre->rn_qos_priority || !pre->rn_start_sec)) return refuse(CNS_ERR_INVALID_ARG, who + ": missing running-job array");
  return {};
}
inline Verdict check_output(const std::string& who, const cns_preempt_out* pout) {
  if (!pout->offsets || !pout->preempted || !pout->cancelled_job_ids || !pout->preempting_job_ids) return refuse(CNS_ERR_INVALID_ARG, who + ": missing output array");
  return {};
}
// cns_select_preempt with preemption enabled (preempt != nullptr, preempt->enabled != 0: the caller has looked); tables_from_ledger: the
// per-slot running tables were built on the device, the host holds no entries for them
inline Verdict check_select_preempt(bool have_nodes, bool tables_from_ledger, const cns_job_soa* jobs, const cns_preempt_soa* pre, const cns_placement_soa* out,
                                    const cns_preempt_out* pout) {
  if (const Verdict v = check_order("cns_select_preempt", have_nodes, jobs, pre, out, pout)) return v;
  if (tables_from_ledger)
    return refuse(CNS_ERR_STATE, "cns_select_preempt: the running tables were built on the device (cns_running_seed / cns_running_advance); hand the running set in with cns_set_running first");
  return {};
}
// ... and its arrays, once the running set's size is known (R: cns_set_running's jobs)
inline Verdict check_select_preempt_arrays(u64 J, u64 R, const cns_preempt_soa* pre, const cns_preempt_out* pout) {
  if (const Verdict v = check_pending("cns_select_preempt", J, pre)) return v;
  if (const Verdict v = check_running("cns_select_preempt", R, pre)) return v;
  return check_output("cns_select_preempt", pout);
}

// ---- which pending jobs may preempt (TryPreempt_ returns at JobScheduler.cpp:6385 for the others) ----
inline bool may_preempt(const cns_preempt_soa* pre, u64 j) {
  const u32 q = pre->pd_qos[j];
  return q < pre->num_qos && pre->qos_preempt_offsets[q + 1] > pre->qos_preempt_offsets[q];
}
// no job of the queue may: the cycle is the plain one (with the preempting jobs ending at now + 1) and runs on the pipelined kernels
inline bool any_may_preempt(const cns_preempt_soa* pre, u64 J) {
  for (u64 j = 0; j < J; ++j)
    if (may_preempt(pre, j)) return true;
  return false;
}
// the engine partitions that have such a job: only they run on k_select's general path.  job_part: job -> engine partition (kNoPart: not
// given to an ordered loop; a shorter table says nothing about the jobs behind it)
inline std::vector<uint8_t> parts_that_may_preempt(const cns_preempt_soa* pre, u64 J, const std::vector<u32>& job_part, u32 P) {
  std::vector<uint8_t> pre_part(P, 0);
  for (u64 j = 0; j < J && j < job_part.size(); ++j)
    if (job_part[(size_t)j] != cns_jobs_host::kNoPart && may_preempt(pre, j)) pre_part[job_part[(size_t)j]] = 1;
  return pre_part;
}

// ---- what goes to the device as it is ----
// the QoS preempt lists flattened; an empty `flat` keeps one element (no zero-byte upload)
struct QosLists {
  std::vector<u32> off, flat;   // [num_qos + 1], [max(off[num_qos], 1)]
};
inline QosLists qos_lists(const cns_preempt_soa* pre) {
  QosLists L;
  L.off.assign((size_t)pre->num_qos + 1, 0);
  for (u32 q = 0; q < pre->num_qos; ++q) {
    for (u32 i = pre->qos_preempt_offsets[q]; i < pre->qos_preempt_offsets[q + 1]; ++i) L.flat.push_back(pre->qos_preempt[i]);
    L.off[q + 1] = (u32)L.flat.size();
  }
  if (L.flat.empty()) L.flat.push_back(0);
  return L;
}
// a caller's per-job array as a table of max(n, 1) rows
template <class T, class S>
inline std::vector<T> padded(const S* src, u64 n) {
  std::vector<T> v((size_t)std::max<u64>(n, 1), T(0));
  for (u64 i = 0; i < n; ++i) v[(size_t)i] = (T)src[i];
  return v;
}

// ---- the size plan of the cycle's work buffers (documented in include/crane_gpu/preempt.h) ----
// Candidate / chosen lists per partition sized for every running job plus every pending job of the cycle (at most all of them hold
// resources on one job's nodes), bounded by 64 Mi entries over all partitions; segment-tree pools of pool_nodes nodes.  Exceeding either
// is CNS_ERR_UNSUPPORTED, not a device fault.  pre_cycle ensures from these sizes, run_resident_once resets from them at every pass.
struct PlanIn {
  u64 J = 0, places = 0;        // pending jobs, their placement records
  u32 R = 0, A = 0;             // running jobs, entries of the per-slot running tables
  u32 P = 0, S = 0;             // engine partitions, slots
  u32 pool_nodes = 0;           // nodes of a partition's segment-tree pool (kPrePoolNodes)
  size_t node_bytes = 0;        // ... and the bytes of one (sizeof(PreNode))
};
struct Plan {
  u32 cand_cap = 0, out_cap = 0, pool_nodes = 0;
  size_t pj4 = 0, pj8 = 0;              // per pending job: a dword (pj_rec0, pj_k), a qword (pj_end)
  size_t ent_gone = 0, slot_head = 0;   // a byte per entry, a dword per slot: reset at every pass (0 / 0xFF)
  size_t rec4 = 0, rec_gone = 0;        // per placement record: a dword (rec_next, rec_orig, rec_slot), a byte (reset at every pass: 0)
  // one block for: segment-tree pools | candidate lists | chosen lists | output counter | output pairs
  size_t off_cand = 0, off_chosen = 0, off_cnt = 0, off_out = 0, misc = 0;
  size_t cnt_bytes = 16;                // the counter's slot: reset at every pass (0)
};
inline Plan plan_buffers(const PlanIn& in) {
  Plan p;
  const u64 J = in.J, places = std::max<u64>(in.places, 1);
  p.pool_nodes = in.pool_nodes;
  p.cand_cap = (u32)std::max<u64>(4096, std::min<u64>((u64)in.R + J + 1, (64ull << 20) / std::max<u32>(in.P, 1)));
  p.out_cap = (u32)std::min<u64>(4 * (J + in.R) + 64, 1u << 28);
  p.pj4 = std::max<u64>(J, 1) * 4; p.pj8 = std::max<u64>(J, 1) * 8;
  p.ent_gone = std::max<u32>(in.A, 1);
  p.slot_head = (size_t)std::max<u32>(in.S, 1) * 4;
  p.rec4 = places * 4; p.rec_gone = places;
  const size_t pool_b = (size_t)in.P * in.pool_nodes * in.node_bytes, cand_b = (size_t)in.P * p.cand_cap * 4;
  p.off_cand = align16(pool_b); p.off_chosen = p.off_cand + align16(cand_b); p.off_cnt = p.off_chosen + align16(cand_b); p.off_out = p.off_cnt + p.cnt_bytes;
  p.misc = p.off_out + (size_t)p.out_cap * 8;
  return p;
}

// ---- the running side of cns_select_preempt ----
// m_preempting_set_: ids that no longer run are dropped, the others end at now + 1 (JobScheduler.cpp:6545-6559).  ent_job / rn_end: the
// entries of the per-slot running tables (snapshot_host.inc: RunLayout), R: the running jobs.
struct RunSide {
  // id -> row (the first row of an id that stands twice).  Part of the value for its lifetime: taking a map of a million ids down costs
  // milliseconds, and it goes down with the value, behind the cycle, not in front of it.  First member: freed last.
  std::map<u32, u32> id_to_rn;
  std::vector<uint8_t> rj_preempting;      // [max(R, 1)] the job stands in the preempting set
  std::vector<u32> set_in;                 // the ids of the set that still run, in the caller's order (an id that stands twice stays twice)
  std::vector<i64> ent_end;                // [A] rn_end with the entries of the preempting jobs at now + 1
  std::vector<i64> rj_end, rj_start;       // [max(R, 1)] per job max(end of its last entry, now + 1) (:6513-6514; 0: no entry), the caller's start
  std::vector<u32> rj_qos, rj_qprio;       // [max(R, 1)] the caller's fields
  std::vector<u32> rj_off, rj_ent;         // [R + 1], [max(A, 1)] job -> its entries, ascending
  bool patched = false;                    // ent_end is not rn_end
};
inline RunSide running_side(const std::vector<u32>& ent_job, const std::vector<i64>& rn_end, u32 R, const cns_preempt_soa* pre, i64 now) {
  RunSide s;
  const u32 A = (u32)ent_job.size();
  for (u32 r = 0; r < R; ++r) s.id_to_rn.emplace(pre->rn_job_id[r], r);
  s.rj_preempting.assign(std::max<u32>(R, 1), 0);
  for (u32 i = 0; i < pre->num_preempting; ++i) {
    auto it = s.id_to_rn.find(pre->preempting_job_ids[i]);
    if (it == s.id_to_rn.end()) continue;
    s.rj_preempting[it->second] = 1;
    s.set_in.push_back(pre->preempting_job_ids[i]);
  }
  s.ent_end = rn_end; s.rj_end.assign(std::max<u32>(R, 1), 0);
  s.rj_start = padded<i64>(pre->rn_start_sec, R); s.rj_qos = padded<u32>(pre->rn_qos, R); s.rj_qprio = padded<u32>(pre->rn_qos_priority, R);
  s.rj_off.assign((size_t)R + 1, 0); s.rj_ent.assign(std::max<u32>(A, 1), 0);
  for (u32 d = 0; d < A; ++d) s.rj_off[ent_job[d] + 1]++;
  for (u32 r = 0; r < R; ++r) s.rj_off[r + 1] += s.rj_off[r];
  {
    std::vector<u32> cur(s.rj_off.begin(), s.rj_off.end() - 1);
    for (u32 d = 0; d < A; ++d) s.rj_ent[cur[ent_job[d]]++] = d;
  }
  for (u32 d = 0; d < A; ++d) {
    const u32 r = ent_job[d];
    if (s.rj_preempting[r]) s.ent_end[d] = now + 1;
    s.rj_end[r] = std::max<i64>(s.ent_end[d], now + 1);
  }
  for (u32 r = 0; r < R; ++r) s.patched = s.patched || s.rj_preempting[r];
  return s;
}

// ---- the results ----
// The preempting set written out in the order given.  Room for fewer ids than given: the endings of a cycle with preemption enabled
// refuse; the pass-through of a call without (truncate) writes what fits, as it always has.
template <class It>
inline Verdict write_set(const std::string& who, It first, It last, cns_preempt_out* pout, bool truncate = false) {
  pout->num_preempting = 0;
  for (; first != last; ++first) {
    if (pout->num_preempting >= pout->preempting_capacity) return truncate ? Verdict{} : refuse(CNS_ERR_INVALID_ARG, who + ": preempting_capacity too small");
    pout->preempting_job_ids[pout->num_preempting++] = *first;
  }
  return {};
}
// preempt == nullptr or preempt->enabled == 0, behind cns_select: nothing preempted, nothing cancelled, the caller's set as it came
inline void pass_through(const cns_job_soa* jobs, const cns_preempt_soa* pre, cns_preempt_out* pout) {
  if (!pout) return;
  if (pout->offsets && jobs) for (u64 j = 0; j <= jobs->num_jobs; ++j) pout->offsets[j] = 0;
  pout->num_cancelled = 0;
  const u32* ids = pre ? pre->preempting_job_ids : nullptr;
  (void)write_set("", ids, ids + (pre ? pre->num_preempting : 0u), pout, true);
}
// no pending job's QoS may preempt anything, behind the plain cycle: the set without the ids that no longer run, ascending
inline Verdict plain_ending(const std::string& who, u64 J, const std::vector<u32>& set_in, cns_preempt_out* pout) {
  for (u64 j = 0; j <= J; ++j) pout->offsets[j] = 0;
  pout->num_cancelled = 0;
  const std::set<u32> keep(set_in.begin(), set_in.end());
  return write_set(who, keep.begin(), keep.end(), pout);
}

// the job ids of running rows, for a caller that handed no rn_job_id in (cns_running_select_preempt_attrs): ids[k] for rows[k]
using RowIds = std::function<Verdict(const std::vector<u32>& rows, std::vector<u32>& ids)>;

// The device's cnt (pending job, reference) pairs, in push_back order per job (the pairs of different jobs may interleave) -> the CSR by
// job; then m_preempting_set_ / EnqueuePreemptCancel (:6786-6793) in queue order: a preempted running job not yet in the set is cancelled
// and joins it.  cnt above out_cap: the device counted on past its buffer, `pairs` is not read.
inline Verdict fold(const std::string& who, u32 cnt, u32 out_cap, const u32* pairs, u64 J, const cns_preempt_soa* pre, const std::vector<u32>& set_in,
                    const RowIds* row_ids, cns_preempt_out* pout) {
  if (cnt > out_cap) return refuse(CNS_ERR_UNSUPPORTED, who + ": more preemptions than the result buffer holds");
  if (cnt > pout->capacity) return refuse(CNS_ERR_INVALID_ARG, who + ": cns_preempt_out::capacity too small");
  for (u64 j = 0; j <= J; ++j) pout->offsets[j] = 0;
  for (u32 i = 0; i < cnt; ++i) pout->offsets[pairs[2 * i] + 1]++;
  for (u64 j = 0; j < J; ++j) pout->offsets[j + 1] += pout->offsets[j];
  {
    std::vector<u64> cur(pout->offsets, pout->offsets + J);
    for (u32 i = 0; i < cnt; ++i) pout->preempted[cur[pairs[2 * i]]++] = pairs[2 * i + 1];   // append order = push_back order within a job
  }
  std::set<u32> pset(set_in.begin(), set_in.end());
  pout->num_cancelled = 0;
  std::vector<u32> rows, ids;   // the running references in queue order, and (with row_ids) their job ids
  for (u64 x = 0; x < pout->offsets[J]; ++x)
    if (!(pout->preempted[x] & CNS_PREEMPT_REF_PENDING)) rows.push_back(pout->preempted[x]);
  if (row_ids) {
    if (const Verdict v = (*row_ids)(rows, ids)) return v;
  }
  for (size_t k = 0; k < rows.size(); ++k) {
    const u32 id = row_ids ? ids[k] : pre->rn_job_id[rows[k]];
    if (!pset.insert(id).second) continue;
    if (pout->num_cancelled >= pout->cancel_capacity) return refuse(CNS_ERR_INVALID_ARG, who + ": cancel_capacity too small");
    pout->cancelled_job_ids[pout->num_cancelled++] = id;
  }
  return write_set(who, pset.begin(), pset.end(), pout);
}

}  // namespace cns_preempt
