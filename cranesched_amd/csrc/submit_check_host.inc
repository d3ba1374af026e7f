// The input rules of include/crane_gpu_submit/submit_limits.h, checked on the host: the tables once (cns_set_submit_limits), the keys of
// a call and the rule on the 32-bit counts in one pass over the caller's arrays (cns_check_submissions, before anything is uploaded).
// No HIP in here: engine.hip includes it, tests/cpp/submit_host_test.cpp compiles it with g++.  What passes here is everything the
// kernels rely on: every index in range, every account chain at most CNS_LIM_MAX_CHAIN long, no count sum beyond UINT32_MAX, record
// ids below 2^32 - 16.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/crane_gpu_submit/submit_limits.h"
#include "acct_space_host.inc"

namespace cns_submit_host {

using cns_acct::Verdict;
using cns_acct::refuse;

inline Verdict check_tables(const cns_submit_tables* t, cns_acct::Space* sp) {
  const uint64_t L = t->num_part_limits;
  if ((t->num_qos && !t->qos) || (t->num_accounts && !t->acct_parent) || (L && !t->part_limits)) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: missing table");
  if (t->gres.num_classes > CNS_MAX_GRES_CLASSES) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: gres.num_classes > 8");
  for (uint32_t g = 0; g < t->gres.num_classes; ++g)
    if (t->gres.class_name[g] >= CNS_MAX_GRES_NAMES) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: gres class name id >= 4");
  cns_acct::Space S;
  if (!cns_acct::make_space(t->num_users, t->num_user_accts, t->num_accounts, t->num_qos, t->num_partitions, &S) || S.NR + S.NE >= cns_acct::kMaxRecords)
    return refuse(CNS_ERR_UNSUPPORTED, "cns_set_submit_limits: more than 2^32 - 16 records");
  if (const auto f = cns_acct::walk_chains(t->acct_parent, S.A, true, nullptr)) {
    const std::string a = std::to_string(f.account);
    if (f.what == cns_acct::ChainFinding::kParentRange) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: acct_parent out of range");
    if (f.what == cns_acct::ChainFinding::kNoEnd) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: the chain of account " + a + " does not end");
    return refuse(CNS_ERR_UNSUPPORTED, "cns_set_submit_limits: account " + a + ": a chain of more than 6 accounts");
  }
  for (int w = 1; w <= 3; w += 2) {   // user_part_limit has the shape of table 1, acct_part_limit of table 3
    const uint32_t* m = w == 1 ? t->user_part_limit : t->acct_part_limit;
    if (m)
      for (uint64_t i = 0; i < S.len[w]; ++i)
        if (m[i] != CNS_LIM_NONE && m[i] >= L) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: partition limit index out of range");
  }
  const cns_usage* tabs[5] = {t->user_qos, t->user_part, t->acct_qos, t->acct_part, t->qos_usage};
  for (int w = 0; w < 5; ++w)
    if (tabs[w])
      for (uint64_t i = 0; i < S.len[w]; ++i)
        if (tabs[w][i].jobs_count == 0xFFFFFFFFu) return refuse(CNS_ERR_INVALID_ARG, "cns_set_submit_limits: a jobs_count of UINT32_MAX");
  *sp = S;
  return {};
}

// The jobs of one call.  max_set / max_cur: the largest submit count of the tables as set / as the last call left them; the call starts
// from the second under CNS_SUBMIT_CARRY.
inline Verdict check_jobs(const cns_acct::Space& sp, const cns_job_soa* jb, const cns_submit_keys* ky, const cns_submit_out* out, uint32_t flags,
                          uint32_t max_set, uint32_t max_cur) {
  if (!jb->partition || !jb->time_limit_sec || !jb->node_mem || !jb->task_cpu_raw || !jb->task_mem || !jb->node_num || !jb->ntasks)
    return refuse(CNS_ERR_INVALID_ARG, "cns_check_submissions: missing job array");
  if (!ky->user || !ky->user_acct || !ky->account || !ky->qos || !ky->count) return refuse(CNS_ERR_INVALID_ARG, "cns_check_submissions: missing key array");
  if (!out->code || !out->time_limit_out) return refuse(CNS_ERR_INVALID_ARG, "cns_check_submissions: missing result array");
  const uint32_t J = (uint32_t)jb->num_jobs;
  uint64_t total = 0;
  for (uint32_t j = 0; j < J; ++j) {
    if (ky->skip && ky->skip[j]) continue;
    if (!cns_acct::keys_in_range(sp, ky->user[j], ky->user_acct[j], ky->account[j], ky->qos[j], jb->partition[j], true))
      return refuse(CNS_ERR_INVALID_ARG, "cns_check_submissions: job " + std::to_string(j) + ": a key index out of range");
    total += ky->count[j];
  }
  if ((uint64_t)((flags & CNS_SUBMIT_CARRY) ? max_cur : max_set) + total > 0xFFFFFFFFull)
    return refuse(CNS_ERR_UNSUPPORTED, "cns_check_submissions: the largest submit count + the sum of count over the call exceeds UINT32_MAX");
  return {};
}

}  // namespace cns_submit_host
