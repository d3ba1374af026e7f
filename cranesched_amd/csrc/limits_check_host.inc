// The input rules of include/crane_gpu/run_limits.h, checked on the host: the tables once (cns_set_run_limits), the keys of a call in one
// pass over the caller's arrays (cns_upload_limit_jobs, before anything is uploaded).  No HIP in here: engine.hip includes it,
// tests/cpp/limits_host_test.cpp compiles it with g++.  What passes here is everything the kernels rely on: every index in range, every
// account chain at most CNS_LIM_MAX_CHAIN long with its levels, no negative max_wall, record ids below 2^32 - 16.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/crane_gpu/run_limits.h"
#include "acct_space_host.inc"

namespace cns_limits_host {

using cns_acct::Verdict;
using cns_acct::refuse;

// *sp: the record space of the tables; *level: every account's depth in the tree (root = 0).
inline Verdict check_tables(const cns_limit_tables* t, cns_acct::Space* sp, std::vector<uint32_t>* level) {
  const uint64_t L = t->num_part_limits;
  if (!t->num_qos || !t->qos) return refuse(CNS_ERR_INVALID_ARG, "cns_set_run_limits: no QoS");
  if (t->num_accounts && !t->acct_parent) return refuse(CNS_ERR_INVALID_ARG, "cns_set_run_limits: acct_parent missing");
  if (L && !t->part_limits) return refuse(CNS_ERR_INVALID_ARG, "cns_set_run_limits: part_limits missing");
  cns_acct::Space S;
  if (!cns_acct::make_space(t->num_users, t->num_user_accts, t->num_accounts, t->num_qos, t->num_partitions, &S) ||
      S.NR >= cns_acct::kMaxRecords || 3 * S.Q + L >= cns_acct::kMaxRecords)
    return refuse(CNS_ERR_UNSUPPORTED, "cns_set_run_limits: more than 2^32 usage records");
  if (const auto f = cns_acct::walk_chains(t->acct_parent, S.A, false, level)) {
    if (f.what == cns_acct::ChainFinding::kParentRange) return refuse(CNS_ERR_INVALID_ARG, "acct_parent out of range");
    return refuse(CNS_ERR_UNSUPPORTED, f.cut_short ? "account chain longer than CNS_LIM_MAX_CHAIN (or a cycle)" : "account chain longer than CNS_LIM_MAX_CHAIN");
  }
  for (uint64_t q = 0; q < S.Q; ++q)
    if (t->qos[q].max_wall_sec < 0) return refuse(CNS_ERR_INVALID_ARG, "negative Qos max_wall");
  for (uint64_t i = 0; i < L; ++i)
    if (t->part_limits[i].max_wall_sec < 0) return refuse(CNS_ERR_INVALID_ARG, "negative partition max_wall");
  for (int w = 1; w <= 3; w += 2) {   // user_part_limit has the shape of table 1, acct_part_limit of table 3
    const uint32_t* tab = w == 1 ? t->user_part_limit : t->acct_part_limit;
    if (!tab) continue;
    for (uint64_t i = 0; i < S.len[w]; ++i)
      if (tab[i] != CNS_LIM_NONE && tab[i] >= L) return refuse(CNS_ERR_INVALID_ARG, "partition limit index out of range");
  }
  *sp = S;
  return {};
}

// The keys of one call.  select_J: jobs of the last cns_select, which select_index (or the job's own position) points into.
inline Verdict check_jobs(const cns_acct::Space& sp, const cns_limit_job_soa* jb, uint64_t select_J) {
  const uint64_t J = jb->num_jobs;
  if (J && (!jb->user || !jb->user_acct || !jb->account || !jb->qos || !jb->partition || !jb->time_limit_sec))
    return refuse(CNS_ERR_INVALID_ARG, "cns_upload_limit_jobs: missing array");
  if (J > cns_acct::kMaxRecords) return refuse(CNS_ERR_UNSUPPORTED, "more than 2^32-16 jobs");
  for (uint64_t i = 0; i < J; ++i) {
    if (jb->skip && jb->skip[i]) continue;
    if (!cns_acct::keys_in_range(sp, jb->user[i], jb->user_acct[i], jb->account[i], jb->qos[i], jb->partition[i], false))
      return refuse(CNS_ERR_INVALID_ARG, "limit job " + std::to_string(i) + ": user / user_acct / account / qos / partition out of range");
    if ((jb->select_index ? jb->select_index[i] : i) >= select_J)
      return refuse(CNS_ERR_INVALID_ARG, "limit job " + std::to_string(i) + ": select_index outside the last cns_select");
  }
  return {};
}

}  // namespace cns_limits_host
