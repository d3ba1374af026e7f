// The input rules of include/crane_gpu_usage/usage.h, checked on the host: the tables once (cns_usage_set_tables), the rows of a call in
// one pass over the caller's arrays (cns_usage_apply, before anything is uploaded).  No HIP in here: engine.hip includes it,
// tests/cpp/usage_host_test.cpp compiles it with g++.  What passes here is everything the kernels rely on: every index in range, every
// account chain at most CNS_LIM_MAX_CHAIN long, every delta component non-negative, at most 2^24 rows, record ids below 2^32 - 16.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/crane_gpu_usage/usage.h"
#include "acct_space_host.inc"

namespace cns_usage_host {

using cns_acct::kMaxRecords;
using cns_acct::Verdict;
using Dims = cns_acct::Space;   // the record space of the tables (acct_space_host.inc)

inline Verdict refuse(const char* call, int code, std::string msg) {
  return cns_acct::refuse(code, std::string(call) + ": " + std::move(msg));
}

inline Verdict check_tables(const cns_usage_tables* t, Dims* dims) {
  const char* C = "cns_usage_set_tables";
  if (t->num_accounts && !t->acct_parent) return refuse(C, CNS_ERR_INVALID_ARG, "missing array: acct_parent");
  if (t->gres.num_classes > CNS_MAX_GRES_CLASSES) return refuse(C, CNS_ERR_INVALID_ARG, "gres.num_classes > 8");
  for (uint32_t g = 0; g < t->gres.num_classes; ++g)
    if (t->gres.class_name[g] >= CNS_MAX_GRES_NAMES) return refuse(C, CNS_ERR_INVALID_ARG, "gres class name id >= 4");
  Dims D;
  if (!cns_acct::make_space(t->num_users, t->num_user_accts, t->num_accounts, t->num_qos, t->num_partitions, &D) || D.NR + D.NE >= kMaxRecords)
    return refuse(C, CNS_ERR_UNSUPPORTED, "more than 2^32 - 16 records");
  if (const auto f = cns_acct::walk_chains(t->acct_parent, D.A, true, nullptr)) {
    const std::string a = std::to_string(f.account);
    if (f.what == cns_acct::ChainFinding::kParentRange) return refuse(C, CNS_ERR_INVALID_ARG, "acct_parent[" + a + "] out of range");
    if (f.what == cns_acct::ChainFinding::kNoEnd) return refuse(C, CNS_ERR_INVALID_ARG, "the chain of account " + a + " does not end");
    return refuse(C, CNS_ERR_UNSUPPORTED, "account " + a + ": a chain of more than 6 accounts");
  }
  const cns_usage* tabs[5] = {t->user_qos, t->user_part, t->acct_qos, t->acct_part, t->qos_usage};
  for (int w = 0; w < 5; ++w)
    if (tabs[w])
      for (uint64_t i = 0; i < D.len[w]; ++i)
        if (tabs[w][i].cpu_raw < 0 || tabs[w][i].wall_sec < 0) return refuse(C, CNS_ERR_INVALID_ARG, "a negative cpu_raw or wall_sec in table " + std::to_string(w));
  *dims = D;
  return {};
}

// The rows of one call.  *applied: rows that are not skipped.
inline Verdict check_jobs(const Dims& D, const cns_usage_jobs* jb, const cns_usage_out* out, uint32_t op, uint64_t* applied) {
  const char* C = "cns_usage_apply";
  const uint64_t J = jb->num_jobs;
  if (J > CNS_USAGE_MAX_JOBS) return refuse(C, CNS_ERR_UNSUPPORTED, "more than 2^24 jobs in one call");
  if (op != CNS_USAGE_RELEASE && op != CNS_USAGE_CHARGE) return refuse(C, CNS_ERR_INVALID_ARG, "unknown op");
  if (!jb->user || !jb->user_acct || !jb->account || !jb->qos || !jb->partition) return refuse(C, CNS_ERR_INVALID_ARG, "missing key array");
  if (!out || !out->not_found || !out->over_free) return refuse(C, CNS_ERR_INVALID_ARG, "missing result array");
  uint64_t n = 0;
  for (uint64_t j = 0; j < J; ++j) {
    if (jb->skip && jb->skip[j]) continue;
    const std::string row = "job " + std::to_string(j) + ": ";
    if (!cns_acct::keys_in_range(D, jb->user[j], jb->user_acct[j], jb->account[j], jb->qos[j], jb->partition[j], true))
      return refuse(C, CNS_ERR_INVALID_ARG, row + "a key index out of range");
    if (op == CNS_USAGE_CHARGE && jb->user_acct[j] == CNS_LIM_NONE) return refuse(C, CNS_ERR_INVALID_ARG, row + "a charge without a user_acct");
    if ((jb->cpu_raw && jb->cpu_raw[j] < 0) || (jb->wall_sec && jb->wall_sec[j] < 0)) return refuse(C, CNS_ERR_INVALID_ARG, row + "a negative cpu_raw or wall_sec");
    bool any = (jb->cpu_raw && jb->cpu_raw[j]) || (jb->mem && jb->mem[j]) || (jb->wall_sec && jb->wall_sec[j]) || (jb->jobs_count && jb->jobs_count[j]) ||
               (jb->submit_count && jb->submit_count[j]);
    if (jb->name_total)
      for (uint32_t n4 = 0; n4 < CNS_MAX_GRES_NAMES; ++n4) any = any || jb->name_total[j * CNS_MAX_GRES_NAMES + n4];
    if (jb->class_count)
      for (uint32_t g = 0; g < CNS_MAX_GRES_CLASSES; ++g) any = any || jb->class_count[j * CNS_MAX_GRES_CLASSES + g];
    if (!any) return refuse(C, CNS_ERR_INVALID_ARG, row + "a delta that is all zero");
    ++n;
  }
  if (applied) *applied = n;
  return {};
}

}  // namespace cns_usage_host
