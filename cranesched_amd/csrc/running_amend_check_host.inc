// The input rules of include/crane_gpu_amend/running_amend.h, checked on the host before anything is uploaded: a ledger to amend, the
// arrays, the size the kernels' 32-bit indices hold, distinct ids; the amend ids sorted here (the device bisects them) with the origin
// of each, as check_step does for retire ids, and the new ends carried along.  No HIP in here: engine.hip includes it
// (running_amend_host.inc calls it first), tests/cpp/running_amend_host_test.cpp compiles it with g++.
#pragma once
#include "running_check_host.inc"

#include "../../include/crane_gpu_amend/running_amend.h"

namespace cns_running {

// cns_running_amend_ends.  have_ledger: a cns_running_seed succeeded and no cns_set_running / change of num_nodes dropped it.
// *sorted_ids: the amend ids ascending; *sorted_ends: their new ends; *order: sorted position -> position in job_ids.
inline Verdict check_amend(bool have_ledger, const cns_running_amend* in, const cns_running_amend_out* out, std::vector<uint32_t>* sorted_ids,
                           std::vector<int64_t>* sorted_ends, std::vector<uint32_t>* order) {
  sorted_ids->clear(); sorted_ends->clear(); order->clear();
  if (!have_ledger) return refuse(CNS_ERR_STATE, "cns_running_amend_ends before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)");
  const uint64_t K = in->num_amend;
  if (K > kMaxAllocs) return refuse(CNS_ERR_UNSUPPORTED, "cns_running_amend_ends: more than 2^32 - 256 amendments");
  if (!K) return {};
  if (!in->job_ids) return refuse(CNS_ERR_INVALID_ARG, "cns_running_amend_ends: missing array: job_ids");
  if (!in->end_sec) return refuse(CNS_ERR_INVALID_ARG, "cns_running_amend_ends: missing array: end_sec");
  if (!out || !out->found) return refuse(CNS_ERR_INVALID_ARG, "cns_running_amend_ends: missing array: out->found");
  order->resize(K);
  for (uint64_t i = 0; i < K; ++i) (*order)[i] = (uint32_t)i;
  std::sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) { return in->job_ids[a] < in->job_ids[b]; });
  sorted_ids->resize(K); sorted_ends->resize(K);
  for (uint64_t i = 0; i < K; ++i) {
    (*sorted_ids)[i] = in->job_ids[(*order)[i]];
    (*sorted_ends)[i] = in->end_sec[(*order)[i]];
  }
  uint32_t twice = 0;
  if (first_repeat(*sorted_ids, &twice)) return refuse(CNS_ERR_INVALID_ARG, "cns_running_amend_ends: job id " + std::to_string(twice) + " stands twice in job_ids");
  return {};
}

}  // namespace cns_running
