// Host pass of cns_schedule_steps (include/crane_gpu/steps.h): every argument check and the re-layout of the caller's arrays
// (SoA -> one StepRec per step, one Res per (job, node)), before anything goes to the device.  Pure arithmetic on the ABI structs:
// no HIP, no handle, no error string but the one pack() returns.  What passes here is what k_sched_steps may index without a bound
// check of its own: offsets that start at 0, never decrease and end at their array's length, include / exclude ranges inside the
// staged lists, at most CNS_STEP_MAX_NODES heap entries and at most CNS_STEP_MAX_TASKS_PER_NODE turns of the per-node task loop.
// steps_call.inc uploads the result and launches; tests/cpp/steps_host_test.cpp compiles this file with g++ and holds it to
// hand-written records and to one input per refusal (tests/test_steps_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/crane_gpu/steps.h"
#include "csr_host.inc"
#include "res_dev.h"

namespace cns_steps {

using cns::Req;
using cns::Res;
using cns::u32;
using cns::u64;

struct StepRec {
  Req node_req, task_req;      // req_node_res_view, req_task_res_view
  u32 node_num, ntasks, tmin, tmax;
  u32 incl_b, incl_e, excl_b, excl_e;
  u64 place_off, task_off;
};

struct Status {
  int code = 0;                // CNS_OK or a cns_status
  std::string msg;
  explicit operator bool() const { return code != 0; }
};

struct Packed {
  std::vector<StepRec> recs;   // [max(S, 1)]
  std::vector<Res> avail;      // [max(num_nodes, 1)] step_res_avail_ of every (job, node)
  u64 places = 0, tasks = 0;   // sum node_num, sum ntasks: the result records
  u32 n_incl = 0, n_excl = 0;  // entries of the include / exclude lists (the last offset)
};

// num_classes: the GRES classes the handle's layout defines (cns_set_nodes).  Fills out->place_offsets / task_offsets.
inline Status pack(u32 num_classes, const cns_step_job_soa* jb, const cns_step_soa* st, cns_step_result_soa* out, Packed& P) {
  auto bad = [](int code, std::string msg) { return Status{code, std::move(msg)}; };
  if (!jb || !st || !out) return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: null argument");
  const u32 Jn = jb->num_jobs, S = st->num_steps, Nn = jb->num_nodes;
  if (Jn && (!jb->node_offsets || !jb->step_offsets)) return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing job offsets");
  if (Nn && (!jb->node_idx || !jb->avail_cpu_raw || !jb->avail_mem || !jb->avail_core_lo))
    return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing node array");
  if (S && (!st->task_cpu_raw || !st->task_mem || !st->node_num || !st->ntasks || !st->ntasks_per_node_min || !st->ntasks_per_node_max))
    return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing step array");
  if (!out->scheduled || !out->place_offsets || !out->task_offsets) return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing result array");
  // a CSR [n + 1] that starts at 0, never decreases and (end known) ends at `end`; NULL is an empty one
  auto csr = [&](const u32* off, u32 n, const u64* end, const char* name) -> Status {
    if (!off) return (end && *end) ? bad(CNS_ERR_INVALID_ARG, std::string("cns_schedule_steps: ") + name + " do not cover the node / step arrays") : Status{};
    const cns_csr::OffsetsVerdict v = cns_csr::check_offsets(off, n);
    if (v.what == cns_csr::Offsets::FirstNot0) return bad(CNS_ERR_INVALID_ARG, std::string("cns_schedule_steps: ") + name + " do not start at 0");
    if (v.what == cns_csr::Offsets::Decreases) return bad(CNS_ERR_INVALID_ARG, std::string("cns_schedule_steps: ") + name + " decrease after entry " + std::to_string(v.index));
    if (end && off[n] != *end) return bad(CNS_ERR_INVALID_ARG, std::string("cns_schedule_steps: ") + name + " do not cover the node / step arrays");
    return Status{};
  };
  const u64 end_n = Nn, end_s = S;
  if (Status s = csr(jb->node_offsets, Jn, &end_n, "node_offsets")) return s;
  if (Status s = csr(jb->step_offsets, Jn, &end_s, "step_offsets")) return s;
  if (Status s = csr(st->incl_offsets, S, nullptr, "incl_offsets")) return s;
  if (Status s = csr(st->excl_offsets, S, nullptr, "excl_offsets")) return s;
  P.n_incl = st->incl_offsets ? st->incl_offsets[S] : 0;
  P.n_excl = st->excl_offsets ? st->excl_offsets[S] : 0;
  if ((P.n_incl && !st->incl_nodes) || (P.n_excl && !st->excl_nodes)) return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: include / exclude offsets without node lists");
  P.recs.assign(std::max<u32>(S, 1), StepRec{});
  P.places = P.tasks = 0;
  auto pack_req = [&](Req& q, const int64_t* cpu, const uint64_t* mem, const uint8_t* gt, const uint8_t* gs, u32 s) -> bool {
    q.cpu = cpu ? cpu[s] : 0; q.mem = mem ? mem[s] : 0; q.gtot = 0; q.gspec = 0;
    if (gt) memcpy(&q.gtot, gt + (size_t)s * CNS_MAX_GRES_NAMES, 4);
    if (gs) memcpy(&q.gspec, gs + (size_t)s * CNS_MAX_GRES_CLASSES, 8);
    for (u32 c = num_classes; c < CNS_MAX_GRES_CLASSES; ++c)
      if ((q.gspec >> (8 * c)) & 0xFF) return false;
    return q.cpu >= 0;
  };
  for (u32 s = 0; s < S; ++s) {
    StepRec& r = P.recs[s];
    if (!pack_req(r.node_req, st->node_cpu_raw, st->node_mem, st->node_gres_total, st->node_gres_spec, s) ||
        !pack_req(r.task_req, st->task_cpu_raw, st->task_mem, st->task_gres_total, st->task_gres_spec, s))
      return bad(CNS_ERR_INVALID_ARG, "step " + std::to_string(s) + ": negative cpu or undefined GRES class");
    r.node_num = st->node_num[s]; r.ntasks = st->ntasks[s]; r.tmin = st->ntasks_per_node_min[s]; r.tmax = st->ntasks_per_node_max[s];
    if (r.node_num == 0 || r.ntasks < r.node_num || r.tmin == 0 || r.tmax < r.tmin)
      return bad(CNS_ERR_INVALID_ARG, "step " + std::to_string(s) + ": invalid node_num / ntasks / ntasks_per_node");
    if (r.node_num > CNS_STEP_MAX_NODES) return bad(CNS_ERR_UNSUPPORTED, "step " + std::to_string(s) + ": more than CNS_STEP_MAX_NODES nodes");
    // the per-node task loop of the kernel stops at tmax or at the first task that does not fit; a task that asks for nothing
    // always fits, so tmax is the one bound that holds for every request
    if (r.tmax > CNS_STEP_MAX_TASKS_PER_NODE)
      return bad(CNS_ERR_UNSUPPORTED, "step " + std::to_string(s) + ": ntasks_per_node_max above CNS_STEP_MAX_TASKS_PER_NODE");
    r.incl_b = st->incl_offsets ? st->incl_offsets[s] : 0; r.incl_e = st->incl_offsets ? st->incl_offsets[s + 1] : 0;
    r.excl_b = st->excl_offsets ? st->excl_offsets[s] : 0; r.excl_e = st->excl_offsets ? st->excl_offsets[s + 1] : 0;
    r.place_off = P.places; r.task_off = P.tasks;
    out->place_offsets[s] = P.places; out->task_offsets[s] = P.tasks;
    P.places += r.node_num; P.tasks += r.ntasks;
  }
  out->place_offsets[S] = P.places; out->task_offsets[S] = P.tasks;
  if (P.places && (!out->node_idx || !out->node_ntasks || !out->node_cpu_raw || !out->node_mem || !out->node_core_lo || !out->node_core_hi || !out->node_gres))
    return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing node result array");
  if (P.tasks && (!out->task_node || !out->task_cpu_raw || !out->task_mem || !out->task_core_lo || !out->task_core_hi || !out->task_gres))
    return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing task result array");
  if (Nn && (!out->avail_cpu_raw || !out->avail_mem || !out->avail_core_lo || !out->avail_core_hi || !out->avail_gres))
    return bad(CNS_ERR_INVALID_ARG, "cns_schedule_steps: missing availability result array");
  P.avail.assign(std::max<u32>(Nn, 1), Res{});
  for (u32 n = 0; n < Nn; ++n) {
    Res& a = P.avail[n];
    a.cpu = jb->avail_cpu_raw[n]; a.mem = jb->avail_mem[n]; a.clo = jb->avail_core_lo[n];
    a.chi = jb->avail_core_hi ? jb->avail_core_hi[n] : 0; a.gres = jb->avail_gres ? jb->avail_gres[n] : 0;
    a.c2 = jb->avail_core_w2 ? jb->avail_core_w2[n] : 0; a.c3 = jb->avail_core_w3 ? jb->avail_core_w3[n] : 0;
  }
  return Status{};
}

}  // namespace cns_steps
