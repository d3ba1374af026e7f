// cranesched_amd/csrc/running_preempt_check_host.inc (the input rules of cns_running_select_preempt, and of the admit step behind it)
// compiled with g++ and driven over hand cases: a valid call, then every rule of include/crane_gpu_running/running_preempt.h broken
// in turn.  Prints "<case>: <status> <message>" per case, so that tests/test_running_preempt_host.py can hold every refusal to its
// message; built once plain and once with -fsanitize=address,undefined: every array below is exactly as long as the header says.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../cranesched_amd/csrc/running_preempt_check_host.inc"

namespace {

struct Call {   // two pending jobs, three ledger rows, two QoS
  std::vector<uint32_t> qoff{0, 0, 1}, qp{0}, pd_id{1, 2}, pd_qos{1, 0}, pd_qprio{20, 10}, rn_id{7, 3, 9}, rn_qos{0, 0, 1}, rn_qprio{10, 10, 20}, set{9, 4, 9, 3};
  std::vector<double> pd_prio{1.5, 0.5};
  std::vector<int64_t> rn_start{10, 20, 30};
  std::vector<uint64_t> offsets = std::vector<uint64_t>(3);
  std::vector<uint32_t> preempted = std::vector<uint32_t>(8), cancelled = std::vector<uint32_t>(3), preempting = std::vector<uint32_t>(6);
  cns_job_soa jobs{};
  cns_preempt_soa pre{};
  cns_placement_soa out{};
  cns_preempt_out pout{};
  cns_running::PreemptFacts F;
  void bind() {
    jobs.num_jobs = 2;
    pre.enabled = 1; pre.num_qos = 2; pre.qos_preempt_offsets = qoff.data(); pre.qos_preempt = qp.data();
    pre.pd_job_id = pd_id.data(); pre.pd_qos = pd_qos.data(); pre.pd_qos_priority = pd_qprio.data(); pre.pd_priority = pd_prio.data();
    pre.rn_job_id = rn_id.data(); pre.rn_qos = rn_qos.data(); pre.rn_qos_priority = rn_qprio.data(); pre.rn_start_sec = rn_start.data();
    pre.num_preempting = (uint32_t)set.size(); pre.preempting_job_ids = set.data();
    pout.capacity = preempted.size(); pout.offsets = offsets.data(); pout.preempted = preempted.data();
    pout.cancel_capacity = (uint32_t)cancelled.size(); pout.cancelled_job_ids = cancelled.data();
    pout.preempting_capacity = (uint32_t)preempting.size(); pout.preempting_job_ids = preempting.data();
    F.have_nodes = F.have_ledger = F.tables_are_ledgers = true; F.ledger_jobs = 3;
  }
};

int g_fail = 0;

void call(const char* name, const std::function<void(Call&)>& edit, int null_arg = 0) {
  Call c;
  c.bind();
  edit(c);
  const cns_running::Verdict v = cns_running::check_select_preempt(c.F, null_arg == 1 ? nullptr : &c.jobs, null_arg == 2 ? nullptr : &c.pre, null_arg == 3 ? nullptr : &c.out,
                                                                   null_arg == 4 ? nullptr : &c.pout);
  printf("%s: %d %s", name, v.code, v.msg.c_str());
  if (!v) {
    printf("set=");
    for (uint32_t x : cns_running::preempting_sorted(c.pre.preempting_job_ids, c.pre.num_preempting)) printf("%u,", x);
  }
  printf("\n");
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

void admit(const char* name, bool resident_preempt_cycle, uint64_t num_jobs, bool mask) {
  std::vector<uint8_t> m(num_jobs, 1);
  std::vector<uint32_t> ids(num_jobs, 5);
  cns_running_step in{};
  in.num_jobs = num_jobs; in.job_id = ids.data(); in.admit = mask ? m.data() : nullptr;
  const cns_running::Verdict v = cns_running::check_step_after_preempt(resident_preempt_cycle, &in);
  printf("%s: %d %s\n", name, v.code, v.msg.c_str());
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

}  // namespace

int main() {
  call("call_valid", [](Call&) {});
  call("call_no_jobs_arg", [](Call&) {}, 1);
  call("call_no_preempt_arg", [](Call&) {}, 2);
  call("call_no_out_arg", [](Call&) {}, 3);
  call("call_no_pout_arg", [](Call&) {}, 4);
  call("call_no_nodes", [](Call& c) { c.F.have_nodes = false; });
  call("call_no_ledger", [](Call& c) { c.F.have_ledger = false; });
  call("call_tables_not_the_ledgers", [](Call& c) { c.F.tables_are_ledgers = false; });
  call("call_too_many_pending", [](Call& c) { c.jobs.num_jobs = 0x80000000ull; });
  call("call_pending_at_the_limit", [](Call& c) { c.jobs.num_jobs = 0x7FFFFFFFull; });
  call("call_too_many_rows", [](Call& c) { c.F.ledger_jobs = 0x80000000ull; });
  call("call_no_pd_qos", [](Call& c) { c.pre.pd_qos = nullptr; });
  call("call_no_pd_qos_priority", [](Call& c) { c.pre.pd_qos_priority = nullptr; });
  call("call_no_pd_priority", [](Call& c) { c.pre.pd_priority = nullptr; });
  call("call_empty_queue_needs_no_pending_array", [](Call& c) { c.jobs.num_jobs = 0; c.pre.pd_qos = nullptr; c.pre.pd_qos_priority = nullptr; c.pre.pd_priority = nullptr; });
  call("call_no_rn_job_id", [](Call& c) { c.pre.rn_job_id = nullptr; });
  call("call_no_rn_qos", [](Call& c) { c.pre.rn_qos = nullptr; });
  call("call_no_rn_qos_priority", [](Call& c) { c.pre.rn_qos_priority = nullptr; });
  call("call_no_rn_start", [](Call& c) { c.pre.rn_start_sec = nullptr; });
  call("call_empty_ledger_needs_no_running_array", [](Call& c) { c.F.ledger_jobs = 0; c.pre.rn_job_id = nullptr; c.pre.rn_qos = nullptr; c.pre.rn_qos_priority = nullptr; c.pre.rn_start_sec = nullptr; });
  call("call_no_qos_offsets", [](Call& c) { c.pre.qos_preempt_offsets = nullptr; });
  call("call_no_qos_lists", [](Call& c) { c.pre.qos_preempt = nullptr; });
  call("call_empty_qos_lists_need_no_array", [](Call& c) { c.qoff = {0, 0, 0}; c.pre.qos_preempt_offsets = c.qoff.data(); c.pre.qos_preempt = nullptr; });
  call("call_no_set", [](Call& c) { c.pre.preempting_job_ids = nullptr; });
  call("call_empty_set", [](Call& c) { c.pre.num_preempting = 0; c.pre.preempting_job_ids = nullptr; });
  call("call_no_offsets_out", [](Call& c) { c.pout.offsets = nullptr; });
  call("call_no_preempted_out", [](Call& c) { c.pout.preempted = nullptr; });
  call("call_no_cancelled_out", [](Call& c) { c.pout.cancelled_job_ids = nullptr; });
  call("call_no_preempting_out", [](Call& c) { c.pout.preempting_job_ids = nullptr; });
  {
    const cns_running::Verdict v = cns_running::refuse_row_id(2, 9, 8);
    printf("row_id: %d %s\n", v.code, v.msg.c_str());
  }
  admit("admit_mask_given", true, 4, true);
  admit("admit_no_mask", true, 4, false);
  admit("admit_no_mask_no_admit_step", true, 0, false);
  admit("admit_no_mask_after_a_plain_cycle", false, 4, false);
  return g_fail ? 1 : 0;
}
