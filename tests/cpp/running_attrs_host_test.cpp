// cranesched_amd/csrc/running_attrs_check_host.inc (the input rules of the calls of include/crane_gpu_running/running_attrs.h)
// compiled with g++ and driven over hand cases: a valid call, then every rule broken in turn, and the two refusals that start from a
// device flag word.  Prints "<case>: <status> <message>" per case, so that tests/test_running_attrs_host.py can hold every refusal to
// its message; built once plain and once with -fsanitize=address,undefined: every array below is exactly as long as the header says.
#include <cstdio>
#include <functional>
#include <vector>

#include "../../cranesched_amd/csrc/running_attrs_check_host.inc"

namespace {

int g_fail = 0;

void show(const char* name, const cns_running::Verdict& v) {
  printf("%s: %d %s\n", name, v.code, v.msg.c_str());
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

struct Attrs {   // three rows / three queue jobs
  std::vector<int64_t> start{10, 20, 30};
  std::vector<uint32_t> qos{0, 1, 0}, qprio{10, 20, 10}, part{1, 1, 5}, account{2, 0, 1};
  cns_running_attrs a{};
  Attrs() { a.start_sec = start.data(); a.qos = qos.data(); a.qos_priority = qprio.data(); a.partition_priority = part.data(); a.account = account.data(); }
};

void seed(const char* name, uint64_t jobs, const std::function<void(Attrs&)>& edit, bool null_attrs = false) {
  Attrs t;
  edit(t);
  show(name, cns_running::check_seed_attrs(jobs, null_attrs ? nullptr : &t.a));
}

void step(const char* name, bool columns, uint64_t num_jobs, const std::function<void(Attrs&)>& edit, bool null_attrs = false) {
  Attrs t;
  edit(t);
  cns_running_step in{};
  in.num_jobs = num_jobs;
  show(name, cns_running::check_step_attrs(columns, &in, null_attrs ? nullptr : &t.a));
}

struct Pending {   // two pending jobs, three accounts
  std::vector<int64_t> submit{5, 6}, cpu{256, 512};
  std::vector<uint32_t> qos{1, 2}, part{1, 1}, nodes{1, 2}, account{0, 2}, order = std::vector<uint32_t>(2);
  std::vector<uint64_t> mem{7, 8};
  std::vector<double> prio = std::vector<double>(2);
  cns_priority_config cfg{};
  cns_prio_pending_soa pd{};
  uint64_t n = 0;
  Pending() {
    pd.num_jobs = 2; pd.submit_sec = submit.data(); pd.qos_priority = qos.data(); pd.partition_priority = part.data(); pd.node_num = nodes.data();
    pd.total_cpu_raw = cpu.data(); pd.total_mem = mem.data(); pd.account = account.data();
  }
};

void order(const char* name, bool ledger, bool columns, uint32_t accounts, const std::function<void(Pending&)>& edit, int null_arg = 0) {
  Pending p;
  edit(p);
  cns_running::Verdict v = cns_running::check_order_resident(ledger, columns, null_arg == 1 ? nullptr : &p.cfg, null_arg == 2 ? nullptr : &p.pd, null_arg == 4 ? nullptr : p.order.data(),
                                                             null_arg == 5 ? nullptr : p.prio.data(), null_arg == 3 ? nullptr : &p.n);
  if (!v && null_arg == 0) v = cns_running::check_order_pending(&p.pd, accounts);
  show(name, v);
}

void get(const char* name, bool ledger, bool columns, uint64_t capacity, uint64_t rows, bool arrays, bool null_arg = false) {
  std::vector<uint32_t> qos(capacity ? capacity : 1);
  uint64_t n = 0;
  cns_running_attrs_out o{};
  o.capacity_jobs = capacity; o.num_jobs = &n; o.qos = arrays ? qos.data() : nullptr;
  show(name, cns_running::check_get_attrs(ledger, columns, null_arg ? nullptr : &o, rows));
}

struct Call {   // two pending jobs, three ledger rows, two QoS: running_preempt_host_test.cpp's call without the running-job arrays
  std::vector<uint32_t> qoff{0, 0, 1}, qp{0}, pd_id{1, 2}, pd_qos{1, 0}, pd_qprio{20, 10}, set{9, 4}, rn{7, 3, 9};
  std::vector<double> pd_prio{1.5, 0.5};
  std::vector<int64_t> rn_start{10, 20, 30};
  std::vector<uint64_t> offsets = std::vector<uint64_t>(3);
  std::vector<uint32_t> preempted = std::vector<uint32_t>(8), cancelled = std::vector<uint32_t>(3), preempting = std::vector<uint32_t>(6);
  cns_job_soa jobs{};
  cns_preempt_soa pre{};
  cns_placement_soa out{};
  cns_preempt_out pout{};
  cns_running::PreemptFacts F;
  bool columns = true;
  Call() {
    jobs.num_jobs = 2;
    pre.enabled = 1; pre.num_qos = 2; pre.qos_preempt_offsets = qoff.data(); pre.qos_preempt = qp.data();
    pre.pd_job_id = pd_id.data(); pre.pd_qos = pd_qos.data(); pre.pd_qos_priority = pd_qprio.data(); pre.pd_priority = pd_prio.data();
    pre.num_preempting = (uint32_t)set.size(); pre.preempting_job_ids = set.data();
    pout.capacity = preempted.size(); pout.offsets = offsets.data(); pout.preempted = preempted.data();
    pout.cancel_capacity = (uint32_t)cancelled.size(); pout.cancelled_job_ids = cancelled.data();
    pout.preempting_capacity = (uint32_t)preempting.size(); pout.preempting_job_ids = preempting.data();
    F.have_nodes = F.have_ledger = F.tables_are_ledgers = true; F.ledger_jobs = 3;
  }
};

void call(const char* name, const std::function<void(Call&)>& edit, int null_arg = 0) {
  Call c;
  edit(c);
  show(name, cns_running::check_select_preempt_attrs(c.F, c.columns, null_arg == 1 ? nullptr : &c.jobs, null_arg == 2 ? nullptr : &c.pre, null_arg == 3 ? nullptr : &c.out,
                                                     null_arg == 4 ? nullptr : &c.pout));
}

void worst(const char* name, uint32_t account_row, uint32_t negative_row, uint32_t range_row) {
  uint32_t row = 0;
  const int kind = cns_running::worst_row(account_row, negative_row, range_row, &row);
  printf("%s: %d row=%u\n", name, kind, row);
}

}  // namespace

int main() {
  const auto none = [](auto&) {};
  seed("seed_valid", 3, none);
  seed("seed_empty_set_needs_no_attrs", 0, none, true);
  seed("seed_no_attrs", 3, none, true);
  seed("seed_no_start", 3, [](Attrs& t) { t.a.start_sec = nullptr; });
  seed("seed_no_qos", 3, [](Attrs& t) { t.a.qos = nullptr; });
  seed("seed_no_qos_priority", 3, [](Attrs& t) { t.a.qos_priority = nullptr; });
  seed("seed_no_partition_priority", 3, [](Attrs& t) { t.a.partition_priority = nullptr; });
  seed("seed_no_account", 3, [](Attrs& t) { t.a.account = nullptr; });

  step("step_valid", true, 3, none);
  step("step_start_is_not_read", true, 3, [](Attrs& t) { t.a.start_sec = nullptr; });
  step("step_no_admit_step_needs_no_attrs", true, 0, none, true);
  step("step_no_columns", false, 0, none, true);
  step("step_no_attrs", true, 3, none, true);
  step("step_no_qos", true, 3, [](Attrs& t) { t.a.qos = nullptr; });
  step("step_no_qos_priority", true, 3, [](Attrs& t) { t.a.qos_priority = nullptr; });
  step("step_no_partition_priority", true, 3, [](Attrs& t) { t.a.partition_priority = nullptr; });
  step("step_no_account", true, 3, [](Attrs& t) { t.a.account = nullptr; });

  get("get_valid", true, true, 3, 3, true);
  get("get_sizes_only", true, true, 0, 3, false);
  get("get_null", true, true, 3, 3, true, true);
  get("get_no_ledger", false, false, 3, 3, true);
  get("get_no_columns", true, false, 3, 3, true);
  get("get_too_small", true, true, 2, 3, true);

  order("order_valid", true, true, 3, none);
  order("order_no_cfg", true, true, 3, none, 1);
  order("order_no_pending", true, true, 3, none, 2);
  order("order_no_num_ordered", true, true, 3, none, 3);
  order("order_no_order_out", true, true, 3, none, 4);
  order("order_no_priority_out", true, true, 3, none, 5);
  order("order_no_submit", true, true, 3, [](Pending& p) { p.pd.submit_sec = nullptr; });
  order("order_no_pending_account", true, true, 3, [](Pending& p) { p.pd.account = nullptr; });
  order("order_empty_queue_needs_no_array", true, true, 3, [](Pending& p) { p.pd = cns_prio_pending_soa{}; }, 4);
  order("order_no_ledger", false, false, 3, none);
  order("order_no_columns", true, false, 3, none);
  order("order_pending_account", true, true, 2, none);
  order("order_pending_negative_cpu", true, true, 3, [](Pending& p) { p.cpu[1] = -1; });

  worst("worst_none", cns_running::kNoRow, cns_running::kNoRow, cns_running::kNoRow);
  worst("worst_account_least", 2, 5, 9);
  worst("worst_range_least", 7, 5, 3);
  worst("worst_negative_least", 7, 1, 3);
  worst("worst_account_before_range_on_one_row", 4, cns_running::kNoRow, 4);
  show("row_account", cns_running::refuse_account_row(5, 64, 64));
  show("row_negative", cns_running::refuse_sum_row(9, cns_running::kRowCpuNegative));
  show("row_range", cns_running::refuse_sum_row(0, cns_running::kRowSumRange));

  call("call_valid", none);
  call("call_no_jobs_arg", none, 1);
  call("call_no_preempt_arg", none, 2);
  call("call_no_out_arg", none, 3);
  call("call_no_pout_arg", none, 4);
  call("call_no_nodes", [](Call& c) { c.F.have_nodes = false; });
  call("call_no_ledger", [](Call& c) { c.F.have_ledger = false; });
  call("call_no_columns", [](Call& c) { c.columns = false; });
  call("call_tables_not_the_ledgers", [](Call& c) { c.F.tables_are_ledgers = false; });
  call("call_too_many_pending", [](Call& c) { c.jobs.num_jobs = 0x80000000ull; });
  call("call_too_many_rows", [](Call& c) { c.F.ledger_jobs = 0x80000000ull; });
  call("call_rn_job_id_given", [](Call& c) { c.pre.rn_job_id = c.rn.data(); });
  call("call_rn_qos_given", [](Call& c) { c.pre.rn_qos = c.rn.data(); });
  call("call_rn_qos_priority_given", [](Call& c) { c.pre.rn_qos_priority = c.rn.data(); });
  call("call_rn_start_given", [](Call& c) { c.pre.rn_start_sec = c.rn_start.data(); });
  call("call_no_pd_qos", [](Call& c) { c.pre.pd_qos = nullptr; });
  call("call_no_qos_offsets", [](Call& c) { c.pre.qos_preempt_offsets = nullptr; });
  call("call_no_set", [](Call& c) { c.pre.preempting_job_ids = nullptr; });
  call("call_no_offsets_out", [](Call& c) { c.pout.offsets = nullptr; });
  return g_fail ? 1 : 0;
}
