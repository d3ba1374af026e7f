// cranesched_amd/csrc/submit_check_host.inc (the input rules of cns_set_submit_limits / cns_check_submissions) compiled with g++ and
// driven over hand cases: valid calls, then every rule of include/crane_gpu_submit/submit_limits.h broken in turn, each at its edge.
// Prints "<case>: <status> <message>" per case, so that tests/test_submit_host.py can hold every refusal to its message; built once plain
// and once with -fsanitize=address,undefined: every array below is exactly as long as the header says, so a pass that reads past one is
// caught.  (The cases "by counts alone" are refused before any table of that size is read.)
#include <cstdio>
#include <functional>
#include <vector>

#include "../../cranesched_amd/csrc/submit_check_host.inc"

namespace {

constexpr uint32_t N = CNS_LIM_NONE;

struct Case {
  // the smallest tables that reach every rule: 2 users, 2 (user, account) pairs, 2 accounts (0 root <- 1), 1 QoS, 1 partition
  std::vector<uint32_t> parent{N, 0};
  std::vector<cns_submit_qos> qos = std::vector<cns_submit_qos>(1);
  std::vector<cns_submit_part_limit> pl = std::vector<cns_submit_part_limit>(1);
  std::vector<uint32_t> upl{N, 0}, apl{0, N};
  std::vector<cns_usage> uq = std::vector<cns_usage>(2), aq = std::vector<cns_usage>(2), g = std::vector<cns_usage>(1);
  // three submissions: what the job table carries, then the keys
  std::vector<uint32_t> part{0, 0, 0}, k{1, 1, 1}, nt{1, 1, 1};
  std::vector<int64_t> tl{60, 60, 60}, tcpu{256, 256, 256};
  std::vector<uint64_t> nmem{0, 0, 0}, tmem{1, 1, 1};
  std::vector<uint32_t> user{0, 1, 1}, ua{0, N, 0}, account{1, 0, 1}, qosk{0, 0, 0}, count{1, 1, 1};
  std::vector<uint8_t> skip{0, 0, 0}, code = std::vector<uint8_t>(3);
  std::vector<int64_t> tlo = std::vector<int64_t>(3);
  uint32_t flags = 0, max_set = 0, max_cur = 0;
  cns_submit_tables t{};
  cns_job_soa jb{};
  cns_submit_keys ky{};
  cns_submit_out out{};
  void bind() {
    t.num_users = 2; t.num_user_accts = 2; t.num_accounts = (uint32_t)parent.size(); t.num_qos = 1; t.num_partitions = 1; t.num_part_limits = 1;
    t.gres.num_classes = 2; t.gres.class_name[0] = 0; t.gres.class_name[1] = 3;
    t.qos = qos.data(); t.acct_parent = parent.data(); t.part_limits = pl.data(); t.user_part_limit = upl.data(); t.acct_part_limit = apl.data();
    t.user_qos = uq.data(); t.acct_qos = aq.data(); t.qos_usage = g.data();
    jb.num_jobs = user.size();
    jb.partition = part.data(); jb.time_limit_sec = tl.data(); jb.node_mem = nmem.data(); jb.task_cpu_raw = tcpu.data(); jb.task_mem = tmem.data();
    jb.node_num = k.data(); jb.ntasks = nt.data();
    ky.user = user.data(); ky.user_acct = ua.data(); ky.account = account.data(); ky.qos = qosk.data(); ky.count = count.data(); ky.skip = skip.data();
    out.code = code.data(); out.time_limit_out = tlo.data();
  }
  // an account tree of its own: the per-account tables follow its size
  void tree(std::vector<uint32_t> p) {
    parent = std::move(p);
    apl.assign(parent.size(), N);
    aq.assign(parent.size(), cns_usage{});
    bind();
  }
};

int g_fail = 0;

void run(const char* name, const std::function<void(Case&)>& edit) {
  Case c;
  c.bind();
  edit(c);
  cns_acct::Space sp;
  cns_acct::Verdict v = cns_submit_host::check_tables(&c.t, &sp);
  if (!v) v = cns_submit_host::check_jobs(sp, &c.jb, &c.ky, &c.out, c.flags, c.max_set, c.max_cur);
  printf("%s: %d %s", name, v.code, v.msg.c_str());
  if (!v) printf("NR=%llu NE=%llu", (unsigned long long)sp.NR, (unsigned long long)sp.NE);
  printf("\n");
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

}  // namespace

int main() {
  // ---- cns_set_submit_limits
  run("valid", [](Case&) {});                                                        // CNS_LIM_NONE as user_acct is a key in range
  run("valid_no_accounts_no_tables", [](Case& c) { c.t = cns_submit_tables{}; c.t.num_users = 2; c.t.num_user_accts = 2; c.t.num_qos = 1; c.t.num_partitions = 1;
                                                   c.t.qos = c.qos.data(); c.skip[0] = c.skip[1] = c.skip[2] = 1; });   // no account: no job can have one
  run("no_qos", [](Case& c) { c.t.qos = nullptr; });
  run("no_acct_parent", [](Case& c) { c.t.acct_parent = nullptr; });
  run("no_part_limits", [](Case& c) { c.t.part_limits = nullptr; });
  run("missing_table_before_gres", [](Case& c) { c.t.qos = nullptr; c.t.gres.num_classes = 9; });
  run("gres_classes", [](Case& c) { c.t.gres.num_classes = 9; c.t.gres.class_name[0] = 4; });
  run("gres_class_name", [](Case& c) { c.t.gres.class_name[1] = 4; c.t.num_users = 0x80000000u; c.t.num_qos = 2; });
  run("too_many_records", [](Case& c) { c.t.num_users = 0x80000000u; c.t.num_qos = 2; c.parent[0] = 5; });            // one table, by the counts alone
  run("records_and_entities_at_2_32_minus_16", [](Case& c) { c.t.num_user_accts = 0xFFFFFFF0u - 12; c.t.user_part_limit = nullptr; });   // 2 + UA + 2 + 2 + 1, + 5
  run("records_and_entities_at_2_32_minus_17", [](Case& c) { c.t.num_user_accts = 0xFFFFFFF0u - 13; c.t.user_part_limit = nullptr; });
  run("records_sum_that_wraps_64_bits", [](Case& c) { c.tree({N}); c.t.num_users = 0xFFFFFFFFu; c.t.num_user_accts = 0xFFFFFFFEu; c.t.num_qos = 0x80000000u;
                                                      c.t.num_partitions = 0x80000000u; });
  run("parent_of_A", [](Case& c) { c.tree({N, 2}); });
  run("parents_are_refused_before_chains", [](Case& c) { c.tree({1, 0, N, 4}); });
  run("chain_of_6", [](Case& c) { c.tree({N, 0, 1, 2, 3, 4}); c.account[0] = 5; c.account[2] = 3; });
  run("chain_of_6_leaf_first", [](Case& c) { c.tree({1, 2, 3, 4, 5, N}); });
  run("chain_of_7", [](Case& c) { c.tree({N, 0, 1, 2, 3, 4, 5}); });
  run("chain_of_7_leaf_first", [](Case& c) { c.tree({1, 2, 3, 4, 5, 6, N}); });
  run("chain_of_7_behind_a_short_one", [](Case& c) { c.tree({N, 0, 3, 4, 5, 6, 7, 8, N}); });
  run("chain_cycle_of_two", [](Case& c) { c.tree({1, 0}); });
  run("chain_self_parent", [](Case& c) { c.tree({N, 1}); });
  run("chain_into_a_cycle_of_eight", [](Case& c) { c.tree({N, 2, 3, 4, 5, 6, 7, 8, 9, 2}); });
  run("chains_are_refused_before_limit_indices", [](Case& c) { c.tree({1, 0}); c.upl[0] = 1; });
  run("user_part_limit_index", [](Case& c) { c.upl[0] = 1; c.g[0].jobs_count = 0xFFFFFFFFu; });
  run("acct_part_limit_index", [](Case& c) { c.apl[1] = 1; });
  run("jobs_count_of_uint32_max", [](Case& c) { c.aq[1].jobs_count = 0xFFFFFFFFu; });
  // ---- cns_check_submissions
  run("no_partition", [](Case& c) { c.jb.partition = nullptr; c.ky.user = nullptr; });
  run("no_ntasks", [](Case& c) { c.jb.ntasks = nullptr; });
  run("valid_no_node_cpu_no_gres", [](Case& c) { c.jb.node_cpu_raw = nullptr; c.jb.gres_total = nullptr; c.jb.gres_spec = nullptr; });
  run("no_user", [](Case& c) { c.ky.user = nullptr; c.out.code = nullptr; });
  run("no_count", [](Case& c) { c.ky.count = nullptr; });
  run("no_code", [](Case& c) { c.out.code = nullptr; c.user[0] = 2; });
  run("no_time_limit_out", [](Case& c) { c.out.time_limit_out = nullptr; });
  run("user_out_of_range", [](Case& c) { c.user[2] = 2; });
  run("user_acct_out_of_range", [](Case& c) { c.ua[0] = 2; });
  run("account_out_of_range", [](Case& c) { c.account[1] = 2; });
  run("qos_out_of_range", [](Case& c) { c.qosk[0] = 1; });
  run("partition_out_of_range", [](Case& c) { c.part[2] = 1; });
  run("valid_skipped_job_is_not_read", [](Case& c) { c.user[1] = 99; c.part[1] = 99; c.count[1] = 0xFFFFFFFFu; c.skip[1] = 1; });
  run("keys_are_refused_before_the_sum", [](Case& c) { c.count[0] = 0xFFFFFFFFu; c.qosk[2] = 1; });
  run("sum_at_uint32_max", [](Case& c) { c.max_set = 0xFFFFFFFCu; });
  run("sum_at_2_32", [](Case& c) { c.max_set = 0xFFFFFFFDu; });
  run("sum_of_counts_alone_at_2_32", [](Case& c) { c.count[0] = 0xFFFFFFFFu; c.count[2] = 0; });
  run("carry_sum_at_uint32_max", [](Case& c) { c.flags = CNS_SUBMIT_CARRY; c.max_set = 0xFFFFFFFFu; c.max_cur = 0xFFFFFFFCu; });
  run("carry_sum_at_2_32", [](Case& c) { c.flags = CNS_SUBMIT_CARRY; c.max_cur = 0xFFFFFFFDu; });
  run("without_carry_the_last_call_does_not_count", [](Case& c) { c.max_cur = 0xFFFFFFFDu; });
  return g_fail ? 1 : 0;
}
