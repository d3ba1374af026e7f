// cranesched_amd/csrc/limits_check_host.inc (the input rules of cns_set_run_limits / cns_upload_limit_jobs) and the record space and chain
// walk of acct_space_host.inc compiled with g++ and driven over hand cases: the space by its numbers, valid calls, then every rule of
// include/crane_gpu/run_limits.h broken in turn, each at its edge.  Prints "<case>: <status> <message>" per case, so that
// tests/test_limits_host.py can hold every refusal to its message; built once plain and once with -fsanitize=address,undefined: every
// array below is exactly as long as the header says, so a pass that reads past one is caught.  (The cases "by counts alone" are refused
// before any table of that size is read.)
#include <cstdio>
#include <functional>
#include <vector>

#include "../../cranesched_amd/csrc/limits_check_host.inc"

namespace {

constexpr uint32_t N = CNS_LIM_NONE;

int g_fail = 0;

void list(const char* name, const uint64_t* v, int n) {
  printf(" %s=", name);
  for (int i = 0; i < n; ++i) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
}

void space(const char* name, uint32_t U, uint32_t UA, uint32_t A, uint32_t Q, uint32_t Pn) {
  cns_acct::Space s;
  if (!cns_acct::make_space(U, UA, A, Q, Pn, &s)) { printf("%s: 1 refused\n", name); return; }
  printf("%s: 0", name);
  list("len", s.len, 5); list("base", s.base, 5); list("NR", &s.NR, 1); list("ent", s.ent, 3); list("ent_len", s.ent_len, 3); list("NE", &s.NE, 1);
  printf("\n");
}

struct Case {
  // the smallest tables that reach every rule: 2 users, 2 (user, account) pairs, 2 accounts (0 root <- 1), 1 QoS, 1 partition
  std::vector<uint32_t> parent{N, 0};
  std::vector<cns_qos_limits> qos = std::vector<cns_qos_limits>(1);
  std::vector<cns_part_limit> pl = std::vector<cns_part_limit>(1);
  std::vector<uint32_t> upl{N, 0}, apl{0, N};
  // three jobs of a cycle of three
  std::vector<uint64_t> sel{2, 0, 1};
  std::vector<uint32_t> user{0, 1, 1}, ua{0, 1, 0}, account{1, 0, 1}, qosk{0, 0, 0}, part{0, 0, 0};
  std::vector<int64_t> tl{60, 60, 60};
  std::vector<uint8_t> skip{0, 0, 0};
  uint64_t select_J = 3;
  cns_limit_tables t{};
  cns_limit_job_soa jb{};
  void bind() {
    t.num_users = 2; t.num_user_accts = 2; t.num_accounts = (uint32_t)parent.size(); t.num_qos = 1; t.num_partitions = 1; t.num_part_limits = 1;
    t.qos = qos.data(); t.acct_parent = parent.data(); t.part_limits = pl.data(); t.user_part_limit = upl.data(); t.acct_part_limit = apl.data();
    jb.num_jobs = user.size(); jb.select_index = sel.data();
    jb.user = user.data(); jb.user_acct = ua.data(); jb.account = account.data(); jb.qos = qosk.data(); jb.partition = part.data();
    jb.time_limit_sec = tl.data(); jb.skip = skip.data();
  }
  // an account tree of its own: the per-account tables follow its size
  void tree(std::vector<uint32_t> p) {
    parent = std::move(p);
    apl.assign(parent.size(), N);
    bind();
  }
};

void run(const char* name, const std::function<void(Case&)>& edit) {
  Case c;
  c.bind();
  edit(c);
  cns_acct::Space sp;
  std::vector<uint32_t> level;
  cns_acct::Verdict v = cns_limits_host::check_tables(&c.t, &sp, &level);
  const bool tables_ok = !v;
  if (tables_ok) v = cns_limits_host::check_jobs(sp, &c.jb, c.select_J);
  printf("%s: %d %s", name, v.code, v.msg.c_str());
  if (!v) {
    if (level.size() != sp.A) ++g_fail;
    printf("NR=%llu levels=", (unsigned long long)sp.NR);
    for (size_t i = 0; i < level.size(); ++i) printf("%s%u", i ? "," : "", level[i]);
  }
  printf("\n");
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

}  // namespace

int main() {
  // ---- the record space
  space("space_five_tables", 3, 4, 7, 2, 5);
  space("space_one_qos_alone", 0, 0, 0, 1, 0);
  space("space_table_of_2_32_minus_16", 0, 0xFFFFFFF0u, 0, 1, 1);
  space("space_table_of_2_32_minus_15", 0, 0xFFFFFFF1u, 0, 1, 1);
  space("space_sum_that_wraps_64_bits", 0xFFFFFFFFu, 0xFFFFFFFEu, 1, 0x80000000u, 0x80000000u);
  // ---- cns_set_run_limits
  run("valid", [](Case&) {});
  run("no_qos", [](Case& c) { c.t.num_qos = 0; });
  run("no_qos_array", [](Case& c) { c.t.qos = nullptr; });
  run("no_acct_parent", [](Case& c) { c.t.acct_parent = nullptr; });
  run("no_part_limits", [](Case& c) { c.t.part_limits = nullptr; });
  run("too_many_records", [](Case& c) { c.t.num_users = 0x80000000u; c.t.num_qos = 2; });                  // by the counts alone
  run("records_sum_at_2_32_minus_16", [](Case& c) { c.t.num_user_accts = 0xFFFFFFF0u - 7; c.t.user_part_limit = nullptr; });   // 2 + UA + 2 + 2 + 1
  run("limit_records_at_2_32_minus_16", [](Case& c) { c.t.num_part_limits = 0xFFFFFFF0u - 3; });           // 3 Q + L
  run("records_sum_at_2_32_minus_17", [](Case& c) { c.t.num_user_accts = 0xFFFFFFF0u - 8; c.t.user_part_limit = nullptr; c.ua[1] = 0xFFFFFFF0u - 9; });
  run("records_sum_that_wraps_64_bits", [](Case& c) { c.tree({N}); c.t.num_users = 0xFFFFFFFFu; c.t.num_user_accts = 0xFFFFFFFEu; c.t.num_qos = 0x80000000u;
                                                      c.t.num_partitions = 0x80000000u; });   // U Q + UA Pn + A Q + A Pn + Q = 2^64
  run("chain_of_6", [](Case& c) { c.tree({N, 0, 1, 2, 3, 4}); });
  run("chain_of_6_leaf_first", [](Case& c) { c.tree({1, 2, 3, 4, 5, N}); });
  run("two_trees_share_levels", [](Case& c) { c.tree({3, N, 1, 2, N, 4, 0}); });
  run("chain_of_7", [](Case& c) { c.tree({N, 0, 1, 2, 3, 4, 5}); });
  run("chain_of_7_leaf_first", [](Case& c) { c.tree({1, 2, 3, 4, 5, 6, N}); });
  run("chain_cycle_of_two", [](Case& c) { c.tree({1, 0}); });
  run("chain_self_parent", [](Case& c) { c.tree({N, 1}); });
  run("parent_of_A", [](Case& c) { c.tree({N, 2}); });
  run("chain_is_refused_before_a_later_parent", [](Case& c) { c.tree({1, 0, 9}); });                      // account by account
  run("chain_is_refused_before_max_wall", [](Case& c) { c.tree({1, 0}); c.qos[0].max_wall_sec = -1; });
  run("negative_qos_max_wall", [](Case& c) { c.qos[0].max_wall_sec = -1; c.pl[0].max_wall_sec = -1; });
  run("negative_partition_max_wall", [](Case& c) { c.pl[0].max_wall_sec = -1; c.upl[0] = 1; });
  run("user_part_limit_index", [](Case& c) { c.upl[0] = 1; });
  run("acct_part_limit_index", [](Case& c) { c.apl[1] = 1; });
  // ---- cns_upload_limit_jobs
  run("no_user", [](Case& c) { c.jb.user = nullptr; });
  run("no_time_limit", [](Case& c) { c.jb.time_limit_sec = nullptr; });
  run("no_jobs_needs_no_array", [](Case& c) { c.jb = cns_limit_job_soa{}; });
  run("too_many_jobs", [](Case& c) { c.jb.num_jobs = 0xFFFFFFF1ull; });                                    // by the count alone
  run("user_out_of_range", [](Case& c) { c.user[2] = 2; });
  run("user_acct_out_of_range", [](Case& c) { c.ua[0] = 2; });
  run("user_acct_none", [](Case& c) { c.ua[1] = N; });
  run("account_out_of_range", [](Case& c) { c.account[1] = 2; });
  run("qos_out_of_range", [](Case& c) { c.qosk[0] = 1; });
  run("partition_out_of_range", [](Case& c) { c.part[2] = 1; });
  run("valid_skipped_job_is_not_read", [](Case& c) { c.user[1] = 99; c.ua[1] = N; c.sel[1] = 99; c.skip[1] = 1; });
  run("select_index_at_the_job_count", [](Case& c) { c.sel[1] = 3; });
  run("keys_are_refused_before_select_index", [](Case& c) { c.sel[0] = 3; c.part[0] = 1; });
  run("identity_select_past_the_cycle", [](Case& c) { c.jb.select_index = nullptr; c.select_J = 2; });
  run("valid_identity_select", [](Case& c) { c.jb.select_index = nullptr; });
  return g_fail ? 1 : 0;
}
