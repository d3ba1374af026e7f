// Drives GpuNodeSelectionAlgo::ReleaseMetaResources / ChargeMetaResources (include/crane_gpu_usage/usage.h): hand-derived cases at string
// level — the records after the batch, erased entries erased, the reference's two messages per entity name — and, with --bench, a
// measurement of cns_usage_apply against a single-threaded loop in this file that restates AccountMetaContainer.cpp:1067-1208 over
// std::unordered_maps on the same host.
//   test_usage_adapter            -> needs an MI355X, exit 0 on success
//   test_usage_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_usage_adapter --bench [jobs]   -> a recovery charge of 1 M jobs into empty tables and a status-change burst of 1 M releases over 1024
//                                    users, 64 accounts (8 roots x 7 children), 4 QoS and 8 partitions (the account tree of
//                                    test_submit_adapter --bench): the device call by stage and the CPU loop; one warm-up, median of 5.
//                                    Asserted there: the device's tables and masks equal the loop's.
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_usage/usage.h"

using namespace crane;
using Delta = GpuNodeSelectionAlgo::UsageDelta;
using Report = GpuNodeSelectionAlgo::UsageReport;

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  return m;
}
static ResourceView alloc(int cpu, uint64_t mem_gib) {
  ResourceView v;
  v.cpu_count = cpu_t(cpu); v.memory_bytes = mem_gib * G;
  return v;
}
static MetaResource rec(int cpu, uint64_t mem_gib, uint32_t jobs, uint32_t submit, int64_t wall) {
  MetaResource m;
  m.resource = alloc(cpu, mem_gib); m.jobs_count = jobs; m.submit_jobs_count = submit; m.wall_time = wall;
  return m;
}
static bool is(const MetaResource& m, int cpu, uint64_t mem_gib, uint32_t jobs, uint32_t submit, int64_t wall) {
  return m.resource.cpu_count.raw == (int64_t)cpu * 256 && m.resource.memory_bytes == mem_gib * G && m.resource.gres_map.empty() && m.jobs_count == jobs &&
         m.submit_jobs_count == submit && m.wall_time == wall;
}

static AccountMetaSnapshot start() {
  // accounts: lab -> dept (root); users: ann (lab), bob (lab), eve (no account); QoS normal, tight; partitions p0, p1.
  // ann's two records and lab's two hold {4 cores, 8 GiB, 2 jobs, 3 submitted, 7200 s}; dept's two and the QoS "normal" twice that with 5
  // submitted.  bob and eve have no record.
  AccountMetaSnapshot meta;
  meta.qos["normal"]; meta.qos["tight"];
  meta.account_parent = {{"lab", "dept"}, {"dept", ""}};
  meta.user_accounts["ann"]["lab"]; meta.user_accounts["bob"]["lab"]; meta.user_accounts["eve"];
  meta.user_meta["ann"].qos_to_resource_map["normal"] = rec(4, 8, 2, 3, 7200);
  meta.user_meta["ann"].account_to_partition_to_resource_map["lab"]["p0"] = rec(4, 8, 2, 3, 7200);
  meta.account_meta["lab"].qos_to_resource_map["normal"] = rec(4, 8, 2, 3, 7200);
  meta.account_meta["lab"].partition_to_resource_map["p0"] = rec(4, 8, 2, 3, 7200);
  meta.account_meta["dept"].qos_to_resource_map["normal"] = rec(8, 16, 4, 5, 14400);
  meta.account_meta["dept"].partition_to_resource_map["p0"] = rec(8, 16, 4, 5, 14400);
  meta.qos_meta["normal"] = rec(8, 16, 4, 5, 14400);
  return meta;
}

static int hand_cases(GpuNodeSelectionAlgo& algo) {
  ClusterSnapshot snap;
  snap.craned_metas = {node("n0", 8, 16), node("n1", 8, 16)};
  snap.partitions = {{"p0", {"n0", "n1"}}, {"p1", {"n1"}}};
  algo.SetClusterSnapshot(snap);
  CHECK(algo.Ok());
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }
  using V = std::vector<std::string>;
  struct Want { bool skipped; V not_found, over_free; };
  std::vector<Delta> fr;
  std::vector<Want> want;
  auto add = [&](Delta d, bool skipped, V nf, V of) { fr.push_back(std::move(d)); want.push_back({skipped, std::move(nf), std::move(of)}); };
  // 0: :243 a finished job of ann's: 2 cores, 4 GiB, 1 job, 1 submitted, 3600 s off all seven records
  add(Delta::FreeMetaResource("ann", "lab", "normal", "p0", alloc(2, 4), 3600, false), false, {}, {});
  // 1: :226 two submitted jobs leave the queue: ann's and lab's records at 0 submitted, not zero (the rest is not)
  add(Delta::FreeMetaSubmitResource("ann", "lab", "normal", "p0", 2), false, {}, {});
  // 2: :256 a requeue frees exactly what ann's and lab's records still hold: :1159 erases the four; dept and the QoS keep {4, 8, 2, 2, 7200}
  add(Delta::FreeMetaRunningResource("ann", "lab", "normal", "p0", alloc(2, 4), 3600), false, {}, {});
  // 3: the four keys are gone (:1143); dept and the QoS go to 1 submitted
  add(Delta::FreeMetaSubmitResource("ann", "lab", "normal", "p0", 1), false, {"user ann", "user ann", "account lab", "account lab"}, {});
  // 4: :271 bob has no record (:1162 says nothing); lab's keys are gone; dept and the QoS: {3, 7, 1, 1, 7140}
  {
    PdJobInScheduler j;
    j.username = "bob"; j.account = "lab"; j.qos = "normal"; j.partition_id = "p0"; j.time_limit = 60;
    add(Delta::FreeMetaResource(j, alloc(1, 1)), false, {"account lab", "account lab"}, {});
  }
  // 5: another QoS: nobody has a "tight" entry, ann's and lab's p0 are gone, dept's p0 goes to 0 submitted; the QoS "tight" has no record (:1190)
  add(Delta::FreeMetaSubmitResource("ann", "lab", "tight", "p0", 1), false, {"user ann", "user ann", "account lab", "account lab", "account dept"}, {});
  // 6: 8 cores > 3: dept's two records and the QoS free more than allocated (:1152, :1196): zeroed, dept's erased, the QoS stays
  add(Delta::FreeMetaResource("ann", "lab", "normal", "p0", alloc(8, 1), 10, true), false, {"user ann", "user ann", "account lab", "account lab"},
      {"account dept", "account dept", "qos normal"});
  // 7: an unknown user: not applied
  add(Delta::FreeMetaSubmitResource("zoe", "lab", "normal", "p0", 1), true, {}, {});
  // 8: eve has no record; every account key is gone; the QoS record is zero and over-frees again
  add(Delta::FreeMetaSubmitResource("eve", "lab", "normal", "p0", 1), false, {"account lab", "account lab", "account dept", "account dept"}, {"qos normal"});

  {  // the first two alone: the values in between
    AccountMetaSnapshot meta = start();
    CHECK(algo.ReleaseMetaResources(&meta, {fr[0], fr[1]}));
    CHECK(is(meta.user_meta["ann"].qos_to_resource_map["normal"], 2, 4, 1, 0, 3600) && is(meta.user_meta["ann"].account_to_partition_to_resource_map["lab"]["p0"], 2, 4, 1, 0, 3600));
    CHECK(is(meta.account_meta["lab"].qos_to_resource_map["normal"], 2, 4, 1, 0, 3600) && is(meta.account_meta["lab"].partition_to_resource_map["p0"], 2, 4, 1, 0, 3600));
    CHECK(is(meta.account_meta["dept"].qos_to_resource_map["normal"], 6, 12, 3, 2, 10800) && is(meta.account_meta["dept"].partition_to_resource_map["p0"], 6, 12, 3, 2, 10800));
    CHECK(is(meta.qos_meta["normal"], 6, 12, 3, 2, 10800));
  }
  {  // up to delta 5: what is erased and what is left
    AccountMetaSnapshot meta = start();
    CHECK(algo.ReleaseMetaResources(&meta, {fr[0], fr[1], fr[2], fr[3], fr[4], fr[5]}));
    CHECK(meta.user_meta.count("ann") && meta.user_meta["ann"].qos_to_resource_map.empty());
    CHECK(meta.user_meta["ann"].account_to_partition_to_resource_map.count("lab") && meta.user_meta["ann"].account_to_partition_to_resource_map["lab"].empty());
    CHECK(meta.account_meta["lab"].qos_to_resource_map.empty() && meta.account_meta["lab"].partition_to_resource_map.empty());
    CHECK(is(meta.account_meta["dept"].qos_to_resource_map["normal"], 3, 7, 1, 1, 7140) && is(meta.account_meta["dept"].partition_to_resource_map["p0"], 3, 7, 1, 0, 7140));
    CHECK(is(meta.qos_meta["normal"], 3, 7, 1, 1, 7140) && !meta.qos_meta.count("tight") && !meta.user_meta.count("bob"));
  }
  AccountMetaSnapshot meta = start();
  std::vector<Report> rep;
  cns_usage_timing tm{};
  CHECK(algo.ReleaseMetaResources(&meta, fr, &rep, &tm));
  if (!algo.Ok()) printf("ReleaseMetaResources: %s\n", algo.LastError().c_str());
  CHECK(rep.size() == fr.size());
  for (size_t i = 0; i < rep.size() && i < want.size(); ++i) {
    const bool ok = rep[i].skipped == want[i].skipped && rep[i].not_found == want[i].not_found && rep[i].over_free == want[i].over_free;
    if (!ok) {
      printf("delta %zu: skipped %d, not found:", i, (int)rep[i].skipped);
      for (const auto& s : rep[i].not_found) printf(" [%s]", s.c_str());
      printf(", freed more than allocated:");
      for (const auto& s : rep[i].over_free) printf(" [%s]", s.c_str());
      printf("\n");
      ++g_fail;
    }
  }
  CHECK(meta.user_meta.count("ann") && meta.user_meta["ann"].qos_to_resource_map.empty() && meta.user_meta["ann"].account_to_partition_to_resource_map["lab"].empty());
  CHECK(meta.account_meta.count("lab") && meta.account_meta.count("dept"));                     // DoFreeResource_ removes no entity
  CHECK(meta.account_meta["dept"].qos_to_resource_map.empty() && meta.account_meta["dept"].partition_to_resource_map.empty());
  CHECK(meta.qos_meta.count("normal") && is(meta.qos_meta["normal"], 0, 0, 0, 0, 0));           // never erased (:1190-1202)
  CHECK(!meta.user_meta.count("bob") && !meta.user_meta.count("eve") && !meta.user_meta.count("zoe") && !meta.qos_meta.count("tight"));
  CHECK(tm.records == 10 && tm.items > 0);   // the seven of "normal" on p0 and the three "tight" entries delta 5 looks for

  // charges: the two recovery calls create bob's record, the "tight" entries along lab -> dept, and the QoS "tight"
  AccountMetaSnapshot cm = start();
  ResourceView a22 = alloc(2, 2);
  a22.gres_map["fpga"];                                                                           // a zero-count entry: dropped
  CHECK(algo.ChargeMetaResources(&cm, {Delta::MallocMetaSubmitResource("bob", "lab", "tight", "p1", 4),
                                       Delta::MallocMetaResourceToRecoveredRunningJob("bob", "lab", "tight", "p1", a22, 500, false),
                                       Delta::MallocMetaResourceToRecoveredRunningJob("ann", "lab", "normal", "p0", alloc(1, 1), 100, true)}));
  if (!algo.Ok()) printf("ChargeMetaResources: %s\n", algo.LastError().c_str());
  CHECK(cm.user_meta.count("bob") && is(cm.user_meta["bob"].qos_to_resource_map["tight"], 2, 2, 1, 5, 500));
  CHECK(is(cm.user_meta["bob"].account_to_partition_to_resource_map["lab"]["p1"], 2, 2, 1, 5, 500));
  CHECK(is(cm.account_meta["lab"].qos_to_resource_map["tight"], 2, 2, 1, 5, 500) && is(cm.account_meta["lab"].partition_to_resource_map["p1"], 2, 2, 1, 5, 500));
  CHECK(is(cm.account_meta["dept"].qos_to_resource_map["tight"], 2, 2, 1, 5, 500) && is(cm.account_meta["dept"].partition_to_resource_map["p1"], 2, 2, 1, 5, 500));
  CHECK(cm.qos_meta.count("tight") && is(cm.qos_meta["tight"], 2, 2, 1, 5, 500));
  CHECK(is(cm.user_meta["ann"].qos_to_resource_map["normal"], 5, 9, 3, 3, 7300) && is(cm.account_meta["dept"].partition_to_resource_map["p0"], 9, 17, 5, 5, 14500));
  CHECK(is(cm.qos_meta["normal"], 9, 17, 5, 5, 14500));
  // refused, nothing written: a charge under an unknown user; an all-zero delta
  AccountMetaSnapshot keep = start();
  CHECK(!algo.ChargeMetaResources(&keep, {Delta::MallocMetaSubmitResource("zoe", "lab", "tight", "p1", 4)}) && algo.LastStatus() == CNS_ERR_INVALID_ARG);
  CHECK(!algo.ReleaseMetaResources(&keep, {Delta::FreeMetaSubmitResource("ann", "lab", "normal", "p0", 0)}) && algo.LastStatus() == CNS_ERR_INVALID_ARG);
  CHECK(is(keep.user_meta["ann"].qos_to_resource_map["normal"], 4, 8, 2, 3, 7200) && !keep.qos_meta.count("tight"));
  std::vector<Report> none;
  CHECK(algo.ReleaseMetaResources(&keep, {}, &none) && none.empty());
  printf("hand cases: %zu frees, 3 charges, %d failures\n", fr.size(), g_fail);
  return g_fail;
}

// ---- --bench: the loop that restates the reference over unordered_maps, the device call ------------------------------------------------------
using Rec = std::array<uint64_t, 17>;   // cpu, mem, wall, jobs, submit, 4 name totals, 8 class counts (a MetaResource; zero = no GRES entry)
struct Stat {                           // MetaResourceStat, AccountMetaContainer.h:62-80
  std::unordered_map<uint32_t, Rec> qos;
  std::unordered_map<uint32_t, std::unordered_map<uint32_t, Rec>> acct_part;   // users
  std::unordered_map<uint32_t, Rec> part;                                      // accounts
};
struct Maps {
  std::unordered_map<uint32_t, Stat> user, account;
  std::unordered_map<uint32_t, Rec> qos;
};
struct Jobs {
  std::vector<uint32_t> user, acct, qos, part, jc, sc;
  std::vector<int64_t> cpu, wall;
  std::vector<uint64_t> mem;
};
static Rec delta_of(const Jobs& B, size_t j) {
  Rec d{};
  d[0] = (uint64_t)B.cpu[j]; d[1] = B.mem[j]; d[2] = (uint64_t)B.wall[j]; d[3] = B.jc[j]; d[4] = B.sc[j];
  return d;
}
static bool le(const Rec& a, const Rec& b) { for (int c = 0; c < 17; ++c) if (a[c] > b[c]) return false; return true; }            // :33-37
static bool zero(const Rec& a) { for (int c = 0; c < 17; ++c) if (a[c]) return false; return true; }

// DoMallocResource_, :1067-1124
static void cpu_charge(Maps& M, const std::vector<uint32_t>& parent, const Jobs& B, size_t j) {
  const Rec d = delta_of(B, j);
  auto upsert = [&](std::unordered_map<uint32_t, Rec>& m, uint32_t key) {                                                            // :1078-1084
    auto it = m.find(key);
    if (it == m.end()) m.emplace(key, d);
    else for (int c = 0; c < 17; ++c) it->second[c] += d[c];
  };
  Stat& us = M.user[B.user[j]];                                                                                                        // :1086
  upsert(us.qos, B.qos[j]);
  upsert(us.acct_part[B.acct[j]], B.part[j]);
  for (uint32_t a = B.acct[j]; a != CNS_LIM_NONE; a = parent[a]) { Stat& as = M.account[a]; upsert(as.qos, B.qos[j]); upsert(as.part, B.part[j]); }   // :1106
  upsert(M.qos, B.qos[j]);                                                                                                             // :1118
}
// DoFreeResource_, :1126-1208
static void cpu_release(Maps& M, const std::vector<uint32_t>& parent, const Jobs& B, size_t j, uint16_t& nf, uint16_t& of) {
  const Rec d = delta_of(B, j);
  nf = of = 0;
  auto safe_sub = [&](std::unordered_map<uint32_t, Rec>& m, uint32_t key, uint32_t bit) {                                              // :1138-1160
    auto it = m.find(key);
    if (it == m.end()) { nf |= (uint16_t)(1u << bit); return; }
    Rec& val = it->second;
    if (le(d, val)) { for (int c = 0; c < 17; ++c) val[c] -= d[c]; }
    else { of |= (uint16_t)(1u << bit); val = Rec{}; }
    if (zero(val)) m.erase(it);
  };
  if (auto u = M.user.find(B.user[j]); u != M.user.end()) {                                                                            // :1162
    safe_sub(u->second.qos, B.qos[j], CNS_USAGE_BIT_USER_QOS);
    auto ap = u->second.acct_part.find(B.acct[j]);
    if (ap != u->second.acct_part.end()) safe_sub(ap->second, B.part[j], CNS_USAGE_BIT_USER_PART);
    else nf |= 1u << CNS_USAGE_BIT_USER_PART;                                                                                          // :1172
  }
  uint32_t i = 0;
  for (uint32_t a = B.acct[j]; a != CNS_LIM_NONE; a = parent[a], ++i)                                                                  // :1179
    if (auto s = M.account.find(a); s != M.account.end()) { safe_sub(s->second.qos, B.qos[j], CNS_USAGE_BIT_ACCT_QOS(i)); safe_sub(s->second.part, B.part[j], CNS_USAGE_BIT_ACCT_PART(i)); }
  if (auto q = M.qos.find(B.qos[j]); q != M.qos.end()) {                                                                               // :1190
    if (le(d, q->second)) { for (int c = 0; c < 17; ++c) q->second[c] -= d[c]; }
    else { of |= 1u << CNS_USAGE_BIT_QOS; q->second = Rec{}; }
  }
}

struct Dense {
  std::vector<cns_usage> uq, up, aq, ap, qu;
  std::vector<uint32_t> uqs, ups, aqs, aps, qs;
  std::vector<uint8_t> uqe, upe, aqe, ape, uex, aex, qex;
  Dense(uint32_t U, uint32_t A, uint32_t Q, uint32_t Pn)
      : uq((size_t)U * Q), up((size_t)U * Pn), aq((size_t)A * Q), ap((size_t)A * Pn), qu(Q), uqs(uq.size()), ups(up.size()), aqs(aq.size()), aps(ap.size()), qs(Q),
        uqe(uq.size()), upe(up.size()), aqe(aq.size()), ape(ap.size()), uex(U), aex(A), qex(Q) {}
  cns_usage_tables_out out() {
    cns_usage_tables_out o{};
    o.user_qos = uq.data(); o.user_part = up.data(); o.acct_qos = aq.data(); o.acct_part = ap.data(); o.qos_usage = qu.data();
    o.user_qos_submit = uqs.data(); o.user_part_submit = ups.data(); o.acct_qos_submit = aqs.data(); o.acct_part_submit = aps.data(); o.qos_submit = qs.data();
    o.user_qos_exists = uqe.data(); o.user_part_exists = upe.data(); o.acct_qos_exists = aqe.data(); o.acct_part_exists = ape.data();
    o.user_exists = uex.data(); o.acct_exists = aex.data(); o.qos_exists = qex.data();
    return o;
  }
  cns_usage_tables in(uint32_t U, uint32_t A, uint32_t Q, uint32_t Pn, const std::vector<uint32_t>& parent) const {
    cns_usage_tables t{};
    t.num_users = t.num_user_accts = U; t.num_accounts = A; t.num_qos = Q; t.num_partitions = Pn; t.acct_parent = parent.data();
    t.user_qos = uq.data(); t.user_part = up.data(); t.acct_qos = aq.data(); t.acct_part = ap.data(); t.qos_usage = qu.data();
    t.user_qos_submit = uqs.data(); t.user_part_submit = ups.data(); t.acct_qos_submit = aqs.data(); t.acct_part_submit = aps.data(); t.qos_submit = qs.data();
    t.user_qos_exists = uqe.data(); t.user_part_exists = upe.data(); t.acct_qos_exists = aqe.data(); t.acct_part_exists = ape.data();
    t.user_exists = uex.data(); t.acct_exists = aex.data(); t.qos_exists = qex.data();
    return t;
  }
};
static void put(std::vector<cns_usage>& tab, std::vector<uint32_t>& sub, std::vector<uint8_t>& ex, size_t i, const Rec& r) {
  tab[i].cpu_raw = (int64_t)r[0]; tab[i].mem = r[1]; tab[i].wall_sec = (int64_t)r[2]; tab[i].jobs_count = (uint32_t)r[3]; sub[i] = (uint32_t)r[4]; ex[i] = 1;
}
// the maps as dense tables (the bench's user_acct index is the user's: every user has one account)
static Dense dense_of(const Maps& M, uint32_t U, uint32_t A, uint32_t Q, uint32_t Pn) {
  Dense D(U, A, Q, Pn);
  for (const auto& [u, s] : M.user) {
    D.uex[u] = 1;
    for (const auto& [q, r] : s.qos) put(D.uq, D.uqs, D.uqe, (size_t)u * Q + q, r);
    for (const auto& [a, pm] : s.acct_part) for (const auto& [p, r] : pm) put(D.up, D.ups, D.upe, (size_t)u * Pn + p, r);
  }
  for (const auto& [a, s] : M.account) {
    D.aex[a] = 1;
    for (const auto& [q, r] : s.qos) put(D.aq, D.aqs, D.aqe, (size_t)a * Q + q, r);
    for (const auto& [p, r] : s.part) put(D.ap, D.aps, D.ape, (size_t)a * Pn + p, r);
  }
  for (const auto& [q, r] : M.qos) { std::vector<uint8_t> e(Q); put(D.qu, D.qs, e, q, r); D.qex[q] = 1; }
  return D;
}
static bool same_usage(const std::vector<cns_usage>& a, const std::vector<cns_usage>& b) {
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].cpu_raw != b[i].cpu_raw || a[i].mem != b[i].mem || a[i].wall_sec != b[i].wall_sec || a[i].jobs_count != b[i].jobs_count ||
        memcmp(a[i].name_total, b[i].name_total, sizeof a[i].name_total) || memcmp(a[i].class_count, b[i].class_count, sizeof a[i].class_count)) return false;
  return a.size() == b.size();
}
static bool same(const Dense& a, const Dense& b) {
  return same_usage(a.uq, b.uq) && same_usage(a.up, b.up) && same_usage(a.aq, b.aq) && same_usage(a.ap, b.ap) && same_usage(a.qu, b.qu) && a.uqs == b.uqs && a.ups == b.ups &&
         a.aqs == b.aqs && a.aps == b.aps && a.qs == b.qs && a.uqe == b.uqe && a.upe == b.upe && a.aqe == b.aqe && a.ape == b.ape && a.uex == b.uex && a.aex == b.aex && a.qex == b.qex;
}

static int bench(size_t J) {
  cns_config cfg{};
  cfg.abi_version = CNS_ABI_VERSION;
  cns_handle* h = nullptr;
  if (cns_create(&cfg, &h) != 0) { printf("no usable device: %s\n", cns_last_error(nullptr)); return 2; }
  const uint32_t U = 1024, A = 64, Q = 4, Pn = 8;
  std::vector<uint32_t> parent(A);
  for (uint32_t a = 0; a < A; ++a) parent[a] = a < 8 ? CNS_LIM_NONE : a % 8;
  Jobs B;
  B.user.resize(J); B.acct.resize(J); B.qos.resize(J); B.part.resize(J); B.jc.assign(J, 1); B.sc.resize(J); B.cpu.resize(J); B.wall.resize(J); B.mem.resize(J);
  Rng g{0xC4C4C4ull};
  for (size_t j = 0; j < J; ++j) {
    const uint64_t a = g(), b = g();
    B.user[j] = (uint32_t)(a % U); B.acct[j] = B.user[j] % A; B.qos[j] = (uint32_t)((a >> 16) % Q); B.part[j] = (uint32_t)((a >> 24) % Pn);
    B.cpu[j] = (int64_t)(1 + (a >> 40) % 8) * 256; B.mem[j] = (1 + (b % 16)) * G; B.wall[j] = 60 + (int64_t)((b >> 16) % (10 * 86400)); B.sc[j] = (b >> 8) % 10 ? 1 : 0;
  }
  cns_usage_jobs jb{};
  jb.num_jobs = J; jb.user = B.user.data(); jb.user_acct = B.user.data(); jb.account = B.acct.data(); jb.qos = B.qos.data(); jb.partition = B.part.data();
  jb.cpu_raw = B.cpu.data(); jb.mem = B.mem.data(); jb.wall_sec = B.wall.data(); jb.jobs_count = B.jc.data(); jb.submit_count = B.sc.data();
  std::vector<uint16_t> nf(J), of(J), cnf(J), cof(J);
  uint64_t clean = 0;
  cns_usage_out uo{nf.data(), of.data(), &clean};
  int rc = 0;
  // op 1 first: the recovery charge into empty tables.  Then the release of ALL jobs from tables that hold only nine in ten of them
  // (every tenth was never charged), so records trip and are erased inside the burst.
  Maps before_release;
  for (size_t j = 0; j < J; ++j) if (j % 10) cpu_charge(before_release, parent, B, j);
  for (uint32_t op : {CNS_USAGE_CHARGE, CNS_USAGE_RELEASE}) {
    const Maps M0 = op == CNS_USAGE_CHARGE ? Maps{} : before_release;
    const Dense D0 = dense_of(M0, U, A, Q, Pn);
    const cns_usage_tables t = D0.in(U, A, Q, Pn, parent);
    if (cns_usage_set_tables(h, &t) != 0) { printf("cns_usage_set_tables: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
    std::vector<double> h2d, ker, d2h, call, cpu;
    cns_usage_timing tm{};
    for (int rep = 0; rep < 6; ++rep) {                 // one warm-up, then 5; every call starts from the tables as set
      const auto t0 = std::chrono::steady_clock::now();
      if (cns_usage_apply(h, op, &jb, 0, &uo) != 0) { printf("cns_usage_apply: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      cns_usage_get_timing(h, &tm);
      if (rep) { h2d.push_back(tm.h2d_ms); ker.push_back(tm.kernels_ms); d2h.push_back(tm.d2h_ms); call.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    Maps M;
    for (int rep = 0; rep < 5; ++rep) {
      M = M0;
      const auto t0 = std::chrono::steady_clock::now();
      if (op == CNS_USAGE_CHARGE) for (size_t j = 0; j < J; ++j) cpu_charge(M, parent, B, j);
      else for (size_t j = 0; j < J; ++j) cpu_release(M, parent, B, j, cnf[j], cof[j]);
      cpu.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    Dense got(U, A, Q, Pn);
    const cns_usage_tables_out o = got.out();
    cns_usage_get_tables(h, &o);
    const bool same_tables = same(got, dense_of(M, U, A, Q, Pn));
    size_t diff = 0, dirty = 0;
    for (size_t j = 0; j < J; ++j) { diff += op == CNS_USAGE_RELEASE ? (nf[j] != cnf[j] || of[j] != cof[j]) : (nf[j] || of[j]); dirty += (nf[j] | of[j]) != 0; }
    printf("usage bench %s: %zu jobs, %u users, %u accounts, %u QoS, %u partitions: h2d_ms %.3f  kernels_ms %.3f  d2h_ms %.3f  call_ms %.3f  items %llu  records %llu  "
           "cpu_loop_ms %.3f (one thread, unordered_map; median of 5)  jobs with a message %zu  differing jobs %zu  tables %s\n",
           op == CNS_USAGE_CHARGE ? "charge (recovery)" : "release (burst)", J, U, A, Q, Pn, median(h2d), median(ker), median(d2h), median(call), (unsigned long long)tm.items,
           (unsigned long long)tm.records, median(cpu), dirty, diff, same_tables ? "equal" : "DIFFER");
    if (diff || !same_tables || clean != J - dirty) rc = 1;
  }
  cns_destroy(h);
  return rc;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--bench")) return bench(argc > 2 ? (size_t)atoll(argv[2]) : (size_t)1000000);
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  GpuNodeSelectionAlgo algo(0);
  if (no_gpu) {
    if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
    AccountMetaSnapshot meta = start();
    std::vector<Report> rep;
    CHECK(!algo.ReleaseMetaResources(&meta, {Delta::FreeMetaSubmitResource("ann", "lab", "normal", "p0", 1)}, &rep) && !algo.Ok() && algo.LastStatus() != 0);
    CHECK(!algo.ChargeMetaResources(&meta, {Delta::MallocMetaSubmitResource("ann", "lab", "normal", "p0", 1)}) && !algo.Ok());
    CHECK(is(meta.user_meta["ann"].qos_to_resource_map["normal"], 4, 8, 2, 3, 7200));
    printf("no device: ReleaseMetaResources refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
    return g_fail ? 1 : 0;
  }
  if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  return hand_cases(algo) ? 1 : 0;
}
