// Drives GpuNodeSelectionAlgo::CheckSubmitLimits (include/crane_gpu_submit/submit_limits.h): hand-derived cases at string level — the
// reference's CraneErrCode names, the rewritten time limit, the snapshot written back — and, with --bench, a measurement of
// cns_check_submissions against a single-threaded loop in this file that restates AccountMetaContainer.cpp:75-153 and :694-889 over the same
// dense arrays on the same host.
//   test_submit_adapter            -> needs an MI355X, exit 0 on success
//   test_submit_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_submit_adapter --bench [jobs]   -> 1 M submissions in arrival order over 1024 users, 64 accounts (8 roots x 7 children), 4 QoS and
//                                    8 partitions (the shape of config C4's tables) with submit limits, once with unit counts and once with
//                                    10 % array jobs: the device call by stage, rounds, ordered_fallback, the CPU loop; one warm-up, median
//                                    of 5.  Asserted there: the device's codes, time limits and counters equal the loop's.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_submit/submit_limits.h"

using namespace crane;

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  return m;
}

static PdJobInScheduler job(const std::string& user, const std::string& account, const std::string& qos, int64_t tl = 600, double cpu = 1) {
  PdJobInScheduler j;
  j.partition_id = "p0";
  j.username = user; j.account = account; j.qos = qos;
  j.time_limit = tl;
  j.req_task_res_view.cpu_count = cpu_t(cpu);
  j.req_task_res_view.memory_bytes = G;
  j.node_num = 1; j.ntasks = 1;
  return j;
}

static int hand_cases(GpuNodeSelectionAlgo& algo) {
  ClusterSnapshot snap;
  snap.craned_metas = {node("n0", 8, 16), node("n1", 8, 16)};
  snap.partitions = {{"p0", {"n0", "n1"}}};
  algo.SetClusterSnapshot(snap);
  CHECK(algo.Ok());
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }

  // accounts: lab -> dept (root); users: ann (lab, with a partition limit of 2 submitted jobs on p0), bob (lab), eve (no account)
  // QoS: normal (nothing limited), tight (3 submitted jobs per user, 1 h per job), strict (DenyOnLimit, max_jobs_per_user 0)
  AccountMetaSnapshot meta;
  meta.qos["normal"]; meta.qos["tight"]; meta.qos["strict"];
  meta.qos["tight"].max_submit_jobs_per_user = 3; meta.qos["tight"].max_time_limit_per_job = 3600;
  meta.qos["strict"].deny_on_limit = true; meta.qos["strict"].max_jobs_per_user = 0; meta.qos["strict"].max_time_limit_per_job = 1800;
  meta.account_parent = {{"lab", "dept"}, {"dept", ""}};
  meta.user_accounts["ann"]["lab"]["p0"].max_submit_jobs = 2;
  meta.user_accounts["bob"]["lab"];
  meta.user_accounts["eve"];
  meta.user_meta["ann"].qos_to_resource_map["tight"].submit_jobs_count = 2;
  meta.account_meta["dept"];
  meta.qos_meta["normal"].submit_jobs_count = 7;

  std::vector<PdJobInScheduler> q;
  std::vector<GpuNodeSelectionAlgo::SubmitRequest> rq;
  struct Want { uint8_t code; const char* err; int64_t tl; };
  std::vector<Want> want;
  auto add = [&](PdJobInScheduler j, uint32_t count, bool skip, uint8_t code, const char* err, int64_t tl) {
    q.push_back(std::move(j)); want.push_back({code, err, tl});
    GpuNodeSelectionAlgo::SubmitRequest r; r.count = count; r.skip = skip; rq.push_back(r);
  };
  add(job("ann", "lab", "tight"), 1, false, CNS_SUBMIT_OK, "SUCCESS", 600);                                           // :384 2 + 1 <= 3
  add(job("ann", "lab", "tight"), 1, false, CNS_SUBMIT_MAX_JOB_COUNT_PER_USER, "ERR_MAX_JOB_COUNT_PER_USER", 600);    // :384 3 + 1 > 3
  add(job("ann", "lab", "tight", 7200), 1, false, CNS_SUBMIT_TIME_LIMIT_BEYOND, "ERR_TIME_TIMIT_BEYOND", 7200);       // :120
  add(job("ann", "lab", "normal"), 3, false, CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER, "ERR_PARTITION_MAX_SUBMIT_JOBS_PER_USER", 600);   // :741 3 > 2
  add(job("ann", "lab", "normal"), 2, false, CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER, "ERR_PARTITION_MAX_SUBMIT_JOBS_PER_USER", 600);   // :436 1 + 2 > 2 (job 0)
  add(job("ann", "lab", "normal"), 1, false, CNS_SUBMIT_OK, "SUCCESS", 600);                                          // :436 1 + 1 <= 2
  add(job("bob", "lab", "strict", CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC), 1, false, CNS_SUBMIT_OK, "SUCCESS", 1800);      // bob has no record: :751 skips; :119 rewrites
  add(job("bob", "lab", "strict"), 1, false, CNS_SUBMIT_MAX_JOB_COUNT_PER_USER, "ERR_MAX_JOB_COUNT_PER_USER", 600);   // the record exists now: :392 0 + 1 > 0
  add(job("bob", "dept", "normal"), 1, false, CNS_SUBMIT_USER_ACCOUNT_MISMATCH, "ERR_USER_ACCOUNT_MISMATCH", 600);    // :703
  add(job("zoe", "lab", "normal"), 1, false, CNS_SUBMIT_NOT_CANDIDATE, "ERR_INVALID_USER", 600);                      // the caller's lookups
  add(job("bob", "lab", "gold"), 1, false, CNS_SUBMIT_NOT_CANDIDATE, "ERR_INVALID_QOS", 600);                         // :94
  add(job("bob", "lab", "normal"), 0, false, CNS_SUBMIT_BAD_COUNT, "ERR_INVALID_PARAM", 600);
  add(job("bob", "lab", "normal"), 1, true, CNS_SUBMIT_NOT_CANDIDATE, "", 600);
  for (size_t i = 0; i < q.size(); ++i) rq[i].job = &q[i];

  std::vector<GpuNodeSelectionAlgo::SubmitAnswer> ans;
  cns_submit_timing tm{};
  CHECK(algo.CheckSubmitLimits(rq, &meta, &ans, &tm));
  if (!algo.Ok()) printf("CheckSubmitLimits: %s\n", algo.LastError().c_str());
  CHECK(ans.size() == q.size());
  for (size_t i = 0; i < ans.size(); ++i) {
    const bool ok = ans[i].code == want[i].code && !strcmp(ans[i].crane_err, want[i].err) && ans[i].time_limit == want[i].tl;
    if (!ok) { printf("case %zu: got code %u %s tl %lld, want code %u %s tl %lld\n", i, ans[i].code, ans[i].crane_err, (long long)ans[i].time_limit, want[i].code, want[i].err, (long long)want[i].tl); ++g_fail; }
  }
  CHECK(tm.admitted == 3 && tm.candidates == 8);
  CHECK(q[6].time_limit == 1800 && q[2].time_limit == 7200);   // :119 rewrites an admitted job; a rejected one keeps what it came with
  // the snapshot after MallocMetaSubmitResource: jobs 0, 5 (ann) and 6 (bob) along lab -> dept
  CHECK(meta.user_meta["ann"].qos_to_resource_map["tight"].submit_jobs_count == 3);
  CHECK(meta.user_meta["ann"].qos_to_resource_map["normal"].submit_jobs_count == 1);
  CHECK(meta.user_meta["ann"].account_to_partition_to_resource_map["lab"]["p0"].submit_jobs_count == 2);
  CHECK(meta.user_meta.count("bob") && meta.user_meta["bob"].qos_to_resource_map["strict"].submit_jobs_count == 1);
  CHECK(meta.user_meta["bob"].account_to_partition_to_resource_map["lab"]["p0"].submit_jobs_count == 1);
  CHECK(!meta.user_meta.count("eve") && !meta.user_meta.count("zoe"));
  CHECK(meta.account_meta.count("lab") && meta.account_meta["lab"].qos_to_resource_map["tight"].submit_jobs_count == 1);
  CHECK(meta.account_meta["lab"].partition_to_resource_map["p0"].submit_jobs_count == 3);
  CHECK(meta.account_meta["dept"].partition_to_resource_map["p0"].submit_jobs_count == 3);
  CHECK(meta.account_meta["dept"].qos_to_resource_map["strict"].submit_jobs_count == 1);
  CHECK(meta.qos_meta["normal"].submit_jobs_count == 8 && meta.qos_meta["tight"].submit_jobs_count == 1 && meta.qos_meta["strict"].submit_jobs_count == 1);
  CHECK(meta.qos_meta["normal"].jobs_count == 0);              // the run side's counters are inputs and stay
  // the same call on the snapshot it left: ann's tight record is full, bob exists
  std::vector<GpuNodeSelectionAlgo::SubmitAnswer> again;
  CHECK(algo.CheckSubmitLimits({rq[0], rq[6]}, &meta, &again) && again.size() == 2);
  if (again.size() == 2) CHECK(again[0].code == CNS_SUBMIT_MAX_JOB_COUNT_PER_USER && again[1].code == CNS_SUBMIT_MAX_JOB_COUNT_PER_USER);
  std::vector<GpuNodeSelectionAlgo::SubmitAnswer> none;
  CHECK(algo.CheckSubmitLimits({}, &meta, &none) && none.empty());
  printf("hand cases: %zu jobs, %d failures\n", q.size(), g_fail);
  return g_fail;
}

// ---- --bench: the dense arrays, the loop that restates the reference, the device call ------------------------------------------------------

struct View { int64_t cpu; uint64_t mem; uint64_t nt[CNS_MAX_GRES_NAMES]; uint64_t cc[CNS_MAX_GRES_CLASSES]; };

static bool check_gres(const View& r, const cns_tres& lim, const cns_gres_layout& lay) {   // :1030-1050, canonical order
  for (uint32_t n = 0; n < CNS_MAX_GRES_NAMES; ++n) {
    bool present = r.nt[n] > 0;
    for (uint32_t g = 0; g < lay.num_classes; ++g) present = present || (lay.class_name[g] == n && r.cc[g] > 0);
    if (!present) continue;
    if (!(lim.name_mask >> n & 1)) return true;
    if (r.nt[n] > lim.name_total[n]) return false;
    for (uint32_t g = 0; g < lay.num_classes; ++g) {
      if (lay.class_name[g] != n || !r.cc[g]) continue;
      if (!(lim.class_mask >> g & 1)) return true;
      if (r.cc[g] > lim.class_count[g]) return false;
    }
  }
  return true;
}
static bool check_tres(const View& r, const cns_tres& lim, const cns_gres_layout& lay) {   // :345-360
  return r.cpu <= lim.cpu_raw && r.mem <= lim.mem && check_gres(r, lim, lay);
}
static View plus(View r, const cns_usage& u) {
  r.cpu += u.cpu_raw; r.mem += u.mem;
  for (uint32_t n = 0; n < CNS_MAX_GRES_NAMES; ++n) r.nt[n] += u.name_total[n];
  for (uint32_t g = 0; g < CNS_MAX_GRES_CLASSES; ++g) r.cc[g] += u.class_count[g];
  return r;
}

struct Tables {
  uint32_t U, UA, A, Q, Pn;
  cns_gres_layout lay{};
  std::vector<cns_submit_qos> qos;
  std::vector<cns_submit_part_limit> pl;
  std::vector<uint32_t> parent, upl, apl;
  std::vector<cns_usage> uq, aq, qu;
  std::vector<uint32_t> uqs, ups, aqs, aps, qs;
  std::vector<uint8_t> uex, aex, qex;
};
struct Batch {
  std::vector<uint32_t> part, k, nt, user, ua, acct, qos, count;
  std::vector<int64_t> tl, tcpu;
  std::vector<uint64_t> nmem, tmem;
};

// TryMallocMetaSubmitResource + MallocMetaSubmitResource, one job after the other (the bench's jobs: no GRES, no overflow, no skip)
static void cpu_loop(const Tables& T, const Batch& B, Tables& S, std::vector<uint8_t>& code, std::vector<int64_t>& tlo) {
  const size_t J = B.user.size();
  const uint32_t Q = T.Q, Pn = T.Pn;
  for (size_t j = 0; j < J; ++j) {
    const uint32_t count = B.count[j], u = B.user[j], x = B.ua[j], qi = B.qos[j], p = B.part[j];
    const cns_submit_qos& q = T.qos[qi];
    int64_t tl = B.tl[j];
    tlo[j] = tl;
    View req{};
    req.cpu = B.tcpu[j] * (int64_t)B.nt[j]; req.mem = B.nmem[j] * B.k[j] + B.tmem[j] * B.nt[j];
    View use = req;
    use.cpu *= count; use.mem *= count;                                                                          // :97
    uint8_t c = 0;
    if (count == 0) c = CNS_SUBMIT_BAD_COUNT;
    else if (count > q.max_submit_jobs_per_user) c = CNS_SUBMIT_MAX_JOB_COUNT_PER_USER;                          // :99
    else if (count > q.max_submit_jobs_per_account) c = CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT;                    // :102
    else if (count > q.max_submit_jobs) c = CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED;                                   // :105
    else if (use.cpu > q.max_cpus_per_user_raw) c = CNS_SUBMIT_CPUS_PER_TASK_BEYOND;                             // :108
    else if (!check_tres(use, q.max_tres_per_user, T.lay) || !check_tres(use, q.max_tres_per_account, T.lay) || !check_tres(use, q.max_tres, T.lay))
      c = CNS_SUBMIT_TRES_PER_JOB_BEYOND;                                                                        // :111-114
    else if (tl >= CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC) tl = q.max_time_limit_per_job_sec;                         // :118-119
    else if (tl > q.max_time_limit_per_job_sec) c = CNS_SUBMIT_TIME_LIMIT_BEYOND;                                // :120
    tlo[j] = tl;
    auto entity = [&](bool is_user, uint32_t submit_q, const cns_usage& val, uint32_t submit_p, const cns_submit_part_limit* lim) -> uint8_t {
      const uint32_t max_submit = is_user ? q.max_submit_jobs_per_user : q.max_submit_jobs_per_account;
      if ((uint64_t)submit_q + count > max_submit) return is_user ? CNS_SUBMIT_MAX_JOB_COUNT_PER_USER : CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT;   // :384
      if (q.deny_on_limit) {
        if ((uint64_t)val.jobs_count + 1 > (is_user ? q.max_jobs_per_user : q.max_jobs_per_account))             // :392
          return is_user ? CNS_SUBMIT_MAX_JOB_COUNT_PER_USER : CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT;
        const View s = plus(req, val);
        if (is_user) {
          if (s.cpu > q.max_cpus_per_user_raw) return CNS_SUBMIT_CPUS_PER_TASK_BEYOND;                           // :401
          if (!check_tres(s, q.max_tres_per_user, T.lay)) return CNS_SUBMIT_MAX_TRES_PER_USER_BEYOND;            // :403
        } else if (!check_tres(s, q.max_tres_per_account, T.lay)) return CNS_SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND; // :406
      }
      if (lim && max_submit == UINT32_MAX && (uint64_t)submit_p + count > lim->max_submit_jobs)                  // :420-477
        return is_user ? CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER : CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT;
      return 0;
    };
    auto static_part = [&](bool is_user, const cns_submit_part_limit* lim) -> uint8_t {                          // :715-749 / :784-819
      if (!lim) return 0;
      if (!check_tres(req, lim->max_tres_per_job, T.lay)) return CNS_SUBMIT_PARTITION_TRES_PER_JOB_BEYOND;
      if (q.max_time_limit_per_job_sec == CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC && tl > lim->max_wall_duration_per_job_sec) return CNS_SUBMIT_PARTITION_TIME_BEYOND;
      if ((is_user ? q.max_submit_jobs_per_user : q.max_submit_jobs_per_account) == UINT32_MAX && count > lim->max_submit_jobs)
        return is_user ? CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER : CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT;
      return 0;
    };
    if (!c) {
      if (x == CNS_LIM_NONE) c = CNS_SUBMIT_USER_ACCOUNT_MISMATCH;                                               // :703
      else {
        const uint32_t li = T.upl[(size_t)x * Pn + p];
        const cns_submit_part_limit* lim = li == CNS_LIM_NONE ? nullptr : &T.pl[li];
        c = static_part(true, lim);
        if (!c && S.uex[u]) c = entity(true, S.uqs[(size_t)u * Q + qi], T.uq[(size_t)u * Q + qi], S.ups[(size_t)x * Pn + p], lim);   // :751
      }
    }
    for (uint32_t a = B.acct[j]; !c && a != CNS_LIM_NONE; a = T.parent[a]) {                                     // :770
      const uint32_t li = T.apl[(size_t)a * Pn + p];
      const cns_submit_part_limit* lim = li == CNS_LIM_NONE ? nullptr : &T.pl[li];
      c = static_part(false, lim);
      if (!c && S.aex[a]) c = entity(false, S.aqs[(size_t)a * Q + qi], T.aq[(size_t)a * Q + qi], S.aps[(size_t)a * Pn + p], lim);   // :821
    }
    if (!c && S.qex[qi]) {                                                                                       // :841
      const cns_usage& val = T.qu[qi];
      if ((uint64_t)S.qs[qi] + count > q.max_submit_jobs) c = CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED;                 // :844
      else if (q.deny_on_limit) {
        if ((uint64_t)val.jobs_count + 1 > q.max_jobs) c = CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED;                    // :854
        else if (q.max_wall_sec > 0 && val.wall_sec + tl > q.max_wall_sec) c = CNS_SUBMIT_TIME_LIMIT_BEYOND;     // :863-864
        else if (!check_tres(plus(req, val), q.max_tres, T.lay)) c = CNS_SUBMIT_TRES_PER_JOB_BEYOND;             // :877
      }
    }
    code[j] = c;
    if (c) continue;
    S.uex[u] = 1; S.uqs[(size_t)u * Q + qi] += count; S.ups[(size_t)x * Pn + p] += count;                        // :1086-1104
    for (uint32_t a = B.acct[j]; a != CNS_LIM_NONE; a = T.parent[a]) { S.aex[a] = 1; S.aqs[(size_t)a * Q + qi] += count; S.aps[(size_t)a * Pn + p] += count; }
    S.qex[qi] = 1; S.qs[qi] += count;                                                                            // :1118-1123
  }
}

static int bench(size_t J) {
  cns_config cfg{};
  cfg.abi_version = CNS_ABI_VERSION;
  cns_handle* h = nullptr;
  if (cns_create(&cfg, &h) != 0) { printf("no usable device: %s\n", cns_last_error(nullptr)); return 2; }
  Tables T;
  T.U = T.UA = 1024; T.A = 64; T.Q = 4; T.Pn = 8;
  const uint32_t U = T.U, A = T.A, Q = T.Q, Pn = T.Pn;
  auto unlimited = [] { cns_tres t{}; t.cpu_raw = CNS_LIM_UNLIMITED_CPU_RAW; t.mem = 1ull << 60; return t; };
  T.qos.assign(Q, cns_submit_qos{});
  const uint32_t per_user = (uint32_t)std::max<size_t>(J / (U * Q), 1);   // jobs a (user, qos) pair sees on average
  for (uint32_t i = 0; i < Q; ++i) {
    cns_submit_qos& q = T.qos[i];
    q.max_submit_jobs_per_user = q.max_submit_jobs_per_account = q.max_submit_jobs = q.max_jobs_per_user = q.max_jobs_per_account = q.max_jobs = UINT32_MAX;
    q.max_cpus_per_user_raw = CNS_LIM_UNLIMITED_CPU_RAW; q.max_time_limit_per_job_sec = CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC;
    q.max_tres = q.max_tres_per_user = q.max_tres_per_account = unlimited();
  }
  T.qos[0].max_submit_jobs_per_user = per_user; T.qos[0].deny_on_limit = 1; T.qos[0].max_jobs_per_user = 96; T.qos[0].max_tres_per_account.cpu_raw = 3000 * 256;
  T.qos[1].max_submit_jobs_per_user = 2 * per_user; T.qos[1].max_submit_jobs_per_account = per_user * 24; T.qos[1].max_time_limit_per_job_sec = 7 * 86400;
  T.qos[2].max_submit_jobs = (uint32_t)(J / 5); T.qos[2].deny_on_limit = 1; T.qos[2].max_wall_sec = 1ll << 40;
  T.pl.assign(1, cns_submit_part_limit{});
  T.pl[0].max_submit_jobs = per_user * 12; T.pl[0].max_wall_duration_per_job_sec = 30 * 86400; T.pl[0].max_tres_per_job = unlimited();
  T.parent.resize(A);
  for (uint32_t a = 0; a < A; ++a) T.parent[a] = a < 8 ? CNS_LIM_NONE : a % 8;
  T.upl.assign((size_t)U * Pn, CNS_LIM_NONE);
  T.apl.resize((size_t)A * Pn);
  for (size_t i = 0; i < T.apl.size(); ++i) T.apl[i] = (i / Pn) % 4 == 3 ? 0 : CNS_LIM_NONE;
  T.uq.assign((size_t)U * Q, cns_usage{}); T.aq.assign((size_t)A * Q, cns_usage{}); T.qu.assign(Q, cns_usage{});
  Rng r{0x5EEDull};
  for (auto& u : T.uq) { u.jobs_count = (uint32_t)(r() % 100); u.cpu_raw = (int64_t)(r() % 64) * 256; }
  for (auto& u : T.aq) u.cpu_raw = (int64_t)(r() % 2999) * 256;
  T.uqs.assign((size_t)U * Q, 0); T.ups.assign((size_t)U * Pn, 0); T.aqs.assign((size_t)A * Q, 0); T.aps.assign((size_t)A * Pn, 0); T.qs.assign(Q, 0);
  T.uex.resize(U); T.aex.resize(A); T.qex.assign(Q, 1);
  for (auto& e : T.uex) e = r() % 2;
  for (auto& e : T.aex) e = r() % 4 != 0;
  T.qex[3] = 0;
  cns_submit_tables ct{};
  ct.num_users = U; ct.num_user_accts = U; ct.num_accounts = A; ct.num_qos = Q; ct.num_partitions = Pn; ct.num_part_limits = 1;
  ct.qos = T.qos.data(); ct.acct_parent = T.parent.data(); ct.part_limits = T.pl.data(); ct.user_part_limit = T.upl.data(); ct.acct_part_limit = T.apl.data();
  ct.user_qos = T.uq.data(); ct.acct_qos = T.aq.data(); ct.qos_usage = T.qu.data();
  ct.user_exists = T.uex.data(); ct.acct_exists = T.aex.data(); ct.qos_exists = T.qex.data();
  int rc = 0;
  for (int arrays = 0; arrays < 2 && !rc; ++arrays) {
    Batch B;
    B.part.resize(J); B.k.assign(J, 1); B.nt.resize(J); B.user.resize(J); B.ua.resize(J); B.acct.resize(J); B.qos.resize(J); B.count.assign(J, 1);
    B.tl.resize(J); B.tcpu.resize(J); B.nmem.assign(J, 0); B.tmem.resize(J);
    Rng g{0xC4C4C4ull + (uint64_t)arrays};
    for (size_t j = 0; j < J; ++j) {
      const uint64_t a = g(), b = g();
      B.user[j] = B.ua[j] = (uint32_t)(a % U); B.acct[j] = B.user[j] % A; B.qos[j] = (uint32_t)((a >> 16) % Q); B.part[j] = (uint32_t)((a >> 24) % Pn);
      B.nt[j] = 1 + (uint32_t)((a >> 32) % 4); B.tcpu[j] = (int64_t)(1 + (a >> 40) % 8) * 256; B.tmem[j] = (1 + (b % 16)) * G;
      B.tl[j] = (b >> 8) % 50 == 0 ? CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC : 60 + (int64_t)((b >> 16) % (10 * 86400));
      if (arrays && (b >> 40) % 10 == 0) B.count[j] = 2 + (uint32_t)((b >> 44) % 198);
    }
    cns_job_soa js{};
    js.num_jobs = J; js.partition = B.part.data(); js.time_limit_sec = B.tl.data(); js.node_mem = B.nmem.data(); js.task_cpu_raw = B.tcpu.data();
    js.task_mem = B.tmem.data(); js.node_num = B.k.data(); js.ntasks = B.nt.data();
    cns_submit_keys ks{B.user.data(), B.ua.data(), B.acct.data(), B.qos.data(), B.count.data(), nullptr};
    std::vector<uint8_t> code(J), ccode(J);
    std::vector<int64_t> tlo(J), ctlo(J);
    uint64_t adm = 0;
    cns_submit_out so{code.data(), tlo.data(), &adm};
    std::vector<double> h2d, prep, admit, d2h, call, cpu;
    cns_submit_timing tm{};
    for (int rep = 0; rep < 6; ++rep) {                 // one warm-up, then 5; every call starts from the tables as set
      if (rep == 0 && cns_set_submit_limits(h, &ct) != 0) { printf("cns_set_submit_limits: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
      const auto t0 = std::chrono::steady_clock::now();
      if (cns_check_submissions(h, &js, &ks, 0, &so) != 0) { printf("cns_check_submissions: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      cns_get_submit_timing(h, &tm);
      if (rep) { h2d.push_back(tm.h2d_ms); prep.push_back(tm.prep_ms); admit.push_back(tm.admit_ms); d2h.push_back(tm.d2h_ms); call.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    Tables S = T;
    for (int rep = 0; rep < 5; ++rep) {
      S = T;
      const auto t0 = std::chrono::steady_clock::now();
      cpu_loop(T, B, S, ccode, ctlo);
      cpu.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::vector<uint32_t> uqs(S.uqs.size()), ups(S.ups.size()), aqs(S.aqs.size()), aps(S.aps.size()), qs(S.qs.size());
    std::vector<uint8_t> uex(U), aex(A), qex(Q);
    cns_get_submit_usage(h, uqs.data(), ups.data(), aqs.data(), aps.data(), qs.data(), uex.data(), aex.data(), qex.data());
    size_t diff = 0, cpu_adm = 0;
    for (size_t j = 0; j < J; ++j) { diff += code[j] != ccode[j] || tlo[j] != ctlo[j]; cpu_adm += ccode[j] == 0; }
    const bool same_state = uqs == S.uqs && ups == S.ups && aqs == S.aqs && aps == S.aps && qs == S.qs && uex == S.uex && aex == S.aex && qex == S.qex;
    printf("submit bench %s: %zu jobs, %u users, %u accounts, %u QoS, %u partitions: h2d_ms %.3f  prep_ms %.3f  admit_ms %.3f  d2h_ms %.3f  call_ms %.3f  "
           "rounds %u  ordered_fallback %u  cpu_loop_ms %.3f (one thread; median of 5)  admitted %llu of %llu candidates (cpu loop: %zu)  differing jobs %zu  counters %s\n",
           arrays ? "with 10 % array jobs" : "unit counts", J, U, A, Q, Pn, median(h2d), median(prep), median(admit), median(d2h), median(call), tm.rounds, tm.ordered_fallback,
           median(cpu), (unsigned long long)adm, (unsigned long long)tm.candidates, cpu_adm, diff, same_state ? "equal" : "DIFFER");
    if (diff || !same_state || adm != cpu_adm) rc = 1;
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
    std::vector<GpuNodeSelectionAlgo::SubmitAnswer> ans;
    AccountMetaSnapshot meta;
    PdJobInScheduler j = job("ann", "lab", "normal");
    GpuNodeSelectionAlgo::SubmitRequest r; r.job = &j;
    CHECK(!algo.CheckSubmitLimits({r}, &meta, &ans) && ans.empty() && !algo.Ok() && algo.LastStatus() != 0);
    printf("no device: CheckSubmitLimits refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
    return g_fail ? 1 : 0;
  }
  if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  return hand_cases(algo) ? 1 : 0;
}
