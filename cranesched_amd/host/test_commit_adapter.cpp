// Drives GpuNodeSelectionAlgo::CommitCheck (include/crane_gpu_commit/commit_check.h): a hand-made cycle at string level — the reason
// strings of JobScheduler.cpp:1518-1552 in job->reason, a job that is gone, unknown craned and reservation names, a cycle with
// preemption, and CheckAndMallocMetaResource behind it — and, with --bench, a measurement against a single-threaded loop that restates
// :1464-1555 over the same dense arrays on the same host.
//   test_commit_adapter            -> needs an MI355X, exit 0 on success
//   test_commit_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_commit_adapter --bench [jobs] [nodes]   -> 65 536 nodes in 8 partitions and 1 M jobs (the shape of config C4, 90 % one-node jobs) drawn
//                                    by the driver's own generator; one NodeSelect, then the call once without events and once with one event
//                                    that names 4 096 nodes of one partition: kernel_ms, the whole call, the CPU loop; one warm-up, median of 7.
//                                    Nothing is asserted there but the agreement of the codes.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_commit/commit_check.h"

using namespace crane;
using Event = GpuNodeSelectionAlgo::ResReduceEvent;
using ResvNow = GpuNodeSelectionAlgo::ResvMetaNow;

static const TimeSec NOW = 1000000;

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  m.alive = true;
  return m;
}

static std::unique_ptr<PdJobInScheduler> job(job_id_t id, const std::string& part, double cpu, int64_t limit, uint32_t k = 1) {
  auto j = std::make_unique<PdJobInScheduler>();
  j->job_id = id;
  j->partition_id = part;
  j->time_limit = limit;
  j->req_task_res_view.cpu_count = cpu_t(cpu);
  j->req_task_res_view.memory_bytes = G;
  j->node_num = k;
  j->ntasks = k;
  j->username = "alice"; j->account = "lab"; j->qos = "normal";
  return j;
}

static Event node_event(TimeSec t, std::vector<CranedId> ids) { Event e; e.affected_resources = std::make_pair(t, std::move(ids)); return e; }
static Event resv_event(const std::string& name) { Event e; e.affected_resources = name; return e; }

static int hand_cases(GpuNodeSelectionAlgo& algo) {
  // p0 = {n0..n3}, p1 = {n4 n5}, 4 cores / 16 GiB each; reservation "r0" takes n4 and n5 whole until NOW+5000
  ClusterSnapshot snap;
  for (int i = 0; i < 6; ++i) snap.craned_metas.push_back(node("n" + std::to_string(i), 4, 16));
  snap.partitions = {{"p0", {"n0", "n1", "n2", "n3"}}, {"p1", {"n4", "n5"}}};
  ResvMeta rv;
  rv.name = "r0"; rv.start_time = NOW - 10; rv.end_time = NOW + 5000;
  for (const char* n : {"n4", "n5"}) rv.res_total[n] = snap.craned_metas[4].res_total;
  snap.reservations.push_back(rv);
  algo.SetClusterSnapshot(snap);
  CHECK(algo.Ok());
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }

  std::vector<std::unique_ptr<PdJobInScheduler>> pd;
  pd.push_back(job(1, "p0", 1, 101));              // 0: loses its node one second before its end
  pd.push_back(job(2, "p0", 1, 100));              // 1: change == end
  pd.push_back(job(3, "p0", 1, 500));              // 2: cancelled meanwhile
  pd.push_back(job(4, "p1", 1, 100, 2));           // 3: in r0, on n4 and n5
  pd.back()->reservation = "r0";
  pd.push_back(job(5, "p0", 4, 100, 4));           // 4: four whole nodes are not free: the cycle leaves a reason
  pd.push_back(job(6, "p0", 1, 50));               // 5
  std::vector<std::unique_ptr<RnJobInScheduler>> none;
  std::vector<uint8_t> codes;
  CHECK(!algo.CommitCheck({}, nullptr, {}, {}, &codes) && !algo.Ok() && codes.empty());   // before a cycle
  algo.NodeSelect(NOW, none, pd);
  CHECK(algo.Ok());
  for (int i : {0, 1, 2, 3, 5}) CHECK(pd[i]->is_scheduled() && pd[i]->start_time == NOW);
  CHECK(!pd[4]->reason.empty());
  const std::string kept = pd[4]->reason;

  const std::unordered_set<job_id_t> pending = {1, 2, 4, 5, 6};
  std::vector<CranedId> p0_and_ghosts = {"n0", "ghost-a", "n1", "n2", "n3", "ghost-b"};
  ResvNow r0_now{NOW + 5000, {"n4", "ghost-c"}};   // n5 left the reservation
  auto lookup = [&](const std::string& name) -> const ResvNow* { return name == "r0" ? &r0_now : nullptr; };
  std::vector<Event> ev = {node_event(NOW + 100, p0_and_ghosts), node_event(GpuNodeSelectionAlgo::kInfinitePast, {"ghost-a", "n4", "n5"}),
                           resv_event("r0"), resv_event("never-heard-of"), resv_event("r0")};
  double ms = -1;
  CHECK(algo.CommitCheck(ev, lookup, {}, pending, &codes, &ms));
  if (!algo.Ok()) printf("CommitCheck: %s\n", algo.LastError().c_str());
  CHECK(ms >= 0 && codes.size() == 6 && algo.LastOrder().size() == 6);
  const std::vector<uint8_t> want = {CNS_COMMIT_RESOURCE_CHANGED, CNS_COMMIT_OK, CNS_COMMIT_GONE, CNS_COMMIT_RESV_CHANGED, CNS_COMMIT_NOT_STARTED, CNS_COMMIT_OK};
  CHECK(codes == want);
  CHECK(pd[0]->reason == "Resource changed" && pd[1]->reason.empty() && pd[2]->reason.empty() && pd[3]->reason == "Reservation changed");
  CHECK(pd[4]->reason == kept && pd[5]->reason.empty());

  // the admission behind it: one slot per user; the dropped job 1 does not take it, job 2 does, job 6 is refused.  (The gone job 3 is
  // the caller's to drop, :1493-1500: it is taken out of the vector here.)
  {
    AccountMetaSnapshot meta;
    Qos normal;
    normal.max_jobs_per_user = 1;
    meta.qos["normal"] = normal;
    meta.account_parent = {{"root", ""}, {"lab", "root"}};
    meta.user_accounts["alice"]["lab"];
    meta.user_meta["alice"].qos_to_resource_map["normal"];
    for (const char* a : {"root", "lab"}) meta.account_meta[a].qos_to_resource_map["normal"];
    meta.qos_meta["normal"];
    pd[2]->reason = "cancelled";
    std::vector<std::string> res;
    algo.CheckAndMallocMetaResource(meta, pd, res);
    CHECK(algo.Ok());
    CHECK(res.size() == 6 && res[0] == "Resource changed" && res[1].empty() && res[3] == "Reservation changed" && res[4] == kept);
    CHECK(res[5] == "QosJobsResourceLimit");
    CHECK(meta.user_meta["alice"].qos_to_resource_map["normal"].jobs_count == 1);
    pd[2]->reason.clear();
  }

  // the other reservation outcomes; only unknown names: nobody is touched
  for (auto& j : pd) if (j.get() != pd[4].get()) j->reason.clear();
  CHECK(algo.CommitCheck({resv_event("r0")}, [](const std::string&) -> const ResvNow* { return nullptr; }, {}, pending, &codes));
  CHECK(codes[3] == CNS_COMMIT_RESV_DELETED && pd[3]->reason == "Reservation deleted" && codes[0] == CNS_COMMIT_OK && pd[0]->reason.empty());
  ResvNow early{NOW + 99, {"n4", "n5"}};
  CHECK(algo.CommitCheck({resv_event("r0")}, [&](const std::string&) -> const ResvNow* { return &early; }, {}, pending, &codes));
  CHECK(codes[3] == CNS_COMMIT_RESV_ENDS_EARLY && pd[3]->reason == "Resource");
  pd[3]->reason.clear();
  ResvNow whole{NOW + 100, {"n5", "n4"}};
  CHECK(algo.CommitCheck({resv_event("r0"), node_event(GpuNodeSelectionAlgo::kInfinitePast, {"ghost-a", "ghost-b"})},
                         [&](const std::string&) -> const ResvNow* { return &whole; }, {}, pending, &codes));
  CHECK(codes[3] == CNS_COMMIT_OK && codes[0] == CNS_COMMIT_OK && codes[2] == CNS_COMMIT_GONE);
  for (int i : {0, 1, 2, 3, 5}) CHECK(pd[i]->reason.empty());

  // a cycle with preemption: the victim still in the running map -> "Waiting for Preemption"
  {
    ClusterSnapshot s2;
    s2.craned_metas = {node("m0", 2, 8)};
    s2.partitions = {{"p0", {"m0"}}};
    s2.preempt_enabled = true;
    s2.qos_preempt = {{"high", {"low"}}, {"low", {}}};
    algo.SetClusterSnapshot(s2);
    CHECK(algo.Ok());
    std::vector<std::unique_ptr<RnJobInScheduler>> rn;
    auto r = std::make_unique<RnJobInScheduler>();
    r->job_id = 50; r->qos = "low"; r->qos_priority = 1; r->start_time = NOW - 100; r->end_time = NOW + 500;
    r->allocated_res["m0"] = s2.craned_metas[0].res_total;
    r->allocated_res["m0"].memory_bytes = r->allocated_res["m0"].memory_sw_bytes = 2 * G;
    rn.push_back(std::move(r));
    std::vector<std::unique_ptr<PdJobInScheduler>> q;
    q.push_back(job(7, "p0", 2, 100));
    q.back()->qos = "high"; q.back()->qos_priority = 10;
    algo.NodeSelect(NOW, rn, q);
    CHECK(algo.Ok());
    if (!algo.Ok()) printf("NodeSelect with preemption: %s\n", algo.LastError().c_str());
    CHECK(q[0]->is_scheduled() && q[0]->preempted_jobs.size() == 1);
    CHECK(algo.CommitCheck({}, nullptr, {50}, {7}, &codes));
    CHECK(codes.size() == 1 && codes[0] == CNS_COMMIT_WAITING_PREEMPTION && q[0]->reason == "Waiting for Preemption");
    q[0]->reason.clear();
    CHECK(algo.CommitCheck({}, nullptr, {51}, {7}, &codes));
    CHECK(codes.size() == 1 && codes[0] == CNS_COMMIT_OK && q[0]->reason.empty());
  }
  printf("hand cases: %d failures\n", g_fail);
  return g_fail;
}

static int bench(GpuNodeSelectionAlgo& algo, size_t J, int N) {
  const int P = 8;
  ClusterSnapshot snap;
  std::vector<std::vector<CranedId>> parts(P);
  Rng r{0x5EEDull};
  for (int i = 0; i < N; ++i) {
    char name[16];
    snprintf(name, sizeof name, "cn%05d", i);
    const int cores = 16 << (r() % 3);
    snap.craned_metas.push_back(node(name, cores, (uint64_t)cores * 4));
    parts[i % P].push_back(name);
  }
  for (int p = 0; p < P; ++p) snap.partitions.push_back({"P" + std::to_string(p), parts[p]});
  algo.SetClusterSnapshot(snap);
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }
  std::vector<std::unique_ptr<PdJobInScheduler>> q;
  Rng g{0xC4C4C4ull};
  std::unordered_set<job_id_t> pending;
  for (size_t j = 0; j < J; ++j) {
    const uint64_t a = g();
    q.push_back(job((job_id_t)(j + 1), "P" + std::to_string(a % P), (double)(1 << ((a >> 8) % 3)), 60 + (int64_t)((a >> 16) % 7200),
                    (a >> 32) % 10 == 0 ? 2 + (uint32_t)((a >> 40) % 7) : 1));
    pending.insert((job_id_t)(j + 1));
  }
  std::vector<std::unique_ptr<RnJobInScheduler>> none;
  algo.NodeSelect(NOW, none, q);
  if (!algo.Ok()) { printf("NodeSelect: %s\n", algo.LastError().c_str()); return 1; }
  // the dense arrays of the host loop (outside every timed region): node indices of the placements, ends, started
  std::unordered_map<std::string, uint32_t> idx;
  for (int i = 0; i < N; ++i) idx[snap.craned_metas[i].craned_id] = (uint32_t)i;
  std::vector<uint64_t> off(J + 1, 0);
  std::vector<uint32_t> pn;
  std::vector<int64_t> end(J);
  std::vector<uint8_t> started(J);
  size_t n_started = 0;
  for (size_t j = 0; j < J; ++j) {
    started[j] = q[j]->reason.empty();
    n_started += started[j];
    end[j] = q[j]->start_time + q[j]->time_limit;
    if (started[j]) for (const auto& c : q[j]->craned_ids) pn.push_back(idx.at(c));
    off[j + 1] = pn.size();
  }
  for (int with_event = 0; with_event < 2; ++with_event) {
    std::vector<Event> ev;
    std::vector<uint32_t> ev_idx;
    if (with_event) {
      std::vector<CranedId> ids(parts[0].begin(), parts[0].begin() + std::min<size_t>(4096, parts[0].size()));
      for (const auto& c : ids) ev_idx.push_back(idx.at(c));
      ev.push_back(node_event(NOW + 1800, ids));
    }
    std::vector<uint8_t> codes;
    std::vector<double> kms, call;
    for (int rep = 0; rep < 8; ++rep) {
      double ms = 0;
      const auto t0 = std::chrono::steady_clock::now();
      if (!algo.CommitCheck(ev, nullptr, {}, pending, &codes, &ms)) { printf("CommitCheck: %s\n", algo.LastError().c_str()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      if (rep) { kms.push_back(ms); call.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
      for (auto& j : q) if (j->reason == "Resource changed") j->reason.clear();
    }
    // :1464-1555 on one thread over dense indices: the fold into change[N], then per job the walk over its records (no break)
    std::vector<double> cpu_ms;
    std::vector<uint8_t> cpu_code(J);
    for (int rep = 0; rep < 3; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<int64_t> change(N, INT64_MAX);
      for (uint32_t n : ev_idx) if (change[n] > NOW + 1800) change[n] = NOW + 1800;                   // :1479-1483
      for (size_t j = 0; j < J; ++j) {
        if (!started[j]) { cpu_code[j] = CNS_COMMIT_NOT_STARTED; continue; }                           // :1507-1510
        uint8_t c = CNS_COMMIT_OK;
        for (uint64_t x = off[j]; x < off[j + 1]; ++x) if (change[pn[x]] < end[j]) c = CNS_COMMIT_RESOURCE_CHANGED;   // :1514-1519
        cpu_code[j] = c;
      }
      cpu_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    size_t differ = 0, changed = 0;
    for (size_t j = 0; j < J; ++j) { differ += codes[j] != cpu_code[j]; changed += codes[j] == CNS_COMMIT_RESOURCE_CHANGED; }
    printf("commit bench %s: %zu jobs (%zu started) x %d nodes in %d partitions: kernel_ms %.3f  call_ms %.3f  cpu_loop_ms %.3f (one thread, dense "
           "indices; median of %zu / %zu / %zu)  RESOURCE_CHANGED %zu  codes that differ from the cpu loop %zu\n",
           with_event ? "one event naming 4 096 nodes of one partition" : "no events", J, n_started, N, P, median(kms), median(call), median(cpu_ms),
           kms.size(), call.size(), cpu_ms.size(), changed, differ);
    if (differ) return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  GpuNodeSelectionAlgo algo(0);
  if (no_gpu) {
    if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
    std::vector<uint8_t> codes;
    CHECK(!algo.CommitCheck({}, nullptr, {}, {}, &codes) && codes.empty() && !algo.Ok() && algo.LastStatus() != 0);
    printf("no device: CommitCheck refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
    return g_fail ? 1 : 0;
  }
  if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  if (argc > 1 && !strcmp(argv[1], "--bench"))
    return bench(algo, argc > 2 ? (size_t)atoll(argv[2]) : (size_t)1 << 20, argc > 3 ? atoi(argv[3]) : 65536);
  return hand_cases(algo) ? 1 : 0;
}
