// Drives the adapter's side of include/crane_gpu_running/running_attrs.h: GpuNodeSelectionAlgo::UseResidentAttrs (SeedRunning /
// AdvanceRunning hand the running jobs' attributes in) and a GpuMultiFactorPriority that BORROWS the algorithm object's engine and
// ranks the pending queue from the device ledger.  Over several consecutive cycles with jobs ending and starting, the borrowed sorter —
// handed an EMPTY running_jobs vector every time: nothing of the vector can have been read — must give the order, and the priorities
// bit for bit, of a GpuMultiFactorPriority with a handle of its own fed the same running jobs in ledger order.
//   test_running_attrs_adapter            -> needs an MI355X, exit 0 on success
//   test_running_attrs_adapter --no-gpu   -> the loud "no device" behaviour instead
// (The measurement at the shape of profiles/r16_running_ledger.txt is tools/prio_resident_bench.py, on the C ABI through the binding.)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"

using namespace crane;

static const TimeSec NOW = 1000000;
static const TimeSec STEP = 600;
static const char* const ACCOUNTS[] = {"physics", "chem", "bio", "ops"};

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  m.alive = true;
  return m;
}

static std::unique_ptr<PdJobInScheduler> job(job_id_t id, const std::string& part, int cpu, int64_t limit, uint32_t k, int i, TimeSec now) {
  auto j = std::make_unique<PdJobInScheduler>();
  j->job_id = id;
  j->partition_id = part;
  j->time_limit = limit;
  j->req_task_res_view.cpu_count = cpu_t(cpu);
  j->req_task_res_view.memory_bytes = G;
  j->node_num = k;
  j->ntasks = k;
  j->req_total_res_view.cpu_count = cpu_t(cpu * (int)k);
  j->req_total_res_view.memory_bytes = (uint64_t)k * G;
  j->submit_time = now - 100 - 977 * (i % 7);
  j->qos = "normal"; j->qos_priority = (uint32_t)(10 * (i % 4)); j->partition_priority = part == "p0" ? 5 : 1;
  j->account = ACCOUNTS[(i * 3 + (int)(id / 100)) % 4];
  return j;
}

static void sum_view(RnJobInScheduler* r) {   // allocated_res_view = the sum of allocated_res over its nodes (CtldPublicDefs.cpp:1901-1902)
  r->allocated_res_view = ResourceView{};
  for (const auto& [id, res] : r->allocated_res) {
    r->allocated_res_view.cpu_count.raw += res.cpu_set.cpu_count.raw;
    r->allocated_res_view.memory_bytes += res.memory_bytes;
  }
}

static std::unique_ptr<RnJobInScheduler> running(job_id_t id, std::vector<std::pair<std::string, std::vector<uint32_t>>> allocs, TimeSec start, TimeSec end, int i) {
  auto r = std::make_unique<RnJobInScheduler>();
  r->job_id = id; r->start_time = start; r->end_time = end;
  for (const auto& [craned, cores] : allocs) {
    ResourceInNodeV3& res = r->allocated_res[craned];
    res.cpu_set.cpu_count = cpu_t((int)cores.size());
    for (uint32_t c : cores) res.cpu_set.core_ids.insert(c);
    res.memory_bytes = cores.size() * G;
  }
  sum_view(r.get());
  r->qos = "normal"; r->qos_priority = (uint32_t)(10 * (i % 3)); r->partition_priority = 1 + (uint32_t)i % 5; r->account = ACCOUNTS[i % 3];
  return r;
}

static std::vector<std::unique_ptr<PdJobInScheduler>> queue_of(int c, TimeSec now) {
  std::vector<std::unique_ptr<PdJobInScheduler>> pd;
  for (int i = 0; i < 14; ++i) {
    const job_id_t id = 100 * (c + 1) + i;
    if (i == 7) pd.push_back(job(id, "p0", 2, 900, 3, i, now));            // three nodes
    else if (i == 10) pd.push_back(job(id, "p0", 8, 300, 1, i, now));      // a whole node
    else pd.push_back(job(id, i % 2 ? "p1" : "p0", 1 + i % 3, 200 + 250 * (i % 4), 1, i, now));
  }
  return pd;
}

static int cycles() {
  GpuNodeSelectionAlgo algo(0);
  ClusterSnapshot snap;
  for (int i = 0; i < 6; ++i) snap.craned_metas.push_back(node("n" + std::to_string(i), 8, 32));
  snap.partitions = {{"p0", {"n0", "n1", "n2", "n3", "n4", "n5"}}, {"p1", {"n1", "n3", "n5"}}};
  algo.SetClusterSnapshot(snap);
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }
  std::vector<std::unique_ptr<RnJobInScheduler>> run;
  run.push_back(running(1, {{"n0", {0, 1}}}, NOW - 5000, NOW + 300, 0));
  run.push_back(running(2, {{"n1", {0}}}, NOW - 100, NOW + 900, 1));
  run.push_back(running(3, {{"n1", {1, 2}}, {"n2", {0, 1, 2}}}, NOW - 70000, NOW + 1500, 2));   // two nodes: node_num 2, 5 cpus, 5 GiB
  run.push_back(running(4, {{"n4", {0}}}, NOW - 33, NOW + 700, 3));
  run.push_back(running(5, {{"n3", {5}}}, NOW - 900, NOW + 5000, 4));
  const std::vector<std::unique_ptr<RnJobInScheduler>> nothing;
  algo.UseResidentRunning(true);
  algo.UseResidentAttrs(true);
  CHECK(!algo.ResidentAttrs());
  if (!algo.SeedRunning(run)) { printf("SeedRunning: %s\n", algo.LastError().c_str()); return 1; }
  CHECK(algo.ResidentAttrs() && algo.NumAccounts() == 3);
  PriorityConfig pc;
  pc.WeightJobSize = 700;
  GpuMultiFactorPriority borrowed(pc, &algo), own(pc, 0);
  if (!borrowed.Ok() || !own.Ok()) { printf("sorter: %s%s\n", borrowed.LastError().c_str(), own.LastError().c_str()); return 1; }
  size_t admitted_total = 0, retired_total = 0, differ = 0, running_matters = 0;
  for (int c = 0; c < 4; ++c) {
    const TimeSec now = NOW + STEP * c;
    auto pd = queue_of(c, now), pd2 = queue_of(c, now), pd3 = queue_of(c, now);
    const size_t limit = c == 2 ? 9 : 1000;
    std::vector<PdJobInScheduler*> o1, o2, o3;
    borrowed.GetOrderedJobPtrVec(now, pd, nothing, limit, o1);     // EMPTY: the ledger is the running side
    if (!borrowed.Ok()) { printf("borrowed sorter (cycle %d): %s\n", c, borrowed.LastError().c_str()); return 1; }
    own.GetOrderedJobPtrVec(now, pd2, run, limit, o2);             // the same jobs from the host, in ledger order
    if (!own.Ok()) { printf("own sorter (cycle %d): %s\n", c, own.LastError().c_str()); return 1; }
    own.GetOrderedJobPtrVec(now, pd3, nothing, limit, o3);         // ... and without any: a condition on the inputs
    CHECK(o1.size() == o2.size() && o1.size() == std::min(limit, pd.size()));
    for (size_t i = 0; i < std::min(o1.size(), o2.size()); ++i)
      if (o1[i]->job_id != o2[i]->job_id) { if (!differ++) printf("cycle %d: position %zu is job %u, the own sorter has %u\n", c, i, o1[i]->job_id, o2[i]->job_id); }
    for (size_t i = 0; i < pd.size(); ++i) {
      if (memcmp(&pd[i]->priority, &pd2[i]->priority, 8) != 0) { if (!differ++) printf("cycle %d: job %u priority %.17g, the own sorter has %.17g\n", c, pd[i]->job_id, pd[i]->priority, pd2[i]->priority); }
      if (pd[i]->reason != pd2[i]->reason) ++differ;
      if (memcmp(&pd[i]->priority, &pd3[i]->priority, 8) != 0) ++running_matters;
    }
    for (auto& j : pd) { j->priority = 0; j->reason.clear(); }     // (a cycle of its own: the order handed to NodeSelect is the queue's)
    algo.NodeSelect(now, nothing, pd);
    if (!algo.Ok()) { printf("NodeSelect (cycle %d): %s\n", c, algo.LastError().c_str()); return 1; }
    std::vector<const PdJobInScheduler*> admitted;
    size_t started = 0;
    for (const auto& j : pd)
      if (j->reason.empty() && j->start_time == now && started++ % 2 == 0) admitted.push_back(j.get());
    std::vector<job_id_t> finished;
    for (const auto& r : run) if (r->end_time <= now + STEP) finished.push_back(r->job_id);
    finished.push_back(77);   // an unknown job: nothing changes
    run.erase(std::remove_if(run.begin(), run.end(), [&](const auto& r) { return r->end_time <= now + STEP; }), run.end());
    for (const PdJobInScheduler* j : admitted) {   // the caller's mirror, in ledger order: what the columns must hold
      auto r = std::make_unique<RnJobInScheduler>();
      r->job_id = j->job_id; r->start_time = now; r->end_time = j->end_time; r->allocated_res = j->allocated_res;
      r->qos = j->qos; r->qos_priority = j->qos_priority; r->partition_priority = j->partition_priority; r->account = j->account;
      sum_view(r.get());
      run.push_back(std::move(r));
    }
    admitted_total += admitted.size(); retired_total += finished.size() - 1;
    uint64_t nret = 0, nadm = 0;
    if (!algo.AdvanceRunning(finished, admitted, &nret, &nadm)) { printf("AdvanceRunning (cycle %d): %s\n", c, algo.LastError().c_str()); return 1; }
    CHECK(nret == finished.size() - 1 && nadm == admitted.size());
    CHECK(algo.ResidentAttrs());
    if (c == 1) {   // a new snapshot between two cycles: the ledger and its columns stay (the rebuild behind it carries them)
      algo.SetClusterSnapshot(snap);
      if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }
    }
  }
  CHECK(differ == 0);
  CHECK(algo.NumAccounts() == 4);
  CHECK(admitted_total >= 6 && retired_total >= 3 && running_matters > 0);
  printf("attrs adapter: 4 cycles, %zu jobs admitted, %zu retired, %zu orders or priorities differ, %d failures\n", admitted_total, retired_total, differ, g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  {
    GpuNodeSelectionAlgo algo(0);
    if (no_gpu) {
      if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
      GpuMultiFactorPriority borrowed(PriorityConfig{}, &algo);
      CHECK(!borrowed.Ok() && !algo.ResidentAttrs());
      printf("no device: the borrowed sorter refuses (%s)\n", borrowed.LastError().c_str());
      return g_fail ? 1 : 0;
    }
    if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  }
  return cycles();
}
