// Drives GpuNodeSelectionAlgo::ProbeStart: a small string-level scenario built in code (nodes of two sizes, three partitions of which two
// share nodes, running jobs, a queue with multi-node / exclusive / node-list jobs), one NodeSelect, then ProbeStart on M fresh job
// objects.  Yardstick: the CYCLE path of a second GpuNodeSelectionAlgo — what it writes for the same job appended to the same queue
// (that path is held to the oracle job by job by tests/test_adapter_vs_oracle.py).
//   test_probe_adapter [J]        -> needs an MI355X, exit 0 on success (J: jobs of the queue, default 160)
//   test_probe_adapter --no-gpu   -> the loud "no device" behaviour of ProbeStart instead
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu/node_select.h"

using namespace crane;

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  return m;
}

static const char* const kParts[3] = {"P0", "P1", "ALL"};
// job `id` of the stream `r`: the same call sequence gives the same job (the queue is built twice: once per algorithm object)
static std::unique_ptr<PdJobInScheduler> make_job(job_id_t id, Rng& r, const std::vector<CranedId>& ids) {
  auto j = std::make_unique<PdJobInScheduler>();
  const uint64_t a = r(), b = r(), c = r();
  j->job_id = id;
  j->time_limit = 300 * (1 + (int64_t)(a % 23));
  j->partition_id = (a >> 8) % 41 == 0 ? std::string("nowhere") : std::string(kParts[(a >> 16) % 3]);
  j->req_task_res_view.cpu_count = cpu_t((double)(1 << ((a >> 24) & 3)) + (((a >> 28) & 7) == 0 ? 0.5 : 0.0));
  j->req_task_res_view.memory_bytes = (1ull + ((a >> 32) & 3)) << 30;
  if ((b & 7) == 0) { j->node_num = 2 + (uint32_t)((b >> 4) % 3); j->ntasks = j->node_num; }
  if ((b >> 8) % 11 == 0) { j->ntasks = j->node_num + (uint32_t)((b >> 12) % 4); j->ntasks_per_node_max = 1 + j->ntasks - j->node_num; }
  if ((b >> 20) % 19 == 0) j->exclusive = true;
  if ((c & 31) == 0) for (int i = 0; i < 5; ++i) j->included_nodes.insert(ids[(c >> (8 + 6 * i)) % ids.size()]);
  if ((c & 31) == 1) { j->included_nodes.insert("no-such-craned"); j->included_nodes.insert(ids[(c >> 8) % ids.size()]); }
  if ((c & 31) == 2) for (int i = 0; i < 9; ++i) j->excluded_nodes.insert(ids[(c >> (8 + 5 * i)) % ids.size()]);
  if ((c >> 40) % 53 == 0) j->reason = "License";   // the caller pre-set a reason: not asked, reason kept
  return j;
}

static bool same_answer(const PdJobInScheduler& a, const PdJobInScheduler& b) {
  bool ok = a.reason == b.reason && a.craned_ids == b.craned_ids && a.craned_id_to_task_num == b.craned_id_to_task_num &&
            a.allocated_res.size() == b.allocated_res.size();
  if (!a.craned_ids.empty() || a.reason == "Priority" || a.reason == "Resource Reserved") ok = ok && a.start_time == b.start_time && a.end_time == b.end_time;
  if (ok)
    for (const auto& [cid, rb] : b.allocated_res) {
      auto it = a.allocated_res.find(cid);
      ok = ok && it != a.allocated_res.end() && it->second.cpu_set.cpu_count == rb.cpu_set.cpu_count && it->second.cpu_set.core_ids == rb.cpu_set.core_ids &&
           it->second.memory_bytes == rb.memory_bytes && it->second.memory_sw_bytes == rb.memory_sw_bytes && it->second.gres == rb.gres;
    }
  return ok;
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  const int N = 48, M = 32;
  // 160 jobs load the 1 536 cores about half: some probes start now, the wide, exclusive and long ones wait (the checks below ask for both)
  const int J = (argc > 1 && !no_gpu && atoi(argv[1]) > 0) ? atoi(argv[1]) : 160;
  ClusterSnapshot snap;
  std::vector<CranedId> ids;
  std::vector<std::vector<CranedId>> parts(3);
  for (int i = 0; i < N; ++i) {
    char name[16];
    snprintf(name, sizeof name, "cn%03d", i);
    snap.craned_metas.push_back(node(name, i % 3 == 0 ? 64 : 16, i % 3 == 0 ? 256 : 64));
    ids.push_back(name);
    parts[i < N / 2 ? 0 : 1].push_back(name);
    if (i % 4 != 3) parts[2].push_back(name);   // ALL shares three quarters of the nodes with P0 / P1
  }
  snap.partitions = {{"P0", parts[0]}, {"P1", parts[1]}, {"ALL", parts[2]}};
  std::vector<std::unique_ptr<RnJobInScheduler>> running;
  {
    Rng r{0x1234567ull};
    for (int i = 0; i < 30; ++i) {
      auto rj = std::make_unique<RnJobInScheduler>();
      rj->job_id = 100000 + i; rj->partition_id = "P0"; rj->start_time = 500; rj->end_time = 1200 + (int64_t)(r() % 9000);
      ResourceInNodeV3& res = rj->allocated_res[ids[(size_t)i]];   // one running job per node: core ids stay disjoint
      res.cpu_set.cpu_count = cpu_t(4);
      for (uint32_t c = 0; c < 4; ++c) res.cpu_set.core_ids.insert(c);
      res.memory_bytes = 8ull << 30;
      running.push_back(std::move(rj));
    }
  }
  auto build_queue = [&]() {
    std::vector<std::unique_ptr<PdJobInScheduler>> q;
    Rng r{0x9E3779B97F4A7C15ull};
    for (int j = 0; j < J; ++j) q.push_back(make_job((job_id_t)(j + 1), r, ids));
    return q;
  };
  auto build_probes = [&]() {
    std::vector<std::unique_ptr<PdJobInScheduler>> q;
    Rng r{0xC0FFEE1234ull};
    for (int m = 0; m < M; ++m) {
      q.push_back(make_job((job_id_t)(50000 + m), r, ids));
      PdJobInScheduler& p = *q.back();
      if (m % 4 == 0 || p.reason == "License") continue;          // every fourth probe: whatever the generator drew
      // ... the others ask questions whose KIND of answer the scenario fixes (the checks at the end want both kinds):
      p.node_num = p.ntasks = p.ntasks_per_node_min = p.ntasks_per_node_max = 1;
      p.included_nodes.clear(); p.excluded_nodes.clear();
      if (m % 2 == 1) {   // one whole node of P0, where every node runs a job beyond `now`: a later start
        p.partition_id = "P0"; p.exclusive = true;
      } else {            // one cpu for a short while, anywhere: starts now on a half-loaded cluster
        p.partition_id = "ALL"; p.exclusive = false; p.time_limit = 300;
        p.req_task_res_view.cpu_count = cpu_t(1.0); p.req_task_res_view.memory_bytes = 1ull << 30;
      }
    }
    return q;
  };
  auto ptrs = [](const std::vector<std::unique_ptr<PdJobInScheduler>>& v) {
    std::vector<PdJobInScheduler*> p;
    for (const auto& j : v) p.push_back(j.get());
    return p;
  };

  GpuNodeSelectionAlgo algo(0);
  if (no_gpu) {
    // no device: every probe without a reason is marked, the status says why, nothing is thrown
    CHECK(!algo.Ok());
    algo.SetClusterSnapshot(snap);
    auto probes = build_probes();
    algo.ProbeStart(ptrs(probes));
    CHECK(!algo.Ok() && algo.LastStatus() == CNS_ERR_NO_DEVICE && !algo.LastError().empty());
    for (const auto& p : probes) CHECK(p->reason == "GpuEngineError" || p->reason == "License");
    for (const auto& p : probes) CHECK(p->craned_ids.empty() && p->allocated_res.empty());
    algo.ProbeStart({});
    printf("%s\n", g_fail ? "FAIL" : "ok (no device: ProbeStart is loud)");
    return g_fail != 0;
  }
  if (!algo.Ok()) { printf("engine: %s\n", algo.LastError().c_str()); return 2; }
  algo.SetClusterSnapshot(snap);
  CHECK(algo.Ok());
  {  // before any cycle: CNS_ERR_STATE, the probes are marked
    auto probes = build_probes();
    algo.ProbeStart(ptrs(probes));
    CHECK(!algo.Ok() && algo.LastStatus() == CNS_ERR_STATE);
    for (const auto& p : probes) CHECK(p->reason == "GpuEngineError" || p->reason == "License");
  }
  auto queue = build_queue();
  algo.NodeSelect(1000, running, queue);     // (the default, lazy write-back: ProbeStart writes in full all the same)
  CHECK(algo.Ok());
  auto probes = build_probes();
  algo.ProbeStart(ptrs(probes));
  CHECK(algo.Ok());
  if (!algo.Ok()) printf("ProbeStart: %s\n", algo.LastError().c_str());

  GpuNodeSelectionAlgo other(0);
  other.SetClusterSnapshot(snap);
  other.SetFullWriteBack(true);
  size_t same = 0, now = 0, later = 0, none = 0, kept = 0;
  for (int m = 0; m < M; ++m) {
    auto q = build_queue();
    auto fresh = build_probes();
    q.push_back(std::move(fresh[(size_t)m]));
    other.NodeSelect(1000, running, q);
    CHECK(other.Ok());
    const PdJobInScheduler& want = *q.back();
    const PdJobInScheduler& got = *probes[(size_t)m];
    const bool ok = same_answer(got, want);
    if (!ok) printf("  probe %d differs: reason '%s' / '%s', start %lld / %lld, %zu / %zu nodes\n", m, got.reason.c_str(), want.reason.c_str(),
                    (long long)got.start_time, (long long)want.start_time, got.craned_ids.size(), want.craned_ids.size());
    same += ok;
    if (want.reason == "License") ++kept;
    else if (want.reason.empty()) ++now;
    else if (!want.craned_ids.empty()) ++later;
    else ++none;
  }
  CHECK(same == (size_t)M);
  CHECK(now >= 4 && later >= 4);          // the scenario asks both kinds of question
  // the cycle's own results are untouched: a second ProbeStart answers the same, and the queue still materialises
  auto again = build_probes();
  algo.ProbeStart(ptrs(again));
  CHECK(algo.Ok());
  for (int m = 0; m < M; ++m) CHECK(same_answer(*again[(size_t)m], *probes[(size_t)m]) && again[(size_t)m]->start_time == probes[(size_t)m]->start_time);
  CHECK(algo.LastOrder().size() == (size_t)J);
  printf("  %zu of %d probes identical to the cycle path (%zu start now, %zu later, %zu without a start, %zu kept their reason)\n", same, M, now, later, none, kept);
  printf("%s\n", g_fail ? "FAIL" : "ok");
  return g_fail != 0;
}
