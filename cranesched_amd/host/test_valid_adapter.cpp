// Drives GpuNodeSelectionAlgo::CheckJobValidity (include/crane_gpu_valid/validity.h): hand-derived cases at string level — one per code,
// the CraneErrCode names, a down node, an unknown included name — and, with --bench, a measurement against a single-threaded loop that
// restates the reference's walk (JobScheduler.cpp:7353-7365, with its early break at node_num) on the same host.
//   test_valid_adapter            -> needs an MI355X, exit 0 on success
//   test_valid_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_valid_adapter --bench [jobs] [nodes]   -> 65 536 nodes in 8 partitions and 1 M jobs (the shape of config C4) drawn by the driver's own
//                                    generator, once plain and once with 5 % of the jobs carrying lists: kernel_ms, the whole call, the CPU loop;
//                                    one warm-up, median of 7.  Nothing is asserted there but the agreement of the OK / not-OK split.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_valid/validity.h"

using namespace crane;

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib, bool alive = true) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  m.alive = alive;
  return m;
}

static PdJobInScheduler job(const std::string& part, double cpu, uint64_t mem, uint32_t k = 1, uint32_t nt = 0) {
  PdJobInScheduler j;
  j.partition_id = part;
  j.time_limit = 3600;
  j.req_task_res_view.cpu_count = cpu_t(cpu);
  j.req_task_res_view.memory_bytes = mem;
  j.node_num = k;
  j.ntasks = nt ? nt : k;
  return j;
}

struct Want { uint8_t code; uint32_t eligible; const char* err; };

static int hand_cases(GpuNodeSelectionAlgo& algo) {
  // n0 8c 16G | n1 8c 16G DOWN | n2 16c 64G a100 x2 | n3 16c 64G a100 x1 + v100 x2 | n4 4c 8G | n6 8c 16G fpga x1
  // p0 = {n0 n1 n2 n3}   p1 = {n3 n4}   p3 = {n6}   p2 = {n4 n5}, n5 not expressible   reservation "r0" = {n2 n3}
  ClusterSnapshot snap;
  snap.craned_metas = {node("n0", 8, 16), node("n1", 8, 16, false), node("n2", 16, 64), node("n3", 16, 64), node("n4", 4, 8), node("n6", 8, 16)};
  snap.craned_metas[2].res_total.gres["gpu"]["a100"] = {"/dev/a0", "/dev/a1"};
  snap.craned_metas[3].res_total.gres["gpu"]["a100"] = {"/dev/a0"};
  snap.craned_metas[3].res_total.gres["gpu"]["v100"] = {"/dev/v0", "/dev/v1"};
  snap.craned_metas[5].res_total.gres["fpga"]["x"] = {"/dev/f0"};
  snap.craned_metas.push_back(node("n5", 4, 8));
  snap.craned_metas.back().res_total.cpu_set.core_ids.insert(300);   // a core id the engine's masks do not hold: the node is flagged unsupported
  snap.partitions = {{"p0", {"n0", "n1", "n2", "n3"}}, {"p1", {"n3", "n4"}}, {"p3", {"n6"}}, {"p2", {"n4", "n5"}}};
  ResvMeta rv;
  rv.name = "r0"; rv.start_time = 1000; rv.end_time = 2000;
  for (const char* n : {"n2", "n3"}) {
    ResourceInNodeV3& r = rv.res_total[n];
    r.cpu_set.cpu_count = cpu_t(1); r.cpu_set.core_ids = {0}; r.memory_bytes = G;
  }
  snap.reservations.push_back(rv);
  algo.SetClusterSnapshot(snap);
  CHECK(algo.Ok());
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }

  std::vector<PdJobInScheduler> q;
  std::vector<Want> want;
  auto add = [&](PdJobInScheduler j, uint8_t code, uint32_t elig, const char* err) { q.push_back(std::move(j)); want.push_back({code, elig, err}); };
  { auto j = job("p0", 1, G); j.node_num = 0; add(j, CNS_VALID_BAD_REQUEST, 0, "ERR_INVALID_PARAM"); }
  { auto j = job("p0", 1, G, 2, 1); j.ntasks = 1; add(j, CNS_VALID_BAD_REQUEST, 0, "ERR_INVALID_PARAM"); }
  add(job("p0", 1, 0), CNS_VALID_ZERO_MEM, 0, "ERR_INVALID_PARAM");
  add(job("nowhere", 0, G), CNS_VALID_ZERO_CPU, 0, "ERR_INVALID_PARAM");
  add(job("nowhere", 1, G), CNS_VALID_PARTITION_NOT_FOUND, 0, "ERR_INVALID_PARTITION");
  { auto j = job("nowhere", 1, G); j.reservation = "r0"; add(j, CNS_VALID_PARTITION_NOT_FOUND, 0, "ERR_INVALID_PARTITION"); }
  { auto j = job("p0", 8, G, 1, 4); j.ntasks_per_node_min = 4; j.ntasks_per_node_max = 4; add(j, CNS_VALID_OK, 4, ""); }   // one task per node is what is tested
  add(job("p0", 8, 16 * G, 4), CNS_VALID_OK, 4, "");                                   // the down node n1 counts
  add(job("p3", 8, 16 * G), CNS_VALID_OK, 1, "");                                      // exactly res_total
  { auto j = job("p0", 1, G); j.req_task_res_view.cpu_count = cpu_t::from_raw(16 * 256 + 1); add(j, CNS_VALID_NOT_ENOUGH_NODES, 0, "ERR_NO_ENOUGH_NODE"); }
  add(job("p1", 1, G, 1, 20), CNS_VALID_OK, 2, "");                                    // total cpu exactly the partition's
  { auto j = job("p1", 1, G, 1, 20); j.req_node_res_view.cpu_count = cpu_t::from_raw(1); add(j, CNS_VALID_NO_RESOURCE, 0, "ERR_NO_RESOURCE"); }
  { auto j = job("p3", 1, G); j.req_node_res_view.gres_map["gpu"].specified["a100"] = 1; add(j, CNS_VALID_NO_RESOURCE, 0, "ERR_NO_RESOURCE"); }
  { auto j = job("p0", 1, G, 2); j.req_node_res_view.gres_map["gpu"].specified["v100"] = 1; add(j, CNS_VALID_NOT_ENOUGH_NODES, 1, "ERR_NO_ENOUGH_NODE"); }
  { auto j = job("p0", 1, G); j.req_node_res_view.gres_map["gpu"].total = 3; add(j, CNS_VALID_OK, 1, ""); }                 // 1 a100 + 2 v100 on n3
  { auto j = job("p0", 1, G); j.req_node_res_view.gres_map["fpga"].total = 1; add(j, CNS_VALID_NO_RESOURCE, 0, "ERR_NO_RESOURCE"); }
  { auto j = job("p0", 1, G); j.req_node_res_view.gres_map["tpu"].total = 1; add(j, CNS_VALID_NO_RESOURCE, 0, "ERR_NO_RESOURCE"); }   // a name nobody has
  { auto j = job("p1", 1, G); j.included_nodes = {"n0", "n4"}; add(j, CNS_VALID_OK, 1, ""); }
  { auto j = job("p1", 1, G); j.included_nodes = {"ghost-a", "ghost-b", "n4"}; add(j, CNS_VALID_OK, 1, ""); }               // two unknown names: no "node twice"
  { auto j = job("p3", 1, G); j.excluded_nodes = {"n6"}; add(j, CNS_VALID_NOT_ENOUGH_NODES, 0, "ERR_NO_ENOUGH_NODE"); }
  add(job("p0", 16, G, 2), CNS_VALID_OK, 2, "");
  add(job("p0", 16, G, 3), CNS_VALID_NOT_ENOUGH_NODES, 2, "ERR_NO_ENOUGH_NODE");
  add(job("p3", 1, G, 2), CNS_VALID_NODE_NUM, 0, "ERR_INVALID_NODE_NUM");
  { auto j = job("p0", 1, G); j.reservation = "never"; add(j, CNS_VALID_RESV_NOT_FOUND, 0, "ERR_INVALID_PARAM"); }
  { auto j = job("p0", 1, G); j.reservation = "r0"; j.included_nodes = {"n0", "n2"}; add(j, CNS_VALID_RESV_NODE, 0, "ERR_INVALID_PARAM"); }
  { auto j = job("p0", 1, G); j.reservation = "r0"; j.included_nodes = {"n2"}; add(j, CNS_VALID_OK, 1, ""); }
  add(job("p0", 16, G), CNS_VALID_OK, 2, "");                                          // n3 is shared: two answers
  add(job("p1", 16, G), CNS_VALID_OK, 1, "");
  add(job("p2", 1, G), CNS_VALID_REFUSED, 0, "");                                      // ask the CPU code; p1 shares n4 with it and is answered
  CHECK(algo.UnsupportedNodes() == 1);

  std::vector<const PdJobInScheduler*> ptr;
  for (const auto& j : q) ptr.push_back(&j);
  std::vector<GpuNodeSelectionAlgo::ValidityAnswer> ans;
  double ms = -1;
  CHECK(algo.CheckJobValidity(ptr, &ans, &ms));
  if (!algo.Ok()) printf("CheckJobValidity: %s\n", algo.LastError().c_str());
  CHECK(ans.size() == q.size());
  for (size_t i = 0; i < ans.size(); ++i) {
    const bool ok = ans[i].code == want[i].code && ans[i].eligible == want[i].eligible && !strcmp(ans[i].crane_err, want[i].err) && ans[i].refused == (want[i].code == CNS_VALID_REFUSED);
    if (!ok) { printf("case %zu: got code %u eligible %u %s, want code %u eligible %u %s\n", i, ans[i].code, ans[i].eligible, ans[i].crane_err, want[i].code, want[i].eligible, want[i].err); ++g_fail; }
  }
  CHECK(ms >= 0);
  for (const auto& j : q) CHECK(j.reason.empty() && j.craned_ids.empty());             // nothing of a job is written
  std::vector<GpuNodeSelectionAlgo::ValidityAnswer> none;
  CHECK(algo.CheckJobValidity({}, &none) && none.empty());
  // a node going down changes nothing: res_total stays (SetCranedState flips the schedulable flag only)
  algo.SetCranedState("n0", false, false);
  std::vector<GpuNodeSelectionAlgo::ValidityAnswer> again;
  CHECK(algo.CheckJobValidity(ptr, &again) && again.size() == ans.size());
  for (size_t i = 0; i < again.size() && i < ans.size(); ++i) CHECK(again[i].code == ans[i].code && again[i].eligible == ans[i].eligible);
  printf("hand cases: %zu jobs, %d failures\n", q.size(), g_fail);
  return g_fail;
}

static int bench(GpuNodeSelectionAlgo& algo, size_t J, int N) {
  const int P = 8;
  ClusterSnapshot snap;
  std::vector<std::vector<CranedId>> parts(P);
  std::vector<int> cores(N);
  std::vector<uint64_t> mem(N);
  Rng r{0x5EEDull};
  for (int i = 0; i < N; ++i) {
    char name[16];
    snprintf(name, sizeof name, "cn%05d", i);
    cores[i] = 16 << (r() % 3);                      // 16 / 32 / 64 cores, 4 GiB per core
    mem[i] = (uint64_t)cores[i] * 4;
    snap.craned_metas.push_back(node(name, cores[i], mem[i], r() % 50 != 0));
    parts[i % P].push_back(name);
  }
  for (int p = 0; p < P; ++p) snap.partitions.push_back({"P" + std::to_string(p), parts[p]});
  algo.SetClusterSnapshot(snap);
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return 1; }
  for (int with_lists = 0; with_lists < 2; ++with_lists) {
    std::vector<PdJobInScheduler> q(J);
    Rng g{0xC4C4C4ull + (uint64_t)with_lists};
    for (size_t j = 0; j < J; ++j) {
      const uint64_t a = g(), b = g();
      q[j] = job("P" + std::to_string(a % P), (double)(1 << ((a >> 8) % 7)), (1ull + ((a >> 16) % 64)) * 4 * G, 1 + (uint32_t)((a >> 24) % 4 == 0 ? (a >> 28) % 8 : 0));
      if (with_lists && b % 20 == 0) {
        const int p = (int)(a % P);
        auto& lst = (b >> 8) % 2 ? q[j].included_nodes : q[j].excluded_nodes;
        for (int i = 0; i < 8; ++i) lst.insert(parts[p][(size_t)((b >> (12 + 6 * i)) % parts[p].size())]);
      }
    }
    std::vector<const PdJobInScheduler*> ptr;
    for (const auto& j : q) ptr.push_back(&j);
    std::vector<GpuNodeSelectionAlgo::ValidityAnswer> ans;
    std::vector<double> kms, call;
    for (int rep = 0; rep < 8; ++rep) {              // one warm-up (it also builds the derived tables), then 7
      double ms = 0;
      const auto t0 = std::chrono::steady_clock::now();
      if (!algo.CheckJobValidity(ptr, &ans, &ms)) { printf("CheckJobValidity: %s\n", algo.LastError().c_str()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      if (rep) { kms.push_back(ms); call.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    // the reference's walk, one thread: per job the nodes of its partition in order, stop at node_num (:7364)
    std::vector<std::vector<int>> pidx(P);
    for (int i = 0; i < N; ++i) pidx[i % P].push_back(i);
    std::unordered_map<std::string, int> name_idx;
    for (int i = 0; i < N; ++i) name_idx[snap.craned_metas[i].craned_id] = i;
    std::vector<double> cpu_ms;
    size_t cpu_ok = 0;
    for (int rep = 0; rep < 3; ++rep) {
      cpu_ok = 0;
      const auto t0 = std::chrono::steady_clock::now();
      for (size_t j = 0; j < J; ++j) {
        const PdJobInScheduler& p = q[j];
        const int part = atoi(p.partition_id.c_str() + 1);
        const int64_t need_cpu = p.req_node_res_view.cpu_count.raw + p.req_task_res_view.cpu_count.raw;
        const uint64_t need_mem = p.req_node_res_view.memory_bytes + p.req_task_res_view.memory_bytes;
        uint32_t avail = 0;
        for (int n : pidx[part]) {                                                               // :7354
          const CranedMeta& m = snap.craned_metas[n];
          if (need_cpu <= m.res_total.cpu_set.cpu_count.raw && need_mem <= m.res_total.memory_bytes &&   // :7356-7357
              (p.included_nodes.empty() || p.included_nodes.count(m.craned_id)) &&               // :7358-7359
              (p.excluded_nodes.empty() || !p.excluded_nodes.count(m.craned_id)))                // :7360-7361
            ++avail;                                                                             // :7362
          if (avail >= p.node_num) break;                                                        // :7364
        }
        cpu_ok += avail >= p.node_num;
      }
      cpu_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    size_t gpu_ok = 0, gpu_walked = 0;
    for (const auto& a : ans) { gpu_ok += a.code == CNS_VALID_OK; gpu_walked += a.code == CNS_VALID_OK || a.code == CNS_VALID_NOT_ENOUGH_NODES; }
    printf("validity bench %s: %zu jobs x %d nodes in %d partitions: kernel_ms %.3f  call_ms %.3f  cpu_walk_ms %.3f (one thread, early break; median of %zu / %zu / %zu)"
           "  OK %zu of %zu walked (cpu walk: %zu of all)\n",
           with_lists ? "with lists on 5 % of the jobs" : "plain", J, N, P, median(kms), median(call), median(cpu_ms), kms.size(), call.size(), cpu_ms.size(),
           gpu_ok, gpu_walked, cpu_ok);
  }
  return 0;
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  GpuNodeSelectionAlgo algo(0);
  if (no_gpu) {
    if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
    std::vector<GpuNodeSelectionAlgo::ValidityAnswer> ans;
    PdJobInScheduler j = job("p0", 1, G);
    CHECK(!algo.CheckJobValidity({&j}, &ans) && ans.empty() && !algo.Ok() && algo.LastStatus() != 0);
    printf("no device: CheckJobValidity refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
    return g_fail ? 1 : 0;
  }
  if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  if (argc > 1 && !strcmp(argv[1], "--bench"))
    return bench(algo, argc > 2 ? (size_t)atoll(argv[2]) : (size_t)1 << 20, argc > 3 ? atoi(argv[3]) : 65536);
  return hand_cases(algo) ? 1 : 0;
}
