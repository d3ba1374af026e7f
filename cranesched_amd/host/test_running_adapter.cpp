// Drives GpuNodeSelectionAlgo::UseResidentRunning / SeedRunning / AdvanceRunning (include/crane_gpu_running/running.h): three consecutive
// cycles through NodeSelect, each built from the previous one's results, once with the running set handed in every cycle and once with it
// kept on the device — every job's reason, start, nodes and allocated cores must be identical — and, with --bench, a measurement of
// cns_running_advance against cns_set_running with the full arrays on the same handle.
//   test_running_adapter            -> needs an MI355X, exit 0 on success
//   test_running_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_running_adapter --bench [jobs] [nodes]   -> 65 536 nodes in 8 partitions, 1 M running jobs (90 % one-node, the rest 2..8), per step 1 %
//                                    retired and 1 % admitted from a real cycle: cns_running_advance (the whole call, and by stage),
//                                    cns_set_running with the arrays of the same ledger (the path this one replaces), cns_running_seed; one
//                                    warm-up, median of 5.  Asserted there: a cycle behind either gives the same digest.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_running/running.h"

using namespace crane;

static const TimeSec NOW = 1000000;
static const TimeSec STEP = 600;

static CranedMeta node(const std::string& id, int cores, uint64_t mem_gib) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = mem_gib << 30;
  m.alive = true;
  return m;
}

static std::unique_ptr<PdJobInScheduler> job(job_id_t id, const std::string& part, double cpu, int64_t limit, uint32_t k = 1, const std::string& resv = "") {
  auto j = std::make_unique<PdJobInScheduler>();
  j->job_id = id;
  j->partition_id = part;
  j->reservation = resv;
  j->time_limit = limit;
  j->req_task_res_view.cpu_count = cpu_t(cpu);
  j->req_task_res_view.memory_bytes = G;
  j->node_num = k;
  j->ntasks = k;
  return j;
}

static std::unique_ptr<RnJobInScheduler> running(job_id_t id, const std::string& craned, std::vector<uint32_t> cores, TimeSec end, const std::string& resv = "") {
  auto r = std::make_unique<RnJobInScheduler>();
  r->job_id = id; r->end_time = end; r->reservation = resv;
  ResourceInNodeV3& res = r->allocated_res[craned];
  res.cpu_set.cpu_count = cpu_t((double)cores.size());
  for (uint32_t c : cores) res.cpu_set.core_ids.insert(c);
  res.memory_bytes = cores.size() * G;
  return r;
}

// three cycles; *trace: one line per job and cycle
static bool three_cycles(bool resident, std::vector<std::string>* trace, size_t* admitted_total, size_t* retired_total) {
  GpuNodeSelectionAlgo algo(0);
  // p0 = {n0..n5}, p1 = {n1 n3 n5} (shared nodes: an allocation counts on two slots), 8 cores / 32 GiB each; reservation "r0" takes four
  // cores of n4 and n5 until NOW + 50000
  ClusterSnapshot snap;
  for (int i = 0; i < 6; ++i) snap.craned_metas.push_back(node("n" + std::to_string(i), 8, 32));
  snap.partitions = {{"p0", {"n0", "n1", "n2", "n3", "n4", "n5"}}, {"p1", {"n1", "n3", "n5"}}};
  ResvMeta rv;
  rv.name = "r0"; rv.start_time = NOW - 10; rv.end_time = NOW + 50000;
  for (const char* n : {"n4", "n5"}) {
    ResourceInNodeV3& r = rv.res_total[n];
    r.cpu_set.cpu_count = cpu_t(4.0);
    for (uint32_t c = 0; c < 4; ++c) r.cpu_set.core_ids.insert(c);
    r.memory_bytes = 8 * G;
  }
  snap.reservations.push_back(rv);
  algo.SetClusterSnapshot(snap);
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return false; }
  std::vector<std::unique_ptr<RnJobInScheduler>> run;
  run.push_back(running(1, "n0", {0, 1}, NOW + 300));
  run.push_back(running(2, "n1", {0}, NOW + 900));
  run.push_back(running(3, "n1", {1, 2}, NOW + 1500));
  run.push_back(running(4, "n4", {0}, NOW + 700, "r0"));
  run.push_back(running(5, "n3", {5}, NOW + 5000));
  const std::vector<std::unique_ptr<RnJobInScheduler>> nothing;
  if (resident) {
    algo.UseResidentRunning(true);
    if (!algo.SeedRunning(run)) { printf("SeedRunning: %s\n", algo.LastError().c_str()); return false; }
  }
  for (int c = 0; c < 3; ++c) {
    const TimeSec now = NOW + STEP * c;
    std::vector<std::unique_ptr<PdJobInScheduler>> pd;
    for (int i = 0; i < 12; ++i) {
      const job_id_t id = 100 * (c + 1) + i;
      if (i == 3) pd.push_back(job(id, "p0", 1, 400, 1, "r0"));            // inside the reservation
      else if (i == 7) pd.push_back(job(id, "p0", 2, 900, 3));             // three nodes
      else if (i == 10) pd.push_back(job(id, "p0", 8, 300));               // a whole node: backfilled or failed once the nodes fill up
      else pd.push_back(job(id, i % 2 ? "p1" : "p0", 1 + i % 3, 200 + 250 * (i % 4)));
    }
    if (c == 1) {   // a craned goes down and comes back between two cycles: a new snapshot, the ledger stays
      snap.craned_metas[2].alive = false;
      algo.SetClusterSnapshot(snap);
      snap.craned_metas[2].alive = true;
      algo.SetClusterSnapshot(snap);
      if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return false; }
    }
    algo.NodeSelect(now, resident ? nothing : run, pd);
    if (!algo.Ok()) { printf("NodeSelect (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
    std::vector<const PdJobInScheduler*> admitted;
    size_t started = 0;
    for (const auto& j : pd) {
      std::string line = "c" + std::to_string(c) + " job " + std::to_string(j->job_id) + " '" + j->reason + "' " + std::to_string(j->start_time);
      for (const CranedId& id : j->craned_ids) {
        line += " " + id + ":";
        for (uint32_t core : j->allocated_res.at(id).cpu_set.core_ids) line += std::to_string(core) + ",";
      }
      trace->push_back(line);
      if (j->reason.empty() && j->start_time == now && started++ % 2 == 0) admitted.push_back(j.get());   // every second started job
    }
    // the boundary: what ended by the next cycle leaves, what the commit loop started enters — on the caller's vector in ledger order
    std::vector<job_id_t> finished;
    for (const auto& r : run) if (r->end_time <= now + STEP) finished.push_back(r->job_id);
    finished.push_back(77);   // an unknown job: nothing changes (CranedMetaContainer.cpp:248-253)
    run.erase(std::remove_if(run.begin(), run.end(), [&](const auto& r) { return r->end_time <= now + STEP; }), run.end());
    for (const PdJobInScheduler* j : admitted) {
      auto r = std::make_unique<RnJobInScheduler>();
      r->job_id = j->job_id; r->end_time = j->end_time; r->reservation = j->reservation; r->allocated_res = j->allocated_res;
      run.push_back(std::move(r));
    }
    *admitted_total += admitted.size(); *retired_total += finished.size() - 1;
    if (resident) {
      uint64_t nret = 0, nadm = 0;
      if (!algo.AdvanceRunning(finished, admitted, &nret, &nadm)) { printf("AdvanceRunning (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
      CHECK(nret == finished.size() - 1 && nadm == admitted.size());
    }
  }
  return true;
}

static int hand_cases() {
  std::vector<std::string> with, without;
  size_t adm[2] = {0, 0}, ret[2] = {0, 0};
  if (!three_cycles(false, &without, &adm[0], &ret[0]) || !three_cycles(true, &with, &adm[1], &ret[1])) return 1;
  CHECK(with.size() == without.size() && with.size() == 36);
  size_t differ = 0;
  for (size_t i = 0; i < std::min(with.size(), without.size()); ++i)
    if (with[i] != without[i]) { if (!differ++) printf("first difference:\n  handed in: %s\n  resident:  %s\n", without[i].c_str(), with[i].c_str()); }
  CHECK(differ == 0);
  CHECK(adm[0] == adm[1] && ret[0] == ret[1] && adm[0] >= 6 && ret[0] >= 3);
  printf("hand cases: 3 cycles, %zu jobs admitted, %zu retired, %zu lines differ, %d failures\n", adm[1], ret[1], differ, g_fail);
  return g_fail ? 1 : 0;
}

// ---- --bench ------------------------------------------------------------------------------------------------------------------
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

static int bench(size_t R, uint32_t N) {
  cns_config cfg{};
  cfg.abi_version = CNS_ABI_VERSION;
  cns_handle* h = nullptr;
  if (cns_create(&cfg, &h) != 0) { printf("no usable device: %s\n", cns_last_error(nullptr)); return 2; }
  auto die = [&](const char* what) { printf("%s: %s\n", what, cns_last_error(h)); cns_destroy(h); return 1; };
  const uint32_t P = 8, per = N / P;
  std::vector<int64_t> ncpu(N, 64 * 256);
  std::vector<uint64_t> nmem(N, 1024 * G), nlo(N, ~0ull);
  std::vector<uint32_t> poff(P + 1), pnodes(N);
  for (uint32_t p = 0; p <= P; ++p) poff[p] = p * per;
  for (uint32_t n = 0; n < N; ++n) pnodes[n] = n;
  cns_node_soa nd{};
  nd.num_nodes = N; nd.num_partitions = P; nd.cpu_total_raw = ncpu.data(); nd.mem_total = nmem.data(); nd.core_lo = nlo.data();
  nd.part_offsets = poff.data(); nd.part_nodes = pnodes.data();
  if (cns_set_nodes(h, &nd) != 0) return die("cns_set_nodes");
  // the running set: job i on 1 node (90 %) or 2..8 consecutive nodes, a sixteenth of a core and 1 MiB each
  Rng g{0xABCDEF12345ull};
  std::vector<int64_t> end(R), acpu;
  std::vector<uint32_t> off(R + 1, 0), anode, ids(R);
  for (size_t i = 0; i < R; ++i) {
    const uint64_t a = g();
    const uint32_t w = a % 10 ? 1 : 2 + (uint32_t)((a >> 8) % 7), first = (uint32_t)((a >> 16) % N);
    for (uint32_t t = 0; t < w; ++t) anode.push_back((first + t) % N);
    off[i + 1] = (uint32_t)anode.size();
    end[i] = NOW + 100 + (int64_t)((a >> 40) % 100000);
    ids[i] = (uint32_t)i + 1;
  }
  const size_t A = anode.size();
  acpu.assign(A, 16);
  std::vector<uint64_t> amem(A, 1 << 20), alo(A, 0);
  cns_running_soa rn{};
  rn.num_jobs = (uint32_t)R; rn.num_allocs = (uint32_t)A; rn.end_sec = end.data(); rn.alloc_offsets = off.data(); rn.alloc_node = anode.data();
  rn.alloc_cpu_raw = acpu.data(); rn.alloc_mem = amem.data(); rn.alloc_core_lo = alo.data();
  // the queue of a step: 1 % of R one-node jobs of one core
  const size_t J = std::max<size_t>(R / 100, 1);
  std::vector<uint32_t> jpart(J), one(J, 1), jid(J);
  std::vector<int64_t> jl(J, 3600), jcpu(J, 256);
  std::vector<uint64_t> jmem(J, G), zero64(J, 0);
  for (size_t j = 0; j < J; ++j) jpart[j] = (uint32_t)(j % P);
  cns_job_soa js{};
  js.num_jobs = J; js.partition = jpart.data(); js.time_limit_sec = jl.data(); js.node_mem = zero64.data(); js.task_cpu_raw = jcpu.data(); js.task_mem = jmem.data();
  js.node_num = one.data(); js.ntasks = one.data(); js.ntasks_per_node_min = one.data(); js.ntasks_per_node_max = one.data();
  std::vector<int64_t> ostart(J + 1), ocpu(J + 1);
  std::vector<uint8_t> oreason(J + 1);
  std::vector<uint64_t> ooff(J + 1), omem(J + 1), olo(J + 1), ohi(J + 1), og(J + 1), ow2(J + 1), ow3(J + 1);
  std::vector<uint32_t> onode(J + 1), ont(J + 1);
  cns_placement_soa out{};
  out.place_capacity = J; out.start_sec = ostart.data(); out.reason = oreason.data(); out.place_offsets = ooff.data(); out.node_idx = onode.data(); out.ntasks = ont.data();
  out.cpu_raw = ocpu.data(); out.mem = omem.data(); out.core_lo = olo.data(); out.core_hi = ohi.data(); out.gres = og.data(); out.core_w2 = ow2.data(); out.core_w3 = ow3.data();
  std::vector<double> costs(N);
  auto cycle_digest = [&](int64_t now, uint64_t* digest) {
    if (cns_select(h, now, &js, &out) != 0) return false;
    if (cns_debug_get_costs(h, costs.data()) != 0) return false;
    uint64_t d = fnv(1469598103934665603ull, ostart.data(), J * 8);
    d = fnv(d, oreason.data(), J); d = fnv(d, onode.data(), J * 4); d = fnv(d, olo.data(), J * 8); d = fnv(d, costs.data(), (size_t)N * 8);
    *digest = d;
    return true;
  };
  auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  std::vector<double> seed_ms, adv_ms, adv_h2d, adv_ker, adv_d2h, set_ms;
  cns_running_timing tm{};
  for (int rep = 0; rep < 6; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    if (cns_running_seed(h, &rn, ids.data()) != 0) return die("cns_running_seed");
    if (rep) seed_ms.push_back(ms_since(t0));
  }
  int rc = 0;
  uint32_t next_id = (uint32_t)R + 1;
  size_t cursor = 0;
  std::vector<uint8_t> found(R / 100 + 1);
  for (int step = 0; step < 6; ++step) {   // one warm-up, then 5 steps, each from what the previous one left
    const int64_t now = NOW + step;
    uint64_t d0 = 0, d1 = 0, d2 = 0;
    if (!cycle_digest(now, &d0)) return die("cns_select");
    // 1 % retired: the next R / 100 seeded ids; 1 % admitted: the cycle's jobs
    std::vector<uint32_t> retire;
    for (size_t k = 0; k < R / 100 && cursor < R; ++k) retire.push_back(ids[cursor++]);
    for (size_t j = 0; j < J; ++j) jid[j] = next_id++;
    cns_running_step in{};
    in.num_retire = retire.size(); in.retire_ids = retire.data(); in.num_jobs = J; in.now_sec = now; in.job_id = jid.data();
    uint64_t nret = 0, nadm = 0;
    const cns_running_step_out so{found.data(), &nret, &nadm};
    const auto t0 = std::chrono::steady_clock::now();
    if (cns_running_advance(h, &in, &so) != 0) return die("cns_running_advance");
    const double call = ms_since(t0);
    cns_running_get_timing(h, &tm);
    if (step) { adv_ms.push_back(call); adv_h2d.push_back(tm.h2d_ms); adv_ker.push_back(tm.kernels_ms); adv_d2h.push_back(tm.d2h_ms); }
    if (nret != retire.size()) rc = 1;
    if (!cycle_digest(now + 1, &d1)) return die("cns_select");
    // the same ledger as arrays, through the path this call replaces (it drops the ledger: seeded again behind it)
    uint64_t lr = 0, la = 0;
    cns_running_ledger lo{};
    lo.num_jobs = &lr; lo.num_allocs = &la;
    if (cns_running_get(h, &lo) != 0) return die("cns_running_get");
    std::vector<uint32_t> gid(lr + 1), gresv(lr + 1), goff(lr + 1), gnode(la + 1);
    std::vector<int64_t> gend(lr + 1), gcpu(la + 1);
    std::vector<uint64_t> gmem(la + 1), glo(la + 1), ghi(la + 1), gw2(la + 1), gw3(la + 1), gg(la + 1);
    lo.capacity_jobs = lr; lo.capacity_allocs = la; lo.job_id = gid.data(); lo.end_sec = gend.data(); lo.reservation = gresv.data(); lo.alloc_offsets = goff.data();
    lo.alloc_node = gnode.data(); lo.alloc_cpu_raw = gcpu.data(); lo.alloc_mem = gmem.data(); lo.alloc_core_lo = glo.data(); lo.alloc_core_hi = ghi.data();
    lo.alloc_core_w2 = gw2.data(); lo.alloc_core_w3 = gw3.data(); lo.alloc_gres = gg.data();
    if (cns_running_get(h, &lo) != 0) return die("cns_running_get");
    cns_running_soa full{};
    full.num_jobs = (uint32_t)lr; full.num_allocs = (uint32_t)la; full.end_sec = gend.data(); full.alloc_offsets = goff.data(); full.alloc_node = gnode.data();
    full.alloc_cpu_raw = gcpu.data(); full.alloc_mem = gmem.data(); full.alloc_core_lo = glo.data(); full.alloc_core_hi = ghi.data(); full.alloc_gres = gg.data();
    full.reservation = gresv.data(); full.alloc_core_w2 = gw2.data(); full.alloc_core_w3 = gw3.data();
    const auto t1 = std::chrono::steady_clock::now();
    if (cns_set_running(h, &full) != 0) return die("cns_set_running");
    if (step) set_ms.push_back(ms_since(t1));
    if (!cycle_digest(now + 1, &d2)) return die("cns_select");
    if (d1 != d2 || d0 == d1 || nadm == 0) { printf("step %d: digests %016llx (before) %016llx (advance) %016llx (cns_set_running), %llu admitted\n", step, (unsigned long long)d0, (unsigned long long)d1, (unsigned long long)d2, (unsigned long long)nadm); rc = 1; }
    if (cns_running_seed(h, &full, gid.data()) != 0) return die("cns_running_seed");
  }
  printf("running bench: %u nodes in %u partitions, %zu running jobs seeded (%zu allocations), per step %zu retired and %zu in the queue: "
         "cns_running_advance call_ms %.3f (h2d_ms %.3f  kernels_ms %.3f  d2h_ms %.3f)  cns_set_running call_ms %.3f  cns_running_seed call_ms %.3f  "
         "(medians of 5; the ledger after the last step: %llu jobs, %llu allocations, %llu pairs)  cycle digests %s\n",
         N, P, R, A, R / 100, J, median(adv_ms), median(adv_h2d), median(adv_ker), median(adv_d2h), median(set_ms), median(seed_ms),
         (unsigned long long)tm.jobs, (unsigned long long)tm.allocs, (unsigned long long)tm.pairs, rc ? "DIFFER" : "equal");
  cns_destroy(h);
  return rc;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--bench")) return bench(argc > 2 ? (size_t)atoll(argv[2]) : (size_t)1000000, argc > 3 ? (uint32_t)atoi(argv[3]) : 65536u);
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  {
    GpuNodeSelectionAlgo algo(0);
    if (no_gpu) {
      if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
      const std::vector<std::unique_ptr<RnJobInScheduler>> none;
      CHECK(!algo.SeedRunning(none) && !algo.Ok() && algo.LastStatus() != 0);
      CHECK(!algo.AdvanceRunning({1}, {}) && !algo.Ok());
      printf("no device: SeedRunning refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
      return g_fail ? 1 : 0;
    }
    if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  }
  return hand_cases();
}
