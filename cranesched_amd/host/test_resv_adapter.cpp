// Drives GpuNodeSelectionAlgo::QueryReservation (include/crane_gpu_resv/resv_probe.h): hand-made string-level clusters, expected
// values written out below — worked out by hand from JobScheduler::CreateResv_'s node walk (JobScheduler.cpp:4383-4419).
//   test_resv_adapter            -> needs an MI355X, exit 0 on success
//   test_resv_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_resv_adapter --bench    -> kernel_ms of cns_resvq_run against a single-threaded C++ loop that restates :4383-4419 (the
//                                   reference's way, and for the earliest start the same loop retried over the event times):
//                                   1 x 65 536 and 1 024 x 4 096 candidates, each mode, 1 warm-up + 3 runs
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_resv/resv_probe.h"

using namespace crane;
using Algo = GpuNodeSelectionAlgo;
using Names = std::vector<CranedId>;

static CranedMeta node(const std::string& id, int cores = 8) {
  CranedMeta m;
  m.craned_id = id;
  m.res_total.cpu_set.cpu_count = cpu_t(cores);
  for (int c = 0; c < cores; ++c) m.res_total.cpu_set.core_ids.insert((uint32_t)c);
  m.res_total.memory_bytes = m.res_total.memory_sw_bytes = 32ull << 30;
  return m;
}
static ResourceInNodeV3 share(uint32_t first_core, uint32_t cores) {
  ResourceInNodeV3 r;
  r.cpu_set.cpu_count = cpu_t((int)cores);
  for (uint32_t c = 0; c < cores; ++c) r.cpu_set.core_ids.insert(first_core + c);
  r.memory_bytes = 1ull << 30;
  return r;
}
static ResvMeta resv(const std::string& name, TimeSec st, TimeSec ed, const Names& nodes, uint32_t first_core = 4, uint32_t cores = 2) {
  ResvMeta r;
  r.name = name; r.start_time = st; r.end_time = ed;
  for (const CranedId& n : nodes) r.res_total[n] = share(first_core, cores);
  return r;
}
static std::unique_ptr<RnJobInScheduler> job(job_id_t id, TimeSec end, const Names& nodes, uint32_t first_core = 0, const std::string& rsv = "") {
  auto j = std::make_unique<RnJobInScheduler>();
  j->job_id = id; j->partition_id = "P"; j->reservation = rsv; j->start_time = 10; j->end_time = end;
  for (const CranedId& n : nodes) j->allocated_res[n] = share(first_core, 1);
  return j;
}
static Names names(int n) {
  Names v;
  for (int i = 0; i < n; ++i) v.push_back("n" + std::to_string(i));
  return v;
}
static bool is(const Algo::ResvAnswer& a, bool ok, TimeSec start, const Names& chosen, const Names& conflicted, const Names& not_found) {
  const bool same = a.ok == ok && !a.in_the_past && a.start == start && a.chosen == chosen && a.conflicted == conflicted && a.not_found == not_found;
  if (!same) {
    printf("  got ok=%d start=%lld chosen:", (int)a.ok, (long long)a.start);
    for (auto& n : a.chosen) printf(" %s", n.c_str());
    printf(" | conflicted:");
    for (auto& n : a.conflicted) printf(" %s", n.c_str());
    printf(" | not found:");
    for (auto& n : a.not_found) printf(" %s", n.c_str());
    printf("\n");
  }
  return same;
}
// the running set reaches the adapter's packed tables through a cycle (here: one small job in the queue)
static void load(Algo& algo, const ClusterSnapshot& snap, TimeSec now, const std::vector<std::unique_ptr<RnJobInScheduler>>& running) {
  algo.SetClusterSnapshot(snap);
  CHECK(algo.Ok());
  std::vector<std::unique_ptr<PdJobInScheduler>> queue;
  queue.push_back(std::make_unique<PdJobInScheduler>());
  queue[0]->job_id = 9000; queue[0]->partition_id = "P"; queue[0]->time_limit = 60;
  queue[0]->req_task_res_view.cpu_count = cpu_t(1); queue[0]->req_task_res_view.memory_bytes = 1ull << 30;
  algo.NodeSelect(now, running, queue);
  if (!algo.Ok()) printf("NodeSelect: %s\n", algo.LastError().c_str());
  CHECK(algo.Ok());
}

// A: every boundary of :4395 and :4405, the node count, the earliest start.  now = 1000; requests of 600 s from 1500.
//    n0 idle | n1 job until 2000 | n2 job until 1500 (== start: free) | n3 reserved [1000, 1500) (ends at the start: free)
//    n4 reserved [2100, 3000) (begins at start + duration: free) | n5 reserved [2099, 3000) (one second earlier: conflict)
static void cluster_a(Algo& algo) {
  ClusterSnapshot snap;
  const Names ids = names(6);
  for (const auto& n : ids) snap.craned_metas.push_back(node(n));
  snap.partitions = {{"P", ids}};
  snap.reservations = {resv("r3", 1000, 1500, {"n3"}), resv("r4", 2100, 3000, {"n4"}), resv("r5", 2099, 3000, {"n5"})};
  std::vector<std::unique_ptr<RnJobInScheduler>> running;
  running.push_back(job(1, 2000, {"n1"}));
  running.push_back(job(2, 1500, {"n2"}));
  load(algo, snap, 1000, running);
  Names with_ghost = ids;
  with_ghost.push_back("ghost");
  std::vector<Algo::ResvRequest> rq = {
      {1500, 600, 0, with_ghost, false},   // all seven: the ghost counts towards k, 4 free -> no
      {1500, 600, 4, with_ghost, false},   // exactly the free ones
      {1500, 600, 5, with_ghost, false},   // one more than there are
      {1500, 600, 5, ids, true},           // 1500: 4 free; 2000: n1 frees, but n4 is now blocked (2000 + 600 > 2100): 4; 3000: all six
      {300, 700, 1, ids, false},           // ends at now: in the past (:4323)
      {1500, 600, 1, {"n1"}, true},        // its job ends at 2000
      {1500, 599, 0, {"n5", "n4"}, false}, // one second shorter: n5 fits too (2099 is not < 2099)
  };
  auto a = algo.QueryReservation(1000, rq);
  CHECK(algo.Ok() && a.size() == rq.size());
  if (a.size() != rq.size()) return;
  CHECK(is(a[0], false, 0, {}, {"n1", "n5"}, {"ghost"}));
  CHECK(is(a[1], true, 1500, {"n0", "n2", "n3", "n4"}, {"n1", "n5"}, {"ghost"}));
  CHECK(is(a[2], false, 0, {}, {"n1", "n5"}, {"ghost"}));
  CHECK(is(a[3], true, 3000, {"n0", "n1", "n2", "n3", "n4"}, {}, {}));
  CHECK(a[4].in_the_past && !a[4].ok && a[4].chosen.empty() && a[4].conflicted.empty());
  CHECK(is(a[5], true, 2000, {"n1"}, {}, {}));
  CHECK(is(a[6], true, 1500, {"n5", "n4"}, {}, {}));
  // a node named twice, a duration of 0: refused, nothing thrown
  CHECK(algo.QueryReservation(1000, std::vector<Algo::ResvRequest>{{1500, 600, 1, {"n0", "n0"}, false}}).empty() && algo.LastStatus() == CNS_ERR_INVALID_ARG);
  CHECK(algo.QueryReservation(1000, std::vector<Algo::ResvRequest>{{1500, 600, 1, {"zz", "zz"}, false}}).empty() && algo.LastStatus() == CNS_ERR_INVALID_ARG);
  CHECK(algo.QueryReservation(1000, std::vector<Algo::ResvRequest>{{1500, 0, 1, {"n0"}, false}}).empty() && algo.LastStatus() == CNS_ERR_INVALID_ARG);
  CHECK(algo.QueryReservation(1000, std::vector<Algo::ResvRequest>{}).empty() && algo.Ok());
}

// B: what the cycle's own tables drop and CreateResv_ does not (:4391-4400, static_meta :4413).  now = 1000.
//    n0 active reservation "in" [500, 6000) with a job INSIDE it until 5000 | n1 dead, its job (until 4000) still in the map
//    n2 drained and in no partition, idle | n3 idle
//    n4 expired reservation "old" [100, 900) with a job INSIDE it that still runs until 2500: no reservation overlaps a window from 1000,
//       so only the running job can conflict — it must not be dropped with the reservation it runs in
static void cluster_b(Algo& algo) {
  ClusterSnapshot snap;
  const Names ids = names(4);
  for (const auto& n : names(5)) snap.craned_metas.push_back(node(n));
  snap.craned_metas[1].alive = false;
  snap.craned_metas[2].drain = true;
  snap.partitions = {{"P", {"n0", "n1", "n3", "n4"}}};
  snap.reservations = {resv("in", 500, 6000, {"n0"}, 4, 4), resv("old", 100, 900, {"n4"}, 4, 4)};
  std::vector<std::unique_ptr<RnJobInScheduler>> running;
  running.push_back(job(1, 5000, {"n0"}, 4, "in"));
  running.push_back(job(2, 4000, {"n1"}));
  running.push_back(job(3, 2500, {"n4"}, 4, "old"));
  load(algo, snap, 1000, running);
  std::vector<Algo::ResvRequest> rq = {
      {1000, 100, 1, ids, false},          // n2: drained and outside every partition, still a node (:4384)
      {1000, 100, 3, ids, false},
      {5000, 100, 1, {"n0"}, false},       // the job inside the reservation is over, the reservation is not
      {1000, 100, 1, {"n0"}, true},        // ... it ends at 6000
      {1000, 100, 4, ids, true},           // n1's job ends at 4000, n0 frees at 6000
      {4000, 100, 3, {"n0", "n1", "n3"}, true},
      {1000, 100, 1, {"n4"}, false},       // the job inside the expired reservation still runs
      {1000, 100, 1, {"n4"}, true},        // ... until 2500
      {2500, 100, 1, {"n4", "n3"}, false},
  };
  auto a = algo.QueryReservation(1000, rq);
  CHECK(algo.Ok() && a.size() == rq.size());
  if (a.size() != rq.size()) return;
  CHECK(is(a[0], true, 1000, {"n2"}, {"n0", "n1"}, {}));
  CHECK(is(a[1], false, 0, {}, {"n0", "n1"}, {}));
  CHECK(is(a[2], false, 0, {}, {"n0"}, {}));
  CHECK(is(a[3], true, 6000, {"n0"}, {}, {}));
  CHECK(is(a[4], true, 6000, {"n0", "n1", "n2", "n3"}, {}, {}));
  CHECK(is(a[5], true, 6000, {"n0", "n1", "n3"}, {}, {}));
  CHECK(is(a[6], false, 0, {}, {"n4"}, {}));
  CHECK(is(a[7], true, 2500, {"n4"}, {}, {}));
  CHECK(is(a[8], true, 2500, {"n4"}, {}, {}));
  // a second call without a new pack reuses the engine's tables: the same answers
  auto again = algo.QueryReservation(1000, rq);
  CHECK(algo.Ok() && again.size() == a.size());
  for (size_t i = 0; i < again.size() && i < a.size(); ++i)
    CHECK(again[i].ok == a[i].ok && again[i].start == a[i].start && again[i].chosen == a[i].chosen && again[i].conflicted == a[i].conflicted);
}

// C: the free count is not monotone, reservations that overlap on a node, ends that never come.  now = 0.
//    n0 job until 50 | n1 reserved [120, 300) | n2 reserved [100, 200) and [150, 400) | n3 job that never ends
//    n4 reserved [500, never)
static void cluster_c(Algo& algo) {
  ClusterSnapshot snap;
  const Names ids = names(5);
  for (const auto& n : ids) snap.craned_metas.push_back(node(n));
  snap.partitions = {{"P", ids}};
  snap.reservations = {resv("a", 120, 300, {"n1"}), resv("b", 100, 200, {"n2"}, 2, 2), resv("c", 150, 400, {"n2"}, 4, 2),
                       resv("d", 500, INT64_MAX, {"n4"})};
  std::vector<std::unique_ptr<RnJobInScheduler>> running;
  running.push_back(job(1, 50, {"n0"}));
  running.push_back(job(2, INT64_MAX, {"n3"}));
  load(algo, snap, 0, running);
  std::vector<Algo::ResvRequest> rq = {
      {1, 100, 2, {"n0", "n1"}, true},     // 1: n1 only; 50: n0 frees, n1 blocked (50 + 100 > 120); 300: both
      {1, 20, 2, {"n0", "n1"}, true},      // 20 s fit in front of n1's reservation at 50
      {90, 50, 1, {"n2"}, true},           // 200 ends the first, the second still holds: 400
      {10, 90, 1, {"n2"}, true},           // [10, 100) ends where the first begins
      {1, 10, 1, {"n3"}, true},            // never
      {600, 10, 1, {"n4", "n3"}, true},    // never either
      {100, 10, 1, {"n4", "n3"}, true},    // in front of n4's reservation
      {1, 100, 0, {"n0", "n1", "n2", "n4"}, true},   // n4 is free until 400 for 100 s, n2 from 400: all four at 400
  };
  auto a = algo.QueryReservation(0, rq);
  CHECK(algo.Ok() && a.size() == rq.size());
  if (a.size() != rq.size()) return;
  CHECK(is(a[0], true, 300, {"n0", "n1"}, {}, {}));
  CHECK(is(a[1], true, 50, {"n0", "n1"}, {}, {}));
  CHECK(is(a[2], true, 400, {"n2"}, {}, {}));
  CHECK(is(a[3], true, 10, {"n2"}, {}, {}));
  CHECK(is(a[4], false, 0, {}, {"n3"}, {}));
  CHECK(is(a[5], false, 0, {}, {"n4", "n3"}, {}));
  CHECK(is(a[6], true, 100, {"n4"}, {"n3"}, {}));
  CHECK(is(a[7], true, 400, {"n0", "n1", "n2", "n4"}, {}, {}));
}

// D: an empty cluster state (no job, no reservation) and lists longer than a workgroup's chunk.
static void cluster_d(Algo& algo) {
  ClusterSnapshot snap;
  const Names ids = names(700);
  for (const auto& n : ids) snap.craned_metas.push_back(node(n));
  snap.partitions = {{"P", ids}};
  load(algo, snap, 0, {});
  Names rev(ids.rbegin(), ids.rend());
  auto a = algo.QueryReservation(0, std::vector<Algo::ResvRequest>{{10, 10, 3, rev, false}, {10, 10, 0, rev, true}});
  CHECK(algo.Ok() && a.size() == 2);
  if (a.size() != 2) return;
  CHECK(is(a[0], true, 10, {"n699", "n698", "n697"}, {}, {}));
  CHECK(is(a[1], true, 10, rev, {}, {}));
}

// ---- --bench -------------------------------------------------------------------------------------------------------------------
// JobScheduler.cpp:4383-4419 over dense tables, single thread: per node the running ends and the (start, end) of its reservations
struct CpuState {
  std::vector<std::vector<int64_t>> ends;
  std::vector<std::vector<std::pair<int64_t, int64_t>>> resv;
};
static bool cpu_walk(const CpuState& s, int64_t start, int64_t dur, uint32_t k, const uint32_t* cand, size_t len, std::vector<uint32_t>& chosen) {
  const int64_t end = start > INT64_MAX - dur ? INT64_MAX : start + dur;
  chosen.clear();
  for (size_t i = 0; i < len; ++i) {
    const uint32_t n = cand[i];
    if (n >= s.ends.size()) continue;
    bool failed = false;
    for (int64_t e : s.ends[n]) if (e > start) { failed = true; break; }
    if (failed) continue;
    for (const auto& [st, ed] : s.resv[n]) if (st < end && ed > start) { failed = true; break; }
    if (failed) continue;
    chosen.push_back(n);
    if (chosen.size() >= k) break;
  }
  return chosen.size() >= k;
}
static int64_t cpu_earliest(const CpuState& s, int64_t start, int64_t dur, uint32_t k, const uint32_t* cand, size_t len, std::vector<uint32_t>& chosen) {
  std::vector<int64_t> ts{start};
  for (size_t i = 0; i < len; ++i) {
    if (cand[i] >= s.ends.size()) continue;
    for (int64_t e : s.ends[cand[i]]) if (e >= start && e != INT64_MAX) ts.push_back(e);
    for (const auto& iv : s.resv[cand[i]]) if (iv.second >= start && iv.second != INT64_MAX) ts.push_back(iv.second);
  }
  std::sort(ts.begin(), ts.end());
  ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
  for (int64_t t : ts) if (cpu_walk(s, t, dur, k, cand, len, chosen)) return t;
  return -1;
}

static int bench() {
  // 65 536 nodes, a third of them busy (ends on a grid of 64 times), a third reserved once or twice; tables straight through the C ABI
  const uint32_t N = 65536;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  CpuState cs;
  cs.ends.resize(N); cs.resv.resize(N);
  std::vector<int64_t> r_end, v_st, v_ed;
  std::vector<uint32_t> r_off{0}, r_node, v_off{0}, v_node;
  for (uint32_t n = 0; n < N; ++n)
    for (int i = 0, m = rnd() % 3 == 0 ? 1 + (int)(rnd() % 4) : 0; i < m; ++i) {
      const int64_t e = 1000 + 600 * (int64_t)(rnd() % 64);
      cs.ends[n].push_back(e); r_end.push_back(e); r_node.push_back(n); r_off.push_back((uint32_t)r_node.size());
    }
  for (uint32_t v = 0; v < 256; ++v) {
    const int64_t st = 1000 + 600 * (int64_t)(rnd() % 48), ed = st + 600 * (1 + (int64_t)(rnd() % 16));
    v_st.push_back(st); v_ed.push_back(ed);
    for (uint32_t n = 0; n < N; ++n) if (rnd() % 512 == 0) { v_node.push_back(n); cs.resv[n].push_back({st, ed}); }
    v_off.push_back((uint32_t)v_node.size());
  }
  cns_config cfg{};
  cfg.abi_version = CNS_ABI_VERSION;
  cns_handle* h = nullptr;
  if (cns_create(&cfg, &h) != 0) { printf("cns_create: %s\n", cns_last_error(nullptr)); return 1; }
  std::vector<int64_t> cpu(N, 8 * 256);
  std::vector<uint64_t> mem(N, 32ull << 30), lo(N, 0xFF);
  std::vector<uint32_t> poff{0, N}, pnodes(N);
  for (uint32_t n = 0; n < N; ++n) pnodes[n] = n;
  cns_node_soa nd{};
  nd.num_nodes = N; nd.num_partitions = 1; nd.cpu_total_raw = cpu.data(); nd.mem_total = mem.data(); nd.core_lo = lo.data();
  nd.part_offsets = poff.data(); nd.part_nodes = pnodes.data();
  cns_running_soa rs{};
  rs.num_jobs = (uint32_t)r_end.size(); rs.num_allocs = (uint32_t)r_node.size(); rs.end_sec = r_end.data(); rs.alloc_offsets = r_off.data(); rs.alloc_node = r_node.data();
  cns_resv_soa rv{};
  rv.num_resv = (uint32_t)v_st.size(); rv.num_allocs = (uint32_t)v_node.size(); rv.start_sec = v_st.data(); rv.end_sec = v_ed.data();
  rv.alloc_offsets = v_off.data(); rv.alloc_node = v_node.data();
  if (cns_set_nodes(h, &nd) != 0 || cns_resvq_set_state(h, &rs, &rv) != 0) { printf("setup: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
  int rc = 0;
  for (const auto& [Q, L] : {std::pair<uint32_t, uint32_t>{1, 65536}, {1024, 4096}})
    for (int mode = 0; mode < 2; ++mode) {
      std::vector<int64_t> start(Q, 1000), dur(Q, 4 * 3600);
      std::vector<uint32_t> k(Q), cand((size_t)Q * L);
      std::vector<uint64_t> off(Q + 1);
      std::vector<uint8_t> fe(Q, (uint8_t)mode);
      for (uint32_t q = 0; q < Q; ++q) {
        const uint32_t base = (uint32_t)(rnd() % N);   // a window of L consecutive nodes, shuffled by a stride coprime to L
        for (uint32_t i = 0; i < L; ++i) cand[(size_t)q * L + i] = (base + (uint32_t)(((uint64_t)i * 2654435761ull) % L)) % N;
        off[q + 1] = (uint64_t)(q + 1) * L;
        k[q] = mode ? L - L / 16 : L / 2;               // given start: about two thirds are free; earliest: all but a sixteenth -> it has to wait
      }
      cns_resvq_soa qs{};
      qs.num_queries = Q; qs.start_sec = start.data(); qs.duration_sec = dur.data(); qs.node_num = k.data(); qs.cand_offsets = off.data();
      qs.cand_nodes = cand.data(); qs.find_earliest = fe.data();
      std::vector<uint8_t> status(Q), code((size_t)Q * L);
      std::vector<int64_t> ostart(Q);
      std::vector<uint32_t> nfree(Q), chosen((size_t)Q * L);
      std::vector<uint64_t> choff(Q + 1);
      cns_resvq_out out{};
      out.code_capacity = code.size(); out.chosen_capacity = chosen.size(); out.status = status.data(); out.start_sec = ostart.data();
      out.num_free = nfree.data(); out.code = code.data(); out.chosen_offsets = choff.data(); out.chosen_nodes = chosen.data();
      double gpu[4] = {0, 0, 0, 0}, host[4] = {0, 0, 0, 0};
      std::vector<int64_t> cpu_start(Q);
      std::vector<uint32_t> tmp, cpu_first(Q, CNS_NODE_NONE);
      for (int r = 0; r < 4; ++r) {   // run 0 is the warm-up
        if (cns_resvq_run(h, 0, &qs, &out, &gpu[r]) != 0) { printf("cns_resvq_run: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t q = 0; q < Q; ++q) {
          const uint32_t* c = cand.data() + (size_t)q * L;
          if (mode) cpu_start[q] = cpu_earliest(cs, start[q], dur[q], k[q], c, L, tmp);
          else cpu_start[q] = cpu_walk(cs, start[q], dur[q], k[q], c, L, tmp) ? start[q] : -1;
          cpu_first[q] = cpu_start[q] >= 0 && !tmp.empty() ? tmp[0] : CNS_NODE_NONE;
        }
        host[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
      size_t okq = 0;
      for (uint32_t q = 0; q < Q; ++q) {   // the two agree (the loop is a baseline, not a second oracle: start and first chosen node only)
        const bool ok = status[q] == CNS_RESVQ_OK;
        okq += ok;
        if (ok != (cpu_start[q] >= 0) || (ok && (ostart[q] != cpu_start[q] || chosen[choff[q]] != cpu_first[q]))) { printf("  query %u: GPU and CPU loop differ\n", q); rc = 1; break; }
      }
      std::sort(gpu + 1, gpu + 4); std::sort(host + 1, host + 4);
      printf("%4u x %5u candidates, %-8s: kernel_ms median %.3f (min %.3f max %.3f) | CPU loop ms median %.3f (min %.3f max %.3f) | ratio %.1fx | %zu ok, first start %lld\n",
             Q, L, mode ? "earliest" : "given", gpu[2], gpu[1], gpu[3], host[2], host[1], host[3], host[2] / gpu[2], okq, (long long)ostart[0]);
    }
  cns_destroy(h);
  return rc;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--bench")) return bench();
  if (argc > 1 && !strcmp(argv[1], "--no-gpu")) {
    Algo algo(0);
    auto a = algo.QueryReservation(0, std::vector<Algo::ResvRequest>{{10, 10, 1, {"n0"}, false}});
    CHECK(a.empty() && !algo.Ok());
    printf("%s\n", g_fail ? "FAIL" : "ok (no device: QueryReservation is loud)");
    return g_fail ? 1 : 0;
  }
  { Algo algo(0); CHECK(algo.QueryReservation(0, std::vector<Algo::ResvRequest>{}).empty() && algo.LastStatus() == CNS_ERR_STATE); }   // no snapshot yet
  { Algo algo(0); cluster_a(algo); }
  { Algo algo(0); cluster_b(algo); }
  { Algo algo(0); cluster_c(algo); }
  { Algo algo(0); cluster_d(algo); }
  printf("%s\n", g_fail ? "FAIL" : "ok: QueryReservation on 4 hand-made clusters");
  return g_fail ? 1 : 0;
}
