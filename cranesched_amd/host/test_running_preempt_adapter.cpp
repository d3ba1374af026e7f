// Drives GpuNodeSelectionAlgo with UseResidentRunning(true) AND a snapshot that has preempt_enabled (include/crane_gpu_running/
// running_preempt.h): three consecutive cycles through NodeSelect, each built from the previous one's results, once with the running set
// handed in every cycle (cns_set_running + cns_select_preempt) and once with it kept on the device (cns_running_select_preempt) — every
// job's reason, start, nodes, allocated cores and preempted list, the cancelled ids and the preempting set must be identical — and, with
// --bench, what the two paths spend per cycle boundary in front of the cycle.
//   test_running_preempt_adapter            -> needs an MI355X, exit 0 on success
//   test_running_preempt_adapter --no-gpu   -> the loud "no device" behaviour instead
//   test_running_preempt_adapter --bench [jobs] [nodes]   -> 65 536 nodes in 8 partitions, 1 M running jobs (90 % one-node, the rest 2..8), a QoS
//                                    that may preempt on the pending jobs of partition 0, per step 1 % retired and 1 % admitted: (a) cns_set_running
//                                    + what cns_select_preempt spends before its cycle, (b) cns_running_advance + what cns_running_select_preempt
//                                    spends before its cycle, by stage, first call behind an advance and a second one; one warm-up, medians of 5.
//                                    Asserted there: the cycles behind either give the same digest.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_running/running_preempt.h"

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

static std::unique_ptr<PdJobInScheduler> job(job_id_t id, const std::string& part, double cpu, int64_t limit, bool high, double prio, const std::string& resv = "") {
  auto j = std::make_unique<PdJobInScheduler>();
  j->job_id = id;
  j->partition_id = part;
  j->reservation = resv;
  j->time_limit = limit;
  j->req_task_res_view.cpu_count = cpu_t(cpu);
  j->req_task_res_view.memory_bytes = G;
  j->qos = high ? "high" : "low"; j->qos_priority = high ? 10 : 1; j->priority = prio;
  return j;
}

static std::unique_ptr<RnJobInScheduler> running(job_id_t id, const std::string& craned, std::vector<uint32_t> cores, TimeSec start, TimeSec end, const std::string& resv = "") {
  auto r = std::make_unique<RnJobInScheduler>();
  r->job_id = id; r->start_time = start; r->end_time = end; r->reservation = resv; r->qos = "low"; r->qos_priority = 1;
  ResourceInNodeV3& res = r->allocated_res[craned];
  res.cpu_set.cpu_count = cpu_t((double)cores.size());
  for (uint32_t c : cores) res.cpu_set.core_ids.insert(c);
  res.memory_bytes = cores.size() * G;
  return r;
}

// three cycles; *trace: one line per job and cycle, one per cycle for the cancelled ids and the preempting set
static bool three_cycles(bool resident, std::vector<std::string>* trace, size_t* admitted_total, size_t* preempted_total) {
  GpuNodeSelectionAlgo algo(0);
  // p0 = {n0..n5}, p1 = {n1 n3 n5} (shared nodes: an allocation counts on two slots), 8 cores / 32 GiB each; reservation "r0" takes four
  // cores of n4 and n5 until NOW + 50000.  QoS "high" may preempt "low".
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
  snap.preempt_enabled = true;
  snap.qos_preempt = {{"high", {"low"}}, {"low", {}}};
  algo.SetClusterSnapshot(snap);
  if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return false; }
  // a crowded cluster: six of the eight cores of n0..n3 are taken by low jobs, so a high job of four cores must preempt
  std::vector<std::unique_ptr<RnJobInScheduler>> run;
  for (int i = 0; i < 4; ++i) run.push_back(running(1 + i, "n" + std::to_string(i), {0, 1, 2, 3, 4, 5}, NOW - 100 - 7 * i, NOW + 3000 + 500 * i));
  run.push_back(running(5, "n4", {0, 1}, NOW - 200, NOW + 700, "r0"));
  run.push_back(running(6, "n5", {4, 5, 6, 7}, NOW - 300, NOW + 5000));
  run.push_back(running(7, "n4", {4, 5, 6}, NOW - 400, NOW + 400));
  if (resident) {
    algo.UseResidentRunning(true);
    if (!algo.SeedRunning(run)) { printf("SeedRunning: %s\n", algo.LastError().c_str()); return false; }
  }
  for (int c = 0; c < 3; ++c) {
    const TimeSec now = NOW + STEP * c;
    std::vector<std::unique_ptr<PdJobInScheduler>> pd;
    for (int i = 0; i < 10; ++i) {
      const job_id_t id = 100 * (c + 1) + i;
      if (i == 3) pd.push_back(job(id, "p0", 1, 400, false, 100 - i, "r0"));   // inside the reservation
      else pd.push_back(job(id, i % 3 == 1 ? "p1" : "p0", i % 2 ? 1 : 4, 200 + 250 * (i % 4), i % 2 == 0, 100 - i));
    }
    if (c == 1) {   // a craned goes down and comes back between two cycles: a new snapshot, the ledger stays
      snap.craned_metas[2].alive = false;
      algo.SetClusterSnapshot(snap);
      snap.craned_metas[2].alive = true;
      algo.SetClusterSnapshot(snap);
      if (!algo.Ok()) { printf("snapshot: %s\n", algo.LastError().c_str()); return false; }
    }
    algo.NodeSelect(now, run, pd);   // (resident: the contents of `run` are read for qos / qos_priority / start_time only, by id)
    if (!algo.Ok()) { printf("NodeSelect (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
    std::vector<const PdJobInScheduler*> admitted;
    for (const auto& j : pd) {
      std::string line = "c" + std::to_string(c) + " job " + std::to_string(j->job_id) + " '" + j->reason + "' " + std::to_string(j->start_time);
      for (const CranedId& id : j->craned_ids) {
        line += " " + id + ":";
        for (uint32_t core : j->allocated_res.at(id).cpu_set.core_ids) line += std::to_string(core) + ",";
      }
      bool waits = false;   // it preempted a running job: the commit loop holds it back (JobScheduler.cpp:1542-1555)
      line += " pre:";
      for (const PreemptedJob& p : j->preempted_jobs) {
        if (std::holds_alternative<RnJobInScheduler*>(p)) { line += "R" + std::to_string(std::get<RnJobInScheduler*>(p)->job_id) + ","; waits = true; }
        else line += "P" + std::to_string(std::get<PdJobInScheduler*>(p)->job_id) + ",";
      }
      *preempted_total += j->preempted_jobs.size();
      trace->push_back(line);
      if (j->reason.empty() && j->start_time == now && !waits) admitted.push_back(j.get());
    }
    std::string line = "c" + std::to_string(c) + " cancelled:";
    for (job_id_t id : algo.LastPreemptCancel()) line += std::to_string(id) + ",";
    line += " preempting:";
    for (job_id_t id : algo.PreemptingSet()) line += std::to_string(id) + ",";
    trace->push_back(line);
    // the boundary: what was cancelled or ends by the next cycle leaves, what the commit loop started enters — on the caller's vector in
    // ledger order
    std::vector<job_id_t> finished = algo.LastPreemptCancel();
    for (const auto& r : run)
      if (r->end_time <= now + STEP && std::find(finished.begin(), finished.end(), r->job_id) == finished.end()) finished.push_back(r->job_id);
    run.erase(std::remove_if(run.begin(), run.end(), [&](const auto& r) { return std::find(finished.begin(), finished.end(), r->job_id) != finished.end(); }), run.end());
    for (const PdJobInScheduler* j : admitted) {
      auto r = std::make_unique<RnJobInScheduler>();
      r->job_id = j->job_id; r->start_time = j->start_time - (TimeSec)(j->job_id % 100); r->end_time = j->end_time; r->reservation = j->reservation; r->allocated_res = j->allocated_res;
      r->qos = j->qos; r->qos_priority = j->qos_priority;
      run.push_back(std::move(r));
    }
    *admitted_total += admitted.size();
    if (resident) {
      uint64_t nret = 0, nadm = 0;
      if (!algo.AdvanceRunning(finished, admitted, &nret, &nadm)) { printf("AdvanceRunning (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
      CHECK(nret == finished.size() && nadm == admitted.size());
    }
  }
  return true;
}

static int hand_cases() {
  std::vector<std::string> with, without;
  size_t adm[2] = {0, 0}, pre[2] = {0, 0};
  if (!three_cycles(false, &without, &adm[0], &pre[0]) || !three_cycles(true, &with, &adm[1], &pre[1])) return 1;
  CHECK(with.size() == without.size() && with.size() == 33);
  size_t differ = 0;
  for (size_t i = 0; i < std::min(with.size(), without.size()); ++i)
    if (with[i] != without[i]) { if (!differ++) printf("first difference:\n  handed in: %s\n  resident:  %s\n", without[i].c_str(), with[i].c_str()); }
  CHECK(differ == 0);
  CHECK(adm[0] == adm[1] && pre[0] == pre[1] && adm[0] >= 3 && pre[0] >= 2);
  for (const std::string& l : with) printf("  %s\n", l.c_str());
  printf("hand cases: 3 cycles with preemption, %zu jobs admitted, %zu preempted, %zu lines differ, %d failures\n", adm[1], pre[1], differ, g_fail);
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
  // the queue of a step: 1 % of R one-node jobs of one core; the jobs of partition 0 carry the QoS that may preempt
  const size_t J = std::max<size_t>(R / 100, 1);
  std::vector<uint32_t> jpart(J), one(J, 1), jid(J), pd_id(J), pd_qos(J), pd_qp(J);
  std::vector<double> pd_prio(J);
  std::vector<int64_t> jl(J, 3600), jcpu(J, 256);
  std::vector<uint64_t> jmem(J, G), zero64(J, 0);
  for (size_t j = 0; j < J; ++j) { jpart[j] = (uint32_t)(j % P); pd_id[j] = (uint32_t)j; pd_qos[j] = jpart[j] == 0; pd_qp[j] = pd_qos[j] ? 10 : 1; pd_prio[j] = (double)(J - j) + 0.5; }
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
  const uint32_t qoff[3] = {0, 0, 1}, qflat[1] = {0};   // QoS 1 may preempt QoS 0
  const size_t Rcap = R + 8 * J;
  std::vector<uint32_t> rn_qos(Rcap, 0), rn_qp(Rcap, 1), po_refs(4 * (J + Rcap) + 64), po_cancel(Rcap + 1), po_set(Rcap + 2), set_in{ids[1], ids[R / 2], 0xFFFFFFF0u};
  std::vector<int64_t> rn_start(Rcap);
  std::vector<uint64_t> po_off(J + 1);
  std::vector<double> costs(N);
  // one cycle with preemption over the ledger rows `rows` (their ids, in ledger order), resident or through cns_select_preempt
  auto cycle_digest = [&](bool resident, int64_t now, const std::vector<uint32_t>& rows, size_t nrows, uint64_t* digest, cns_running_preempt_timing* tm) {
    for (size_t r = 0; r < nrows; ++r) rn_start[r] = NOW - 1 - (int64_t)rows[r];
    cns_preempt_soa ps{};
    ps.enabled = 1; ps.num_qos = 2; ps.qos_preempt_offsets = qoff; ps.qos_preempt = qflat;
    ps.pd_job_id = pd_id.data(); ps.pd_qos = pd_qos.data(); ps.pd_qos_priority = pd_qp.data(); ps.pd_priority = pd_prio.data();
    ps.rn_job_id = rows.data(); ps.rn_qos = rn_qos.data(); ps.rn_qos_priority = rn_qp.data(); ps.rn_start_sec = rn_start.data();
    ps.num_preempting = (uint32_t)set_in.size(); ps.preempting_job_ids = set_in.data();
    cns_preempt_out po{};
    po.capacity = po_refs.size(); po.offsets = po_off.data(); po.preempted = po_refs.data();
    po.cancel_capacity = (uint32_t)po_cancel.size(); po.cancelled_job_ids = po_cancel.data();
    po.preempting_capacity = (uint32_t)po_set.size(); po.preempting_job_ids = po_set.data();
    if ((resident ? cns_running_select_preempt(h, now, &js, &ps, &out, &po) : cns_select_preempt(h, now, &js, &ps, &out, &po)) != 0) return false;
    if (cns_running_preempt_get_timing(h, tm) != 0) return false;
    if (cns_debug_get_costs(h, costs.data()) != 0) return false;
    uint64_t d = fnv(1469598103934665603ull, ostart.data(), J * 8);
    d = fnv(d, oreason.data(), J); d = fnv(d, onode.data(), J * 4); d = fnv(d, olo.data(), J * 8); d = fnv(d, costs.data(), (size_t)N * 8);
    d = fnv(d, po_off.data(), (J + 1) * 8); d = fnv(d, po_set.data(), (size_t)po.num_preempting * 4);
    *digest = d;
    return true;
  };
  auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  if (cns_running_seed(h, &rn, ids.data()) != 0) return die("cns_running_seed");
  std::vector<double> adv_ms, set_ms, a_setup, b_first, b_first_index, b_first_mark, b_again, b_again_mark;
  std::vector<uint32_t> rows = ids;
  size_t nrows = R;
  int rc = 0;
  uint32_t next_id = (uint32_t)R + 1;
  size_t cursor = 0;
  std::vector<uint8_t> found(R / 100 + 1), mask(J, 1);
  cns_running_preempt_timing tm{};
  cns_running_timing rt{};
  for (int step = 0; step < 6; ++step) {   // one warm-up, then 5 steps, each from what the previous one left
    const int64_t now = NOW + 2 * step;
    uint64_t d0 = 0, d0b = 0, d1 = 0, d2 = 0;
    // (b) the first call behind a seed / an advance builds the index, a second one reuses it
    if (!cycle_digest(true, now, rows, nrows, &d0, &tm)) return die("cns_running_select_preempt");
    if (step) { b_first.push_back(tm.setup_ms); b_first_index.push_back(tm.index_ms); b_first_mark.push_back(tm.mark_ms); }
    if (!tm.index_built) rc = 1;
    if (!cycle_digest(true, now, rows, nrows, &d0b, &tm)) return die("cns_running_select_preempt");
    if (step) { b_again.push_back(tm.setup_ms); b_again_mark.push_back(tm.mark_ms); }
    if (tm.index_built || d0 != d0b) rc = 1;
    // 1 % retired: the next R / 100 seeded ids; 1 % admitted: the cycle's jobs (nothing preempts on this cluster: the mask is all ones)
    std::vector<uint32_t> retire;
    for (size_t k = 0; k < R / 100 && cursor < R; ++k) retire.push_back(ids[cursor++]);
    for (size_t j = 0; j < J; ++j) jid[j] = next_id++;
    cns_running_step in{};
    in.num_retire = retire.size(); in.retire_ids = retire.data(); in.num_jobs = J; in.now_sec = now; in.job_id = jid.data(); in.admit = mask.data();
    uint64_t nret = 0, nadm = 0;
    const cns_running_step_out so{found.data(), &nret, &nadm};
    const auto t0 = std::chrono::steady_clock::now();
    if (cns_running_advance(h, &in, &so) != 0) return die("cns_running_advance");
    if (step) adv_ms.push_back(ms_since(t0));
    cns_running_get_timing(h, &rt);
    if (nret != retire.size() || nadm == 0) rc = 1;
    // the same ledger as arrays, through the path this one replaces (it drops the ledger: seeded again behind it)
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
    if (lr > Rcap) { printf("the ledger outgrew the bench's arrays\n"); cns_destroy(h); return 1; }
    rows.assign(gid.begin(), gid.begin() + lr); nrows = lr;
    if (!cycle_digest(true, now + 1, rows, nrows, &d1, &tm)) return die("cns_running_select_preempt");
    cns_running_soa full{};
    full.num_jobs = (uint32_t)lr; full.num_allocs = (uint32_t)la; full.end_sec = gend.data(); full.alloc_offsets = goff.data(); full.alloc_node = gnode.data();
    full.alloc_cpu_raw = gcpu.data(); full.alloc_mem = gmem.data(); full.alloc_core_lo = glo.data(); full.alloc_core_hi = ghi.data(); full.alloc_gres = gg.data();
    full.reservation = gresv.data(); full.alloc_core_w2 = gw2.data(); full.alloc_core_w3 = gw3.data();
    const auto t1 = std::chrono::steady_clock::now();
    if (cns_set_running(h, &full) != 0) return die("cns_set_running");
    if (step) set_ms.push_back(ms_since(t1));
    if (!cycle_digest(false, now + 1, rows, nrows, &d2, &tm)) return die("cns_select_preempt");
    if (step) a_setup.push_back(tm.setup_ms);
    if (d1 != d2 || d0 == d1) { printf("step %d: digests %016llx (before) %016llx (resident) %016llx (cns_set_running + cns_select_preempt)\n", step, (unsigned long long)d0, (unsigned long long)d1, (unsigned long long)d2); rc = 1; }
    if (cns_running_seed(h, &full, gid.data()) != 0) return die("cns_running_seed");
  }
  printf("running preempt bench: %u nodes in %u partitions, %zu running jobs seeded (%zu allocations), per step %zu retired and %zu in the queue (%zu with the preempting QoS)\n"
         "  (a) cns_set_running call_ms %.3f + cns_select_preempt before its cycle %.3f = %.3f\n"
         "  (b) cns_running_advance call_ms %.3f + cns_running_select_preempt before its cycle, first call behind the advance %.3f (device: index %.3f, call part %.3f) = %.3f;"
         " a second call on the same tables %.3f (device: call part %.3f)\n"
         "  (medians of 5; 'before its cycle' is on the host clock and holds cns_upload_jobs of the %zu-job queue in both; the ledger after the last step: %llu jobs, %llu allocations, %llu pairs)"
         "  cycle digests %s\n",
         N, P, R, A, R / 100, J, (J + P - 1) / P, median(set_ms), median(a_setup), median(set_ms) + median(a_setup), median(adv_ms), median(b_first), median(b_first_index),
         median(b_first_mark), median(adv_ms) + median(b_first), median(b_again), median(b_again_mark), J, (unsigned long long)rt.jobs, (unsigned long long)rt.allocs,
         (unsigned long long)rt.pairs, rc ? "DIFFER" : "equal");
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
      const std::vector<std::unique_ptr<PdJobInScheduler>> nopd;
      algo.UseResidentRunning(true);
      algo.NodeSelect(NOW, none, nopd);
      CHECK(!algo.Ok() && algo.LastStatus() != 0);
      printf("no device: NodeSelect refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
      return g_fail ? 1 : 0;
    }
    if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  }
  return hand_cases();
}
