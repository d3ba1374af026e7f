// Drives GpuNodeSelectionAlgo::AmendRunning and QueryReservation on the device ledger (include/crane_gpu_amend/running_amend.h): three
// consecutive cycles through NodeSelect on a small cluster with shared nodes and a reservation; between the cycles a time-limit change
// on a running job (JobScheduler::ChangeJobTimeConstraint), the two running children of an array parent in one call, and a resume that
// moves an end out by the suspended duration (ResumeSuspendedJobs).  Run once with the running set handed in every cycle (the new ends
// written into the RnJobInScheduler objects) and once resident through AmendRunning: every job's reason, start, nodes and allocated
// cores and every answer of QueryReservation must be identical.
//   test_running_amend_adapter            -> needs an MI355X, exit 0 on success
//   test_running_amend_adapter --no-gpu   -> the loud "no device" behaviour instead
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_amend/running_amend.h"

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

static std::string answer_line(const char* tag, const GpuNodeSelectionAlgo::ResvAnswer& a) {
  std::string s = std::string(tag) + (a.ok ? " ok " : " no ") + std::to_string(a.start) + " chosen";
  for (const auto& n : a.chosen) s += " " + n;
  s += " conflicted";
  for (const auto& n : a.conflicted) s += " " + n;
  s += " not_found";
  for (const auto& n : a.not_found) s += " " + n;
  return s;
}

static std::vector<GpuNodeSelectionAlgo::ResvRequest> requests(TimeSec now) {
  const std::vector<CranedId> all{"n0", "n1", "n2", "n3", "n4", "n5", "nX"};
  std::vector<GpuNodeSelectionAlgo::ResvRequest> q(3);
  q[0].start = now + STEP; q[0].duration = 300; q[0].node_num = 2; q[0].craned_ids = all;
  q[1].start = now; q[1].duration = 900; q[1].node_num = 4; q[1].craned_ids = all; q[1].find_earliest = true;
  q[2].start = now + 3000; q[2].duration = 60; q[2].node_num = 0; q[2].craned_ids = {"n1", "n3", "n0"};
  return q;
}

// three cycles; *trace: one line per job and cycle, and one per answer of QueryReservation
// apply = false: the caller forgets the amendments (handed in only) — the trace they must change
static bool three_cycles(bool resident, bool apply, std::vector<std::string>* trace, size_t* amended_total) {
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
  run.push_back(running(6, "n2", {0, 1, 2, 3, 4, 5}, NOW + 2500));
  const std::vector<std::unique_ptr<RnJobInScheduler>> nothing;
  if (resident) {
    algo.UseResidentRunning(true);
    if (!algo.SeedRunning(run)) { printf("SeedRunning: %s\n", algo.LastError().c_str()); return false; }
  }
  // the caller's side of an amendment: the new ends into its own objects (all a handed-in cycle needs), and, resident, AmendRunning
  auto amend = [&](const char* what, std::vector<std::pair<job_id_t, TimeSec>> new_ends, size_t known) {
    if (!apply) return true;
    for (const auto& [id, end] : new_ends)
      for (auto& r : run) if (r->job_id == id) r->end_time = end;
    *amended_total += known;
    if (!resident) return true;
    uint64_t n = 0;
    if (!algo.AmendRunning(new_ends, &n)) { printf("AmendRunning (%s): %s\n", what, algo.LastError().c_str()); return false; }
    CHECK(n == known);
    return true;
  };
  std::vector<job_id_t> children;   // the array parent's running children
  for (int c = 0; c < 3; ++c) {
    const TimeSec now = NOW + STEP * c;
    std::vector<std::unique_ptr<PdJobInScheduler>> pd;
    for (int i = 0; i < 12; ++i) {
      const job_id_t id = 100 * (c + 1) + i;
      if (i == 3) pd.push_back(job(id, "p0", 1, 400, 1, "r0"));            // inside the reservation
      else if (i == 7) pd.push_back(job(id, "p0", 2, 900, 3));             // three nodes
      else if (i == 10) pd.push_back(job(id, "p0", 8, 300));               // a whole node: it waits for the last end on one
      else pd.push_back(job(id, i % 2 ? "p1" : "p0", 1 + i % 3, 200 + 250 * (i % 4)));
    }
    algo.NodeSelect(now, resident ? nothing : run, pd);
    if (!algo.Ok()) { printf("NodeSelect (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
    std::vector<const PdJobInScheduler*> admitted;
    for (const auto& j : pd) {
      std::string line = "c" + std::to_string(c) + " job " + std::to_string(j->job_id) + " '" + j->reason + "' " + std::to_string(j->start_time);
      for (const CranedId& id : j->craned_ids) {
        line += " " + id + ":";
        for (uint32_t core : j->allocated_res.at(id).cpu_set.core_ids) line += std::to_string(core) + ",";
      }
      trace->push_back(line);
      if (j->reason.empty() && j->start_time == now) admitted.push_back(j.get());
    }
    // the reservation what-ifs against the running set this cycle ran on
    const auto q = requests(now);
    const auto ans = algo.QueryReservation(now, q);
    if (!algo.Ok() || ans.size() != q.size()) { printf("QueryReservation (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
    for (size_t i = 0; i < ans.size(); ++i) trace->push_back(answer_line(("c" + std::to_string(c) + " query " + std::to_string(i)).c_str(), ans[i]));
    // the boundary: what ended by the next cycle leaves, what the commit loop started enters
    std::vector<job_id_t> finished;
    for (const auto& r : run) if (r->end_time <= now + STEP) finished.push_back(r->job_id);
    run.erase(std::remove_if(run.begin(), run.end(), [&](const auto& r) { return r->end_time <= now + STEP; }), run.end());
    for (const PdJobInScheduler* j : admitted) {
      auto r = std::make_unique<RnJobInScheduler>();
      r->job_id = j->job_id; r->end_time = j->end_time; r->reservation = j->reservation; r->allocated_res = j->allocated_res;
      run.push_back(std::move(r));
    }
    if (resident && !algo.AdvanceRunning(finished, admitted)) { printf("AdvanceRunning (cycle %d): %s\n", c, algo.LastError().c_str()); return false; }
    if (c == 0) {
      // scontrol update timelimit on running job 6: it holds six of n2's eight cores and now ends 1500 s earlier; a job that does not
      // run is the caller's ERR_NON_EXISTENT and changes nothing
      if (!amend("time limit", {{6, NOW + 1000}, {4242, NOW + 5}}, 1)) return false;
    } else if (c == 1) {
      // an array parent's time limit: both running children in one call (two rows that run on into the next cycle: jobs a cycle
      // admitted first, then a seeded one); and a resume: job 5 was suspended for 800 s
      for (int pass = 0; pass < 2; ++pass)
        for (const auto& r : run)
          if (children.size() < 2 && (pass == 0) == (r->job_id >= 100) && r->job_id != 5 && r->end_time > now + STEP) children.push_back(r->job_id);
      CHECK(children.size() == 2);
      std::vector<std::pair<job_id_t, TimeSec>> ends;
      for (job_id_t id : children) ends.push_back({id, now + STEP + 4000 + (TimeSec)id});
      if (!amend("array children", ends, children.size())) return false;
      if (!amend("resume", {{5, NOW + 5000 + 800}}, 1)) return false;
    }
  }
  if (resident && apply) {
    // an amend alone refreshes the what-ifs: job 5 on n3 now ends beyond the asked start, n3 moves from chosen to conflicted
    const TimeSec now = NOW + 3 * STEP;
    GpuNodeSelectionAlgo::ResvRequest r;
    r.start = NOW + 7000; r.duration = 60; r.node_num = 1; r.craned_ids = {"n3"};
    auto a = algo.QueryReservation(now, std::span<const GpuNodeSelectionAlgo::ResvRequest>(&r, 1));
    CHECK(algo.Ok() && a.size() == 1 && a[0].ok && a[0].chosen == std::vector<CranedId>{"n3"});
    uint64_t n = 0;
    CHECK(algo.AmendRunning({{5, NOW + 9000}}, &n) && n == 1);
    a = algo.QueryReservation(now, std::span<const GpuNodeSelectionAlgo::ResvRequest>(&r, 1));
    CHECK(algo.Ok() && a.size() == 1 && !a[0].ok && a[0].conflicted == std::vector<CranedId>{"n3"});
    // an id twice is refused by the engine and says which
    CHECK(!algo.AmendRunning({{5, NOW + 1}, {5, NOW + 2}}) && algo.LastStatus() == CNS_ERR_INVALID_ARG && algo.LastError().find("job id 5 stands twice") != std::string::npos);
  } else if (apply) {
    // with the running set handed in there is nothing to amend on the device
    CHECK(!algo.AmendRunning({{5, NOW + 9000}}) && algo.LastStatus() == CNS_ERR_STATE);
  }
  return true;
}

static int hand_cases() {
  std::vector<std::string> with, without, forgotten;
  size_t am[3] = {0, 0, 0};
  if (!three_cycles(false, true, &without, &am[0]) || !three_cycles(true, true, &with, &am[1]) || !three_cycles(false, false, &forgotten, &am[2])) return 1;
  CHECK(with.size() == without.size() && with.size() == 3 * (12 + 3));
  size_t differ = 0;
  for (size_t i = 0; i < std::min(with.size(), without.size()); ++i)
    if (with[i] != without[i]) { if (!differ++) printf("first difference:\n  handed in: %s\n  resident:  %s\n", without[i].c_str(), with[i].c_str()); }
  CHECK(differ == 0);
  if (g_fail) for (const std::string& l : with) printf("  %s\n", l.c_str());   // (the resident trace, to read a failure from)
  CHECK(am[0] == am[1] && am[0] == 4);
  // a condition on the inputs: the amendments change the jobs of cycles 1 and 2 and the what-ifs (cycle 0 runs before the first one)
  size_t moved_jobs = 0, moved_answers = 0;
  for (size_t i = 0; i < std::min(without.size(), forgotten.size()); ++i)
    if (without[i] != forgotten[i]) { CHECK(i >= 15); ++(without[i].find(" query ") == std::string::npos ? moved_jobs : moved_answers); }
  CHECK(am[2] == 0 && moved_jobs >= 1 && moved_answers >= 1);
  printf("hand cases: 3 cycles, %zu rows amended, %zu lines compared, %zu differ; without the amendments %zu job lines and %zu answers differ; %d failures\n", am[1], with.size(), differ, moved_jobs, moved_answers, g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  {
    GpuNodeSelectionAlgo algo(0);
    if (no_gpu) {
      if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
      algo.UseResidentRunning(true);
      CHECK(!algo.AmendRunning({{1, 5}}) && !algo.Ok() && algo.LastStatus() != 0);
      printf("no device: AmendRunning refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
      return g_fail ? 1 : 0;
    }
    if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  }
  return hand_cases();
}
