// Drives GpuNodeSelectionAlgo::BuildPendingQueue (include/crane_gpu_gate/pending_gate.h): a generated pending map in CraneCtld's shapes
// (jobs in no particular order, DependenciesInJob with an unordered_map) against a single-threaded loop in this file that restates
// JobScheduler.cpp:1353-1413 on copies of the same structs — codes, reasons, pending_jobs, materializes_array_child, and the
// DependenciesInJob the adapter leaves behind — over two cycles, the second fed with what the first wrote back.
//   test_gate_adapter [jobs] [--dump FILE]   -> needs an MI355X, exit 0 on success; FILE gets both cycles' inputs and what the adapter left,
//                                               as text, for tests/test_gpu_gate_adapter.py to hold against tests/gate_pyref.py
//   test_gate_adapter --no-gpu               -> the loud "no device" behaviour instead
//   test_gate_adapter --bench [jobs] [events] -> 1 M jobs in ascending id, 20 % with 1 - 4 dependency entries, 1 % held, 100 k events, as dense
//                                               arrays: cns_gate_pending on a handle of its own (kernel_ms and the whole call, uploads
//                                               included; one warm-up, median of 7) against the restatement over the same arrays on one
//                                               thread (median of 3), then BuildPendingQueue once over the same queue in CraneCtld's shapes.
//                                               Everything must agree; no time is asserted.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "NodeSelectionAlgo.h"
#include "adapter_test.h"
#include "../../include/crane_gpu_gate/pending_gate.h"

using namespace crane;
using Algo = GpuNodeSelectionAlgo;
using Deps = Algo::DependenciesInJob;
using GateJob = Algo::PendingGateJob;
using Event = Algo::DependencyEvent;

static const TimeSec NOW = 1000000;

// absl::Time + absl::Seconds(uint64), as include/crane_gpu_gate/pending_gate.h states it
static TimeSec time_plus_seconds(TimeSec t, uint64_t s) {
  if (t == INT64_MAX || t == INT64_MIN) return t;
  if (s >> 63) return INT64_MAX;
  return t > INT64_MAX - (int64_t)s ? INT64_MAX : t + (int64_t)s;
}

// ---- JobScheduler.cpp:1353-1413 on CraneCtld's shapes, one thread ------------------------------------------------------------------------
struct RefOut {
  std::map<job_id_t, std::string> reason;   // job->pending_reason
  std::vector<job_id_t> pending;            // pending_jobs
  std::vector<uint8_t> materializes;
};
static RefOut reference_loop(TimeSec now, std::map<job_id_t, GateJob>& pending_job_map, const std::vector<Event>& dep_events) {
  RefOut R;
  for (const Event& event : dep_events) {                                                // :1361
    auto it = pending_job_map.find(event.dependent_job_id);                              // :1362
    if (it == pending_job_map.end() || !it->second.dependencies) continue;               // :1363
    Deps& d = *it->second.dependencies;                                                  // UpdateDependency -> DependenciesInJob::update
    auto e = d.deps.find(event.dependee_job_id);                                         // CtldPublicDefs.cpp:146
    if (e == d.deps.end()) continue;                                                     // :147-150
    const TimeSec dep_ready_time = time_plus_seconds(event.event_time, e->second.second);   // :153
    d.ready_time = d.is_or ? std::min(d.ready_time, dep_ready_time) : std::max(d.ready_time, dep_ready_time);   // :154-158
    d.deps.erase(e);                                                                     // :159
  }
  static const Deps kNone;
  for (auto& [id, job] : pending_job_map) {                                              // :1377
    std::string& reason = R.reason[id];
    if (job.held) { reason = "Held"; continue; }                                         // :1380
    if (job.begin_time > now) { reason = "BeginTime"; continue; }                        // :1384
    const Deps& d = job.dependencies ? *job.dependencies : kNone;
    if (!((d.is_or || d.deps.empty()) && d.ready_time <= now)) {                         // :1388, is_met
      reason = (d.ready_time >= INT64_MAX && (!d.is_or || d.deps.empty())) ? "DependencyNeverSatisfied" : "Dependency";   // :1389-1393
      continue;
    }
    if (job.is_array_parent) {                                                           // :1397
      const Algo::ArrayParentGate& a = job.array;
      bool can = false;
      if (!a.has_meta) reason = "";                                                      // Array.cpp:687-690
      else if (!a.has_parent) reason = "";                                               // Array.cpp:237
      else if (a.materialization_complete) reason = "ArrayMaterializationComplete";      // :240
      else if (a.cancel_requested) reason = "Cancelled";                                 // :243
      else if (a.deadline_time <= now) reason = "Deadline";                              // :246
      else if (!a.has_next_task) reason = "";                                            // :249
      else if (a.running_children >= a.run_limit) reason = "ArrayTaskLimit";             // :255
      else can = true;
      if (!can) continue;                                                                // :1400-1403
      reason.clear();
      R.pending.push_back(id); R.materializes.push_back(1);                              // :1405-1407
      continue;
    }
    R.pending.push_back(id); R.materializes.push_back(0);                                // :1411
  }
  return R;
}

// ---- the generated queue -----------------------------------------------------------------------------------------------------------------
struct Queue {
  std::vector<Deps> deps;        // one per job (stable addresses: sized once)
  std::vector<GateJob> jobs;     // shuffled
};
static void make_queue(Queue& q, size_t J, uint64_t seed, bool features) {
  Rng r{seed};
  q.deps.assign(J, Deps{});
  q.jobs.clear();
  for (size_t i = 0; i < J; ++i) {
    GateJob j;
    j.job_id = (job_id_t)(100 + 2 * i);
    const uint64_t a = r();
    Deps& d = q.deps[i];
    j.held = a % 100 == 0;                                                               // 1 % held
    if ((a >> 8) % 5 == 0) {                                                             // 20 % with dependencies
      size_t n = 1 + (a >> 16) % 4;
      if (features && (a >> 20) % 50 == 0) n = 9 + (a >> 28) % 120;                      // a few lists longer than a lane walks, some longer than a wave
      d.is_or = (a >> 24) & 1;
      d.ready_time = d.is_or ? INT64_MAX : INT64_MIN;
      for (size_t k = 0; k < n; ++k) d.deps[(job_id_t)(1 + (r() % (50 * n)))] = {0, (r() % 4 == 0) ? 600u : 0u};
      j.dependencies = &d;
    } else if (features && (a >> 8) % 5 == 1) {
      j.dependencies = &d;                                                               // a struct with its defaults
    }
    if (features) {
      if ((a >> 32) % 20 == 0) j.begin_time = NOW + (int64_t)((a >> 40) % 3) - 1;
      if ((a >> 44) % 25 == 0) {
        j.is_array_parent = true;
        const uint64_t b = r();
        j.array.has_meta = b % 11 != 0; j.array.has_parent = (b >> 4) % 11 != 0; j.array.materialization_complete = (b >> 8) % 7 == 0;
        j.array.cancel_requested = (b >> 12) % 7 == 0; j.array.deadline_time = (b >> 16) % 5 == 0 ? NOW : INT64_MAX;
        j.array.has_next_task = (b >> 20) % 6 != 0; j.array.running_children = (b >> 24) % 4; j.array.run_limit = 1 + (b >> 28) % 4;
      }
    }
    q.jobs.push_back(j);
  }
  if (features)
    for (size_t i = J; i > 1; --i) std::swap(q.jobs[i - 1], q.jobs[r() % i]);            // the adapter sorts
}
// events for entries that exist (some of them twice, some at +infinity), for jobs that are not pending and for dependees nobody waits for
static std::vector<Event> make_events(const Queue& q, size_t E, uint64_t seed) {
  Rng r{seed};
  std::vector<const GateJob*> with;
  for (const GateJob& j : q.jobs) if (j.dependencies && !j.dependencies->deps.empty()) with.push_back(&j);
  std::vector<Event> ev;
  while (ev.size() < E && !with.empty()) {
    const GateJob& j = *with[r() % with.size()];
    const uint64_t a = r();
    auto it = j.dependencies->deps.begin();
    std::advance(it, (a >> 8) % j.dependencies->deps.size());
    Event e{j.job_id, it->first, NOW - 300 + (TimeSec)((a >> 16) % 900)};
    if ((a >> 32) % 50 == 0) e.event_time = INT64_MAX;                                   // a dependee that failed
    if ((a >> 40) % 20 == 0) e.dependent_job_id += 1;                                    // not pending (ids are even)
    if ((a >> 44) % 20 == 0) e.dependee_job_id += 1000000;                               // not in the list
    ev.push_back(e);
    if ((a >> 48) % 10 == 0 && ev.size() < E) { e.event_time += 500; ev.push_back(e); }  // the same pair again, later
  }
  return ev;
}

static std::map<job_id_t, GateJob> copy_map(const Queue& q, std::vector<Deps>& store) {
  store.assign(q.jobs.size(), Deps{});
  std::map<job_id_t, GateJob> m;
  for (size_t i = 0; i < q.jobs.size(); ++i) {
    GateJob j = q.jobs[i];
    if (j.dependencies) { store[i] = *j.dependencies; j.dependencies = &store[i]; }
    m[j.job_id] = j;
  }
  return m;
}

static void dump_cycle(FILE* f, int cycle, TimeSec now, const Queue& before, const std::vector<Event>& ev) {
  fprintf(f, "cycle %d now %lld\n", cycle, (long long)now);
  for (const GateJob& j : before.jobs) {
    const Deps kNone, &d = j.dependencies ? *j.dependencies : kNone;
    const auto& a = j.array;
    fprintf(f, "job %u %d %lld %d %lld %d %d %d %d %d %lld %d %llu %llu %zu", j.job_id, (int)j.held, (long long)j.begin_time, (int)d.is_or, (long long)d.ready_time,
            (int)j.is_array_parent, (int)a.has_meta, (int)a.has_parent, (int)a.materialization_complete, (int)a.cancel_requested, (long long)a.deadline_time,
            (int)a.has_next_task, (unsigned long long)a.running_children, (unsigned long long)a.run_limit, d.deps.size());
    for (const auto& [k, v] : d.deps) fprintf(f, " %u:%llu", k, (unsigned long long)v.second);
    fprintf(f, "\n");
  }
  for (const Event& e : ev) fprintf(f, "event %u %u %lld\n", e.dependent_job_id, e.dependee_job_id, (long long)e.event_time);
}
static void dump_result(FILE* f, const Queue& after, const Algo::PendingGateResult& R) {
  for (size_t i = 0; i < after.jobs.size(); ++i) {
    const GateJob& j = after.jobs[i];
    const Deps kNone, &d = j.dependencies ? *j.dependencies : kNone;
    fprintf(f, "result %u %d %lld %zu", j.job_id, (int)R.code[i], (long long)d.ready_time, d.deps.size());
    for (const auto& [k, v] : d.deps) fprintf(f, " %u", k);
    fprintf(f, "\n");
  }
  fprintf(f, "pending");
  for (size_t k = 0; k < R.pending.size(); ++k) fprintf(f, " %u:%d", after.jobs[R.pending[k]].job_id, (int)R.materializes_array_child[k]);
  fprintf(f, "\nstats %llu %llu %llu\n", (unsigned long long)R.ev_stats[0], (unsigned long long)R.ev_stats[1], (unsigned long long)R.ev_stats[2]);
}

// one cycle through the adapter and through the loop above; the queue's own structs are the adapter's, a copy is the loop's
static void one_cycle(Algo& algo, Queue& q, const std::vector<Event>& ev, TimeSec now, int cycle, FILE* dump) {
  std::vector<Deps> store;
  std::map<job_id_t, GateJob> ref_map = copy_map(q, store);
  const RefOut want = reference_loop(now, ref_map, ev);
  if (dump) dump_cycle(dump, cycle, now, q, ev);
  Algo::PendingGateResult R;
  CHECK(algo.BuildPendingQueue(now, q.jobs, ev, &R));
  if (!algo.Ok()) { printf("BuildPendingQueue: %s\n", algo.LastError().c_str()); return; }
  if (dump) dump_result(dump, q, R);
  const size_t J = q.jobs.size();
  CHECK(R.code.size() == J && R.reason.size() == J && R.pending.size() == want.pending.size() && R.kernel_ms >= 0);
  size_t bad_reason = 0, bad_state = 0, bad_pending = 0, per_code[16] = {};
  for (size_t i = 0; i < J; ++i) {
    const GateJob& j = q.jobs[i];
    bad_reason += want.reason.at(j.job_id) != R.reason[i];
    per_code[R.code[i] & 15]++;
    if (j.dependencies) {
      const Deps& w = *ref_map.at(j.job_id).dependencies;
      bad_state += !(j.dependencies->ready_time == w.ready_time && j.dependencies->deps == w.deps && j.dependencies->is_or == w.is_or);
    }
  }
  for (size_t k = 0; k < R.pending.size() && k < want.pending.size(); ++k)
    bad_pending += q.jobs[R.pending[k]].job_id != want.pending[k] || R.materializes_array_child[k] != want.materializes[k];
  CHECK(bad_reason == 0); CHECK(bad_state == 0); CHECK(bad_pending == 0);
  for (int c = 0; c < 16; ++c) CHECK(per_code[c] == R.counts[c]);
  CHECK(R.ev_stats[0] + R.ev_stats[1] + R.ev_stats[2] == ev.size());
  printf("cycle %d: %zu jobs, %zu events (%llu applied, %llu without their job, %llu without their dependency), %zu reach NodeSelect; reasons that differ %zu, "
         "DependenciesInJob that differ %zu, pending_jobs entries that differ %zu\n", cycle, J, ev.size(), (unsigned long long)R.ev_stats[0],
         (unsigned long long)R.ev_stats[1], (unsigned long long)R.ev_stats[2], R.pending.size(), bad_reason, bad_state, bad_pending);
}

static int cases(Algo& algo, size_t J, const char* dump_path) {
  FILE* dump = dump_path ? fopen(dump_path, "w") : nullptr;
  if (dump_path && !dump) { printf("cannot write %s\n", dump_path); return 1; }
  Queue q;
  make_queue(q, J, 0x6A7Eull, true);
  one_cycle(algo, q, make_events(q, J, 0xE1ull), NOW, 0, dump);
  // the next cycle: the structs as the adapter left them, ten minutes later, new events
  one_cycle(algo, q, make_events(q, J / 2, 0xE2ull), NOW + 600, 1, dump);
  // an empty map; two jobs with one id
  Algo::PendingGateResult R;
  CHECK(algo.BuildPendingQueue(NOW, {}, {Event{1, 2, 3}}, &R) && R.pending.empty() && R.code.empty() && R.ev_stats[1] == 1);
  std::vector<GateJob> twice(2);
  twice[0].job_id = twice[1].job_id = 7;
  CHECK(!algo.BuildPendingQueue(NOW, twice, {}, &R) && !algo.Ok() && algo.LastStatus() == -1 && R.code.empty());
  CHECK(algo.BuildPendingQueue(NOW, {twice[0]}, {}, &R) && algo.Ok() && R.pending.size() == 1);
  if (dump) fclose(dump);
  printf("gate cases: %d failures\n", g_fail);
  return g_fail;
}

// ---- --bench -----------------------------------------------------------------------------------------------------------------------------
static int bench(Algo& algo, size_t J, size_t E) {
  Queue q;
  make_queue(q, J, 0xB16ull, false);   // ids ascending, 1 - 4 entries
  const std::vector<Event> ev = make_events(q, E, 0xE7ull);
  // the dense arrays (outside every timed region)
  std::vector<uint32_t> job_id(J), dep_job, e_a(ev.size()), e_b(ev.size());
  std::vector<uint8_t> held(J), is_or(J);
  std::vector<int64_t> ready(J), e_t(ev.size());
  std::vector<uint64_t> off(J + 1, 0), delay;
  size_t with_deps = 0, n_held = 0;
  for (size_t i = 0; i < J; ++i) {
    const GateJob& j = q.jobs[i];
    job_id[i] = j.job_id; held[i] = j.held; n_held += j.held;
    const Deps kNone, &d = j.dependencies ? *j.dependencies : kNone;
    is_or[i] = d.is_or; ready[i] = d.ready_time;
    std::vector<std::pair<job_id_t, uint64_t>> l;
    for (const auto& [k, v] : d.deps) l.emplace_back(k, v.second);
    std::sort(l.begin(), l.end());
    for (const auto& [k, dl] : l) { dep_job.push_back(k); delay.push_back(dl); }
    off[i + 1] = dep_job.size();
    with_deps += !l.empty();
  }
  const size_t D = dep_job.size();
  for (size_t e = 0; e < ev.size(); ++e) { e_a[e] = ev[e].dependent_job_id; e_b[e] = ev[e].dependee_job_id; e_t[e] = ev[e].event_time; }
  std::unordered_map<job_id_t, uint32_t> row_of;   // the reference finds a job by id in a map that exists already
  row_of.reserve(J * 2);
  for (size_t i = 0; i < J; ++i) row_of[job_id[i]] = (uint32_t)i;

  // :1353-1413 on one thread over the dense arrays
  std::vector<uint8_t> c_code(J), c_erased(D);
  std::vector<int64_t> c_ready(J);
  std::vector<uint32_t> c_pending, c_left(J);
  std::vector<double> cpu_ms;
  for (int rep = 0; rep < 3; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    c_ready = ready;
    std::fill(c_erased.begin(), c_erased.end(), 0);
    for (size_t i = 0; i < J; ++i) c_left[i] = (uint32_t)(off[i + 1] - off[i]);
    for (size_t e = 0; e < ev.size(); ++e) {                                             // :1361
      auto it = row_of.find(e_a[e]);                                                     // :1362
      if (it == row_of.end()) continue;
      const uint32_t i = it->second;
      for (uint64_t x = off[i]; x < off[i + 1]; ++x)
        if (dep_job[x] == e_b[e] && !c_erased[x]) {                                      // CtldPublicDefs.cpp:146
          const int64_t t = time_plus_seconds(e_t[e], delay[x]);                         // :153
          c_ready[i] = is_or[i] ? std::min(c_ready[i], t) : std::max(c_ready[i], t);     // :154-158
          c_erased[x] = 1; --c_left[i];                                                  // :159
          break;
        }
    }
    c_pending.clear();
    c_pending.reserve(J);
    for (size_t i = 0; i < J; ++i) {                                                     // :1377
      uint8_t c = CNS_GATE_OK;
      if (held[i]) c = CNS_GATE_HELD;                                                    // :1380
      else if (!((is_or[i] || c_left[i] == 0) && c_ready[i] <= NOW))                     // :1388 (no begin times, no array parents in this queue)
        c = (c_ready[i] == INT64_MAX && (!is_or[i] || c_left[i] == 0)) ? CNS_GATE_DEPENDENCY_NEVER : CNS_GATE_DEPENDENCY;
      c_code[i] = c;
      if (c == CNS_GATE_OK) c_pending.push_back((uint32_t)i);                            // :1411
    }
    cpu_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }

  // the call on a handle of its own
  cns_config cfg{};
  cfg.abi_version = CNS_ABI_VERSION;
  cns_handle* h = nullptr;
  if (cns_create(&cfg, &h) != 0) { printf("cns_create: %s\n", cns_last_error(nullptr)); return 1; }
  cns_gate_jobs gj{};
  gj.num_jobs = J; gj.job_id = job_id.data(); gj.held = held.data(); gj.dep_is_or = is_or.data(); gj.dep_ready_sec = ready.data();
  gj.dep_offsets = off.data(); gj.dep_job = dep_job.data(); gj.dep_delay_sec = delay.data();
  cns_gate_events ge{ev.size(), e_a.data(), e_b.data(), e_t.data()};
  std::vector<uint8_t> g_code(J), g_erased(D + 1);
  std::vector<uint32_t> g_pending(J);
  std::vector<int64_t> g_ready(J);
  uint64_t n_pending = 0, counts[16], stats[3];
  cns_gate_out go{g_code.data(), g_pending.data(), &n_pending, g_ready.data(), g_erased.data(), counts, stats};
  std::vector<double> kms, call;
  for (int rep = 0; rep < 8; ++rep) {
    double ms = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int st = cns_gate_pending(h, NOW, &gj, &ge, &go, &ms);
    const auto t1 = std::chrono::steady_clock::now();
    if (st != 0) { printf("cns_gate_pending: %s\n", cns_last_error(h)); cns_destroy(h); return 1; }
    if (rep) { kms.push_back(ms); call.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
  }
  cns_destroy(h);
  size_t differ = 0;
  for (size_t i = 0; i < J; ++i) differ += g_code[i] != c_code[i] || g_ready[i] != c_ready[i];
  for (size_t x = 0; x < D; ++x) differ += g_erased[x] != c_erased[x];
  differ += n_pending != c_pending.size();
  for (size_t k = 0; k < c_pending.size() && k < n_pending; ++k) differ += g_pending[k] != c_pending[k];

  // ... and once through the adapter, in CraneCtld's shapes
  Algo::PendingGateResult R;
  const auto a0 = std::chrono::steady_clock::now();
  const bool ok = algo.BuildPendingQueue(NOW, q.jobs, ev, &R);
  const double adapter_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a0).count();
  if (!ok) { printf("BuildPendingQueue: %s\n", algo.LastError().c_str()); return 1; }
  size_t adapter_differ = R.pending.size() != c_pending.size();
  for (size_t i = 0; i < J; ++i) {
    adapter_differ += R.code[i] != c_code[i];
    if (q.jobs[i].dependencies) adapter_differ += q.jobs[i].dependencies->ready_time != c_ready[i] || q.jobs[i].dependencies->deps.size() != c_left[i];
  }
  for (size_t k = 0; k < R.pending.size() && k < c_pending.size(); ++k) adapter_differ += R.pending[k] != c_pending[k];
  printf("gate bench: %zu jobs (%zu with dependencies, %zu entries, %zu held), %zu events (%llu applied, %llu without their job, %llu without their dependency), "
         "%llu reach NodeSelect: kernel_ms %.3f  call_ms %.3f  cpu_loop_ms %.3f (one thread, dense arrays, the id lookup in a hash map built outside the "
         "timed region; median of %zu / %zu / %zu)  adapter_ms %.3f (one call, CraneCtld's shapes: sort, pack, call, write-back)  "
         "results that differ from the cpu loop %zu, through the adapter %zu\n",
         J, with_deps, D, n_held, ev.size(), (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2],
         (unsigned long long)n_pending, median(kms), median(call), median(cpu_ms), kms.size(), call.size(), cpu_ms.size(), adapter_ms, differ, adapter_differ);
  return differ || adapter_differ ? 1 : 0;
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
  Algo algo(0);
  if (no_gpu) {
    if (algo.Ok()) { printf("a device is present: nothing to check\n"); return 0; }
    Algo::PendingGateResult R;
    CHECK(!algo.BuildPendingQueue(NOW, {}, {}, &R) && R.code.empty() && !algo.Ok() && algo.LastStatus() != 0);
    printf("no device: BuildPendingQueue refuses with status %d (%s)\n", algo.LastStatus(), algo.LastError().c_str());
    return g_fail ? 1 : 0;
  }
  if (!algo.Ok()) { printf("no usable device: %s\n", algo.LastError().c_str()); return 2; }
  if (argc > 1 && !strcmp(argv[1], "--bench"))
    return bench(algo, argc > 2 ? (size_t)atoll(argv[2]) : (size_t)1000000, argc > 3 ? (size_t)atoll(argv[3]) : (size_t)100000);
  size_t J = 2000;
  const char* dump = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else J = (size_t)atoll(argv[i]);
  }
  return cases(algo, J, dump) ? 1 : 0;
}
