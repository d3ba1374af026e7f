// cranesched_amd/csrc/gate_check_host.inc (the input rules of cns_gate_pending) compiled with g++ and driven over hand cases: one valid
// call, then every rule of include/crane_gpu_gate/pending_gate.h broken in turn.  Prints "<case>: <status> <message>" per case, so that
// tests/test_gate_host.py can hold every refusal to its message; built once plain and once with -fsanitize=address,undefined: every
// array below is exactly as long as the header says, so a pass that reads past one is caught.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../cranesched_amd/csrc/gate_check_host.inc"

namespace {

struct Case {
  std::vector<uint32_t> job_id{10, 20, 30, 40};
  std::vector<uint8_t> held{0, 1, 0, 0}, is_or{0, 1, 0, 0}, ap{0, 0, 1, 0}, ap_flags{0, 0, 31, 3};
  std::vector<int64_t> begin{0, 0, 5, INT64_MAX}, ready{INT64_MIN, INT64_MAX, 0, 0}, ap_dead{0, 0, 9, 0};
  std::vector<uint64_t> off{0, 2, 2, 5, 5}, delay{0, 1, 2, 3, ~0ull}, ap_run{0, 0, 1, 0}, ap_lim{0, 0, 2, 0};
  std::vector<uint32_t> dep{7, 9, 1, 2, 0xFFFFFFFFu};
  std::vector<uint32_t> e_dependent{20, 30}, e_dependee{7, 2};
  std::vector<int64_t> e_sec{INT64_MIN, 100};
  std::vector<uint8_t> code = std::vector<uint8_t>(4);
  std::vector<uint32_t> pending = std::vector<uint32_t>(4);
  uint64_t num_pending = 0;
  cns_gate_jobs jobs{};
  cns_gate_events ev{};
  cns_gate_out out{};
  void bind() {
    jobs.num_jobs = job_id.size();
    jobs.job_id = job_id.data(); jobs.held = held.data(); jobs.begin_sec = begin.data(); jobs.dep_is_or = is_or.data(); jobs.dep_ready_sec = ready.data();
    jobs.dep_offsets = off.data(); jobs.dep_job = dep.data(); jobs.dep_delay_sec = delay.data();
    jobs.array_parent = ap.data(); jobs.ap_flags = ap_flags.data(); jobs.ap_deadline_sec = ap_dead.data(); jobs.ap_running = ap_run.data(); jobs.ap_run_limit = ap_lim.data();
    ev.num_events = e_sec.size();
    ev.dependent_job_id = e_dependent.data(); ev.dependee_job_id = e_dependee.data(); ev.event_sec = e_sec.data();
    out.code = code.data(); out.pending = pending.data(); out.num_pending = &num_pending;
  }
};

int g_fail = 0;

void run(const char* name, const std::function<void(Case&)>& edit, bool with_events = true) {
  Case c;
  c.bind();
  edit(c);
  cns_gate::Sizes s;
  const cns_gate::Verdict v = cns_gate::check(&c.jobs, with_events ? &c.ev : nullptr, &c.out, &s);
  printf("%s: %d %s", name, v.code, v.msg.c_str());
  if (!v) printf("J=%llu D=%llu E=%llu deps=%d array=%d", (unsigned long long)s.J, (unsigned long long)s.D, (unsigned long long)s.E, (int)s.has_deps, (int)s.has_array);
  printf("\n");
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

}  // namespace

int main() {
  run("valid", [](Case&) {});
  run("valid_no_events", [](Case&) {}, false);
  run("valid_bare", [](Case& c) { cns_gate_jobs j{}; j.num_jobs = 4; j.job_id = c.jobs.job_id; c.jobs = j; }, false);
  run("valid_empty", [](Case& c) { cns_gate_jobs j{}; c.jobs = j; c.out.code = nullptr; c.out.pending = nullptr; });
  run("valid_offsets_without_entries", [](Case& c) { c.off = {0, 0, 0, 0, 0}; c.jobs.dep_offsets = c.off.data(); c.jobs.dep_job = nullptr; c.jobs.dep_delay_sec = nullptr; });
  run("no_job_id", [](Case& c) { c.jobs.job_id = nullptr; });
  run("no_code", [](Case& c) { c.out.code = nullptr; });
  run("no_pending", [](Case& c) { c.out.pending = nullptr; });
  run("no_num_pending", [](Case& c) { c.out.num_pending = nullptr; });
  run("no_event_sec", [](Case& c) { c.ev.event_sec = nullptr; });
  run("no_event_dependee", [](Case& c) { c.ev.dependee_job_id = nullptr; });
  run("is_or_without_ready", [](Case& c) { c.jobs.dep_ready_sec = nullptr; });
  run("ready_without_is_or", [](Case& c) { c.jobs.dep_is_or = nullptr; });
  run("entries_without_dep_job", [](Case& c) { c.jobs.dep_job = nullptr; });
  run("entries_without_delay", [](Case& c) { c.jobs.dep_delay_sec = nullptr; });
  run("entries_without_is_or", [](Case& c) { c.jobs.dep_is_or = nullptr; c.jobs.dep_ready_sec = nullptr; });
  run("ap_without_flags", [](Case& c) { c.jobs.ap_flags = nullptr; });
  run("ap_without_deadline", [](Case& c) { c.jobs.ap_deadline_sec = nullptr; });
  run("ap_without_running", [](Case& c) { c.jobs.ap_running = nullptr; });
  run("ap_without_limit", [](Case& c) { c.jobs.ap_run_limit = nullptr; });
  run("job_id_equal", [](Case& c) { c.job_id[2] = 20; });
  run("job_id_descends", [](Case& c) { c.job_id[3] = 5; });
  run("offsets_first", [](Case& c) { c.off[0] = 1; });
  run("offsets_decrease", [](Case& c) { c.off[2] = 1; });
  run("list_equal", [](Case& c) { c.dep[1] = 7; });
  run("list_descends", [](Case& c) { c.dep[3] = 0; });
  run("list_border_is_free", [](Case& c) { c.dep[2] = 9; c.dep[3] = 10; });   // the last of one list and the first of the next may be equal
  run("flags_outside", [](Case& c) { c.ap_flags[0] = 32; });
  run("too_many_jobs", [](Case& c) { c.jobs.num_jobs = 0xFFFFFE01ull; });
  run("jobs_at_the_limit_reach_the_arrays", [](Case& c) { c.jobs.num_jobs = 0xFFFFFE00ull; c.jobs.job_id = nullptr; });
  run("too_many_events", [](Case& c) { c.ev.num_events = 0xFFFFFF01ull; });
  run("too_many_entries", [](Case& c) { c.off[3] = c.off[4] = 0xFFFFFF01ull; });
  return g_fail ? 1 : 0;
}
