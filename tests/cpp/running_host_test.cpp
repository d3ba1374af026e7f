// cranesched_amd/csrc/running_check_host.inc (the input rules of cns_running_seed / cns_running_advance) compiled with g++ and driven
// over hand cases: valid calls, then every rule of include/crane_gpu_running/running.h broken in turn.  Prints
// "<case>: <status> <message>" per case, so that tests/test_running_host.py can hold every refusal to its message; built once plain and
// once with -fsanitize=address,undefined: every array below is exactly as long as the header says, so a pass that reads past one is caught.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../cranesched_amd/csrc/running_check_host.inc"

namespace {

struct Seed {
  std::vector<int64_t> end{100, 200, 300};
  std::vector<uint32_t> off{0, 2, 2, 3}, node{0, 4, 2}, ids{7, 3, 9};
  std::vector<int64_t> cpu{256, 256, 512};
  std::vector<uint64_t> mem{1, 1, 1}, lo{1, 1, 3};
  cns_running_soa rn{};
  const uint32_t* job_ids = nullptr;
  uint32_t N = 5;
  void bind() {
    rn.num_jobs = (uint32_t)end.size(); rn.num_allocs = (uint32_t)node.size();
    rn.end_sec = end.data(); rn.alloc_offsets = off.data(); rn.alloc_node = node.data(); rn.alloc_cpu_raw = cpu.data(); rn.alloc_mem = mem.data();
    rn.alloc_core_lo = lo.data();
    job_ids = ids.data();
  }
};

struct Step {
  std::vector<uint32_t> retire{9, 3, 12}, job_id{20, 21, 22, 23};
  std::vector<uint8_t> found = std::vector<uint8_t>(3), admit{1, 0, 1, 1};
  uint64_t nret = 0, nadm = 0;
  cns_running_step in{};
  cns_running_step_out out{};
  cns_running::Facts F;
  void bind() {
    in.num_retire = retire.size(); in.retire_ids = retire.data();
    in.num_jobs = job_id.size(); in.now_sec = 1000; in.job_id = job_id.data(); in.admit = admit.data();
    out.found = found.data(); out.num_retired = &nret; out.num_admitted = &nadm;
    F.have_ledger = true; F.have_cycle = true; F.cycle_jobs = 4; F.cycle_now = 1000; F.ledger_jobs = 3; F.ledger_allocs = 3; F.cycle_places = 6;
  }
};

int g_fail = 0;

void seed(const char* name, const std::function<void(Seed&)>& edit, bool null_set = false) {
  Seed c;
  c.bind();
  edit(c);
  uint64_t R = 99, A = 99;
  const cns_running::Verdict v = cns_running::check_seed(null_set ? nullptr : &c.rn, c.job_ids, c.N, &R, &A);
  printf("%s: %d %s", name, v.code, v.msg.c_str());
  if (!v) printf("R=%llu A=%llu", (unsigned long long)R, (unsigned long long)A);
  printf("\n");
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

void step(const char* name, const std::function<void(Step&)>& edit, bool null_out = false) {
  Step c;
  c.bind();
  edit(c);
  std::vector<uint32_t> sorted, order;
  const cns_running::Verdict v = cns_running::check_step(c.F, &c.in, null_out ? nullptr : &c.out, &sorted, &order);
  printf("%s: %d %s", name, v.code, v.msg.c_str());
  if (!v) {
    printf("sorted=");
    for (uint32_t x : sorted) printf("%u,", x);
    printf(" order=");
    for (uint32_t x : order) printf("%u,", x);
  }
  printf("\n");
  if ((v.code != 0) != !v.msg.empty()) ++g_fail;
}

void pairs(const char* name, uint64_t allocs, uint64_t fan) {
  const cns_running::Verdict v = cns_running::check_pairs(allocs, fan);
  printf("%s: %d %s\n", name, v.code, v.msg.c_str());
}

}  // namespace

int main() {
  seed("seed_valid", [](Seed&) {});
  seed("seed_null_set", [](Seed&) {}, true);
  seed("seed_no_jobs", [](Seed& c) { cns_running_soa e{}; c.rn = e; c.job_ids = nullptr; });
  seed("seed_no_end", [](Seed& c) { c.rn.end_sec = nullptr; });
  seed("seed_no_offsets", [](Seed& c) { c.rn.alloc_offsets = nullptr; });
  seed("seed_no_node", [](Seed& c) { c.rn.alloc_node = nullptr; });
  seed("seed_no_cpu", [](Seed& c) { c.rn.alloc_cpu_raw = nullptr; });
  seed("seed_no_mem", [](Seed& c) { c.rn.alloc_mem = nullptr; });
  seed("seed_no_core_lo", [](Seed& c) { c.rn.alloc_core_lo = nullptr; });
  seed("seed_no_ids", [](Seed& c) { c.job_ids = nullptr; });
  seed("seed_num_allocs", [](Seed& c) { c.rn.num_allocs = 2; });
  seed("seed_offsets_first", [](Seed& c) { c.off[0] = 1; });
  seed("seed_offsets_decrease", [](Seed& c) { c.off = {0, 2, 1, 3}; c.rn.alloc_offsets = c.off.data(); });
  seed("seed_node_outside", [](Seed& c) { c.node[1] = 5; });
  seed("seed_node_at_the_border", [](Seed& c) { c.N = 5; c.node[1] = 4; });
  seed("seed_id_twice", [](Seed& c) { c.ids[2] = 7; });
  seed("seed_too_many_jobs", [](Seed& c) { c.rn.num_jobs = 0xFFFFFE01u; });
  seed("seed_too_many_allocs", [](Seed& c) { c.rn.num_allocs = 0xFFFFFF01u; });

  step("step_valid", [](Step&) {});
  step("step_empty", [](Step& c) { cns_running_step e{}; c.in = e; }, true);
  step("step_retire_only", [](Step& c) { c.in.num_jobs = 0; c.F.have_cycle = false; });
  step("step_admit_all", [](Step& c) { c.in.admit = nullptr; c.in.num_retire = 0; c.in.retire_ids = nullptr; c.out.found = nullptr; });
  step("step_no_ledger", [](Step& c) { c.F.have_ledger = false; });
  step("step_no_retire_ids", [](Step& c) { c.in.retire_ids = nullptr; });
  step("step_no_found", [](Step& c) { c.out.found = nullptr; });
  step("step_no_out", [](Step&) {}, true);
  step("step_retire_twice", [](Step& c) { c.retire[2] = 9; });
  step("step_no_cycle", [](Step& c) { c.F.have_cycle = false; });
  step("step_preempt_cycle", [](Step& c) { c.F.preempt_cycle = true; });
  step("step_other_queue", [](Step& c) { c.F.cycle_jobs = 5; });
  step("step_other_now", [](Step& c) { c.in.now_sec = 999; });
  step("step_no_job_id", [](Step& c) { c.in.job_id = nullptr; });
  step("step_too_many_retire", [](Step& c) { c.in.num_retire = 0xFFFFFF01ull; });
  step("step_too_many_jobs", [](Step& c) { c.F.ledger_jobs = 0xFFFFFE00ull - 3; });
  step("step_jobs_at_the_limit", [](Step& c) { c.F.ledger_jobs = 0xFFFFFE00ull - 4; });
  step("step_too_many_allocs", [](Step& c) { c.F.ledger_allocs = 0xFFFFFF00ull - 5; });

  pairs("pairs_fit", 0xFFFFFF00ull / 3, 3);
  pairs("pairs_no_slot_at_all", 0xFFFFFF00ull, 0);
  pairs("pairs_too_many", 0xFFFFFF00ull / 3 + 1, 3);
  return g_fail ? 1 : 0;
}
