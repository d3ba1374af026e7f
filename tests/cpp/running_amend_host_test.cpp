// cranesched_amd/csrc/running_amend_check_host.inc (the input rules of cns_running_amend_ends) compiled with g++ and driven over hand
// cases: valid calls, then every rule of include/crane_gpu_amend/running_amend.h broken in turn.  Prints "<case>: <status> <message>"
// per case, so that tests/test_running_amend_host.py can hold every refusal to its message; built once plain and once with
// -fsanitize=address,undefined: every array below is exactly as long as the header says, so a pass that reads past one is caught.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../cranesched_amd/csrc/running_amend_check_host.inc"

namespace {

struct Amend {
  std::vector<uint32_t> ids{9, 4294967295u, 0, 12};
  std::vector<int64_t> ends{900, -5, INT64_MAX, INT64_MIN};
  std::vector<uint8_t> found = std::vector<uint8_t>(4);
  uint64_t n = 0;
  cns_running_amend in{};
  cns_running_amend_out out{};
  bool have_ledger = true, null_out = false;
  void bind() {
    in.num_amend = ids.size(); in.job_ids = ids.data(); in.end_sec = ends.data();
    out.found = found.data(); out.num_amended = &n;
  }
};

void amend(const char* name, const std::function<void(Amend&)>& edit) {
  Amend c;
  c.bind();
  edit(c);
  std::vector<uint32_t> sorted, order;
  std::vector<int64_t> sends;
  const auto v = cns_running::check_amend(c.have_ledger, &c.in, c.null_out ? nullptr : &c.out, &sorted, &sends, &order);
  std::string msg = v.msg;
  if (!v) {
    msg = "sorted=";
    for (uint32_t x : sorted) msg += std::to_string(x) + ",";
    msg += " ends=";
    for (int64_t x : sends) msg += std::to_string(x) + ",";
    msg += " order=";
    for (uint32_t x : order) msg += std::to_string(x) + ",";
  }
  printf("%s: %d %s\n", name, v.code, msg.c_str());
}

}  // namespace

int main() {
  amend("valid", [](Amend&) {});
  amend("one", [](Amend& c) { c.ids = {5}; c.ends = {77}; c.found.resize(1); c.bind(); });
  amend("descending", [](Amend& c) { c.ids = {30, 20, 10}; c.ends = {3, 2, 1}; c.found.resize(3); c.bind(); });
  amend("empty", [](Amend& c) { c.in.num_amend = 0; c.in.job_ids = nullptr; c.in.end_sec = nullptr; c.null_out = true; });
  amend("no_count_wanted", [](Amend& c) { c.out.num_amended = nullptr; });
  amend("no_ledger", [](Amend& c) { c.have_ledger = false; });
  amend("no_ledger_and_empty", [](Amend& c) { c.have_ledger = false; c.in.num_amend = 0; });
  amend("no_ids", [](Amend& c) { c.in.job_ids = nullptr; });
  amend("no_ends", [](Amend& c) { c.in.end_sec = nullptr; });
  amend("no_found", [](Amend& c) { c.out.found = nullptr; });
  amend("no_out", [](Amend& c) { c.null_out = true; });
  amend("id_twice", [](Amend& c) { c.ids = {9, 3, 12, 3}; c.bind(); });
  amend("id_zero_twice", [](Amend& c) { c.ids = {0, 3, 12, 0}; c.bind(); });
  // the limit: 2^32 - 255 amendments are refused before any array is read; 2^32 - 256 pass that rule (and are stopped by the next one here)
  amend("too_many", [](Amend& c) { c.in.num_amend = 0xFFFFFF01ull; c.in.job_ids = nullptr; c.in.end_sec = nullptr; });
  amend("at_the_limit", [](Amend& c) { c.in.num_amend = 0xFFFFFF00ull; c.in.job_ids = nullptr; c.in.end_sec = nullptr; });
  return 0;
}
