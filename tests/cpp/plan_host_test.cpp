// The launch plan of a cycle (cranesched_amd/csrc/plan_host.inc) held, row by row, to the rules the engine followed before the plan was
// a file of its own: which k_wide build serves how many partitions, when a group goes to k_mem / k_giant, what a retry may use, what
// kernel_pin means under each value of CNS_SELECT_KERNEL, and the bytes of cns_debug_last_kernel.  The build's figures are the shipped
// ones, written out as literals (engine.hip static_asserts that its constants equal them).  No GPU, no HIP.
#include <cstdio>
#include <string>
#include <vector>

#include "../../cranesched_amd/csrc/plan_host.inc"

using namespace cns_plan;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_failed; } } while (0)

static Facts shipped() {
  Facts f;
  const u32 waves[4] = {64, 32, 16, 8}, group[4] = {17, 9, 5, 3}, max_parts[4] = {8, 24, 48, 80}, lanes[4] = {4096, 2048, 1024, 512}, aux[4] = {3, 1, 1, 1};
  for (int i = 0; i < 4; ++i) {
    WideBuild& b = f.wide[i];
    b.waves = waves[i]; b.group = group[i]; b.max_parts = max_parts[i]; b.aux_max = aux[i]; b.last_in_lds_rows = 4;
    b.tiles.lanes = lanes[i]; b.tiles.block = 512;
    b.tiles.widths = {1, 2, 4, 8};
  }
  f.wide[0].tiles.widths.push_back(16);
  f.wide[0].window_widths = {1, 2};
  f.select.lanes = 448; f.select.block = 512; f.select.widths = {1, 3, 10, 19, 28, 37};
  f.pipe.lanes = 512; f.pipe.block = 768; f.pipe.widths = {1, 4, 8, 16};
  f.mem_slots = 143360; f.giant_mem_slots = 544768; f.giant_helpers_max = 64; f.giant_helper_budget = 64;
  return f;
}
static Inputs cluster(u32 parts, u32 slots, u32 members = 1) {   // `parts` busy partitions of `slots` slots on a whole MI355X
  Inputs in;
  in.parts.assign(parts, Part{10, slots, members, false});
  in.num_cus = 256;
  return in;
}
static std::string names(const Launch& L) {
  std::string s;
  for (const Candidate& c : L.cands) s += (s.empty() ? "" : " | ") + candidate_name(c);
  return s;
}
static bool has(const CyclePlan& P, Family f) {
  for (const Launch* L : {&P.a, &P.b, &P.c}) for (const Candidate& c : L->cands) if (c.family == f) return true;
  return false;
}

// `plan_host_test serial <n>`: what CNS_SELECT_KERNEL=giant launches for 1 .. n busy partitions of 64 slots, one line each:
// "<busy> <first candidate's kernel> <its helper workgroups per partition>" (tests/test_serial_seams.py reads the rule from here).
static int serial_table(const Facts& F, u32 n) {
  printf("helpers_min %u\n", kGiantMinHelpers);
  for (u32 busy = 1; busy <= n; ++busy) {
    Inputs in = cluster(busy, 64);
    in.sw = Switch::Giant;
    const CyclePlan P = plan_cycle(F, in);
    if (!P.a.parts.empty() || !P.b.parts.empty() || P.c.cands.empty()) return 1;
    const Candidate& c = P.c.cands[0];
    printf("%u %s %u %d\n", busy, kernel_of(c).c_str(), c.family == Family::Giant ? c.extra : 0u, (int)c.giant_masks);
  }
  return 0;
}

int main(int argc, char** argv) {
  const Facts F = shipped();
  if (argc == 3 && std::string(argv[1]) == "serial") return serial_table(F, (u32)std::stoul(argv[2]));
  CHECK(kGiantMinHelpers == 4);
  CHECK(F.wide[0].tiles.slots() == 65536 && F.wide[1].tiles.slots() == 16384 && F.wide[2].tiles.slots() == 8192 && F.wide[3].tiles.slots() == 4096);
  CHECK(F.select.slots() == 37 * 448 && F.pipe.slots() == 8192);

  // ---- the switch
  const struct { const char* word; Switch sw; } words[] = {{nullptr, Switch::Unset}, {"legacy", Switch::Legacy}, {"pipe", Switch::Pipe}, {"wide", Switch::Wide}, {"wide32", Switch::Wide32},
                                                           {"wide16", Switch::Wide16}, {"wide8", Switch::Wide8}, {"giant", Switch::Giant}, {"mem", Switch::Mem}, {"widee", Switch::Other},
                                                           {"", Switch::Other}, {"Legacy", Switch::Other}};
  for (const auto& w : words) CHECK(parse_kernel_switch(w.word) == w.sw);

  // ---- P plain partitions of 64 nodes on 256 CUs: the widest build that fits (tests/test_gpu_wide_narrow.py, and the boundaries at 8 / 9)
  const struct { u32 parts, waves, grid; } rows[] = {{8, 64, 8 * 18}, {9, 32, 16 * 10}, {24, 32, 24 * 10}, {25, 16, 32 * 6}, {48, 16, 48 * 5}, {49, 8, 56 * 4}, {80, 8, 80 * 3}, {81, 0, 0}};
  for (const auto& r : rows) {
    const CyclePlan P = plan_cycle(F, cluster(r.parts, 64));
    CHECK(!P.split && P.identity && P.single() == &P.a && P.b.cands.empty() && P.c.cands.empty() && P.a.other_blocks == 0 && !P.a.second_stream);
    const std::vector<Candidate>& c = P.a.cands;
    CHECK(c.size() == (r.waves ? 3u : 2u));
    if (r.waves) CHECK(c[0].family == Family::Wide && c[0].waves == r.waves && c[0].width == 1 && c[0].grid == r.grid && c[0].block == 512 && c[0].waits);
    const size_t n = c.size();
    CHECK(c[n - 2].family == Family::Pipe && c[n - 2].width == 1 && c[n - 2].grid == r.parts && c[n - 2].block == 768 && !c[n - 2].waits);
    CHECK(c[n - 1].family == Family::Select && c[n - 1].width == 1 && c[n - 1].grid == r.parts && c[n - 1].block == 512 && !c[n - 1].waits);
    CHECK(!has(P, Family::Mem) && !has(P, Family::Giant));
  }
  // ---- no proof of co-residency without a CU per workgroup (unknown count: 0; a device smaller than the narrowest build's grid of 24)
  for (u32 cus : {0u, 16u}) { Inputs in = cluster(8, 64); in.num_cus = cus; CHECK(names(plan_cycle(F, in).a) == "k_pipe<1> | k_select<1>"); }
  { Inputs in = cluster(8, 64); in.num_cus = 100; CHECK(plan_cycle(F, in).a.cands[0].waves == 32); }   // 136 > 100 >= 72
  // ---- the other launches' workgroups count: 8 x 17 + 120 = 256 still fits (without the extra home), + 121 does not
  for (u32 other : {120u, 121u}) {
    Launch L;
    for (u32 p = 0; p < 8; ++p) L.parts.push_back(p);
    L.max_np = 64; L.other_blocks = other;
    plan_launch(F, cluster(8, 64), true, L);
    CHECK(L.cands[0].family == Family::Wide && L.cands[0].waves == (other == 120 ? 64u : 32u) && L.cands[0].extra == (other == 120 ? 0u : 1u));
  }
  // ---- cns_config::kernel_pin (tests/test_gpu_fullrun.py: test_kernel_pin_of_the_config), and any set switch against it
  const char* first_of_pin[3] = {"k_wide<1> x64", "k_select<1>", "k_pipe<1>"};
  for (u32 pin = 0; pin < 3; ++pin) {
    Inputs in = cluster(4, 64);
    in.kernel_pin = pin;
    CHECK(candidate_name(plan_cycle(F, in).a.cands[0]) == first_of_pin[pin]);
    CHECK(pin != 1 || plan_cycle(F, in).a.cands.size() == 1);
    for (Switch sw : {Switch::Legacy, Switch::Pipe, Switch::Wide, Switch::Wide32, Switch::Wide16, Switch::Wide8, Switch::Giant, Switch::Mem, Switch::Other}) {
      Inputs free = cluster(4, 64);
      free.sw = in.sw = sw;
      const CyclePlan A = plan_cycle(F, in), B = plan_cycle(F, free);
      CHECK(names(A.a) == names(B.a) && names(A.b) == names(B.b) && names(A.c) == names(B.c));
    }
    in.sw = Switch::Other;   // an unknown word: the default choice, the pin ignored
    CHECK(names(plan_cycle(F, in).a) == "k_wide<1> x64 | k_pipe<1> | k_select<1>");
  }
  // ---- each value of the switch
  {
    Inputs in = cluster(8, 64);
    in.sw = Switch::Legacy; CHECK(names(plan_cycle(F, in).a) == "k_select<1>");
    in.sw = Switch::Pipe; CHECK(names(plan_cycle(F, in).a) == "k_pipe<1> | k_select<1>");
    in.sw = Switch::Wide; CHECK(names(plan_cycle(F, in).a) == "k_wide<1> x64 | k_pipe<1> | k_select<1>");
    in.sw = Switch::Wide32; CHECK(plan_cycle(F, in).a.cands[0].waves == 32);
    in.sw = Switch::Wide16; CHECK(names(plan_cycle(F, in).a) == "k_wide<1> x16 | k_pipe<1> | k_select<1>");
    in.sw = Switch::Wide8; CHECK(plan_cycle(F, in).a.cands[0].waves == 8);
    in.sw = Switch::Giant;
    in.pre_active = true; in.parts[5].may_preempt = true;   // (every partition WITHOUT preemption)
    const CyclePlan G = plan_cycle(F, in);
    CHECK(G.c.parts.size() == 7 && G.a.parts.empty() && G.b.parts == std::vector<u32>{5} && G.c.second_stream && G.c.other_blocks == 0);
    CHECK(G.c.cands.size() == 2 && G.c.cands[0].family == Family::Giant && G.c.cands[0].extra == 9 && G.c.cands[0].grid == 70 && G.c.cands[0].waits && G.c.cands[1].family == Family::Mem);
    CHECK(G.b.other_blocks == 70 && names(G.b) == "k_select<1>");
    Inputs big = cluster(1, 65537);
    big.sw = Switch::Mem;
    const CyclePlan M = plan_cycle(F, big);
    CHECK(M.c.parts.size() == 1 && names(M.c) == "k_mem (k_wide<1> home workgroup, sequential protocol over the HBM arrays)" && M.c.cands[0].grid == 24 && M.c.cands[0].holds == 1);
  }
  // ---- tile widths and names (tests/test_gpu_fullsize.py: 32 768 nodes on k_wide<8> x64)
  const struct { u32 np, window; const char* name; } tiles[] = {{65536, 0, "k_wide<16> x64"}, {32768, 0, "k_wide<8> x64"}, {4097, 0, "k_wide<2> x64"}, {8192, 32, "k_wide<2> windows x64"},
                                                                {4096, 2, "k_wide<1> windows x64"}, {4096, 1, "k_wide<1> x64"}, {8193, 32, "k_wide<4> x64"}};
  for (const auto& t : tiles) { Inputs in = cluster(1, t.np); in.wide_window = t.window; CHECK(candidate_name(plan_cycle(F, in).a.cands[0]) == t.name); }
  { Inputs in = cluster(9, 4096); in.wide_window = 32; CHECK(candidate_name(plan_cycle(F, in).a.cands[0]) == "k_wide<2> x32"); }   // (the 64-wave build alone has windows)
  CHECK(names(plan_cycle(F, cluster(1, 8193)).a) == "k_wide<4> x64 | k_select<19>" && names(plan_cycle(F, cluster(1, 2049)).a) == "k_wide<1> x64 | k_pipe<8> | k_select<10>");
  { Inputs in = cluster(1, 16577); in.sw = Switch::Legacy; const CyclePlan P = plan_cycle(F, in); CHECK(P.a.cands.empty() && std::string(P.a.exhausted) == "partition too large for the widest register tile"); }
  // ---- extra home workgroups of the 64-wave build (3 at most)
  const struct { u32 np, cus; int64_t aux; u32 extra; } homes[] = {{64, 256, -1, 1}, {16384, 256, -1, 1}, {16385, 256, -1, 0}, {16385, 256, 3, 0}, {64, 256, 0, 0}, {64, 256, 3, 3},
                                                                   {64, 256, 9, 3}, {64, 150, 3, 1}, {64, 152, 3, 2}, {64, 136, -1, 0}};
  for (const auto& r : homes) {
    Inputs in = cluster(8, r.np);
    in.num_cus = r.cus; in.aux_override = r.aux;
    const Candidate c = plan_cycle(F, in).a.cands[0];
    CHECK(c.waves == 64 && c.extra == r.extra && c.grid == 8 * (17 + r.extra) && (17 + r.extra) <= 32 && c.grid <= r.cus);
  }
  { Inputs in = cluster(48, 64); in.aux_override = 1; CHECK(plan_cycle(F, in).a.cands[0].extra == 0); }   // 6 partitions per XCD x 6 workgroups > 32
  // ---- k_giant's helpers: 64 per launch, fewer than 4 per partition is no k_giant
  const struct { u32 parts, helpers; } helpers[] = {{1, 64}, {3, 21}, {16, 4}, {17, 0}};
  for (const auto& r : helpers) {
    const CyclePlan P = plan_cycle(F, cluster(r.parts, 70000));
    CHECK(P.a.parts.empty() && P.b.parts.empty() && P.c.parts.size() == r.parts && P.c.max_np == 70000 && P.c.cands.back().family == Family::Mem && !P.c.cands.back().giant_masks);
    CHECK(P.c.cands.size() == (r.helpers ? 2u : 1u));
    if (r.helpers) CHECK(P.c.cands[0].family == Family::Giant && P.c.cands[0].extra == r.helpers && P.c.cands[0].grid == r.parts * (1 + r.helpers) && P.c.cands[0].holds == P.c.cands[0].grid);
  }
  { Inputs in = cluster(1, 70000); in.num_cus = 0; CHECK(!has(plan_cycle(F, in), Family::Giant)); }
  // ---- shared groups and wide shapes
  {
    const CyclePlan B = plan_cycle(F, cluster(2, 37 * 448, 2));
    CHECK(B.single() == &B.b && B.identity && !B.b.second_stream && names(B.b) == "k_select<37>");
    for (u32 np : {37u * 448u + 1u, 143360u}) {
      const CyclePlan C = plan_cycle(F, cluster(2, np, 2));
      CHECK(C.b.parts.empty() && C.c.parts.size() == 2 && names(C.c) == "k_mem (k_wide<1> home workgroup, sequential protocol over the HBM arrays)");
    }
    const CyclePlan G = plan_cycle(F, cluster(1, 143361, 2));
    CHECK(G.c.cands.size() == 2 && G.c.cands[0].family == Family::Giant && G.c.cands[1].family == Family::Mem && G.c.cands[1].giant_masks);
    CHECK(candidate_name(G.c.cands[1]) == "k_mem giant (k_wide<1> home workgroup, sequential protocol over the HBM arrays, 19-word row masks)");
    const CyclePlan W = plan_cycle(F, cluster(1, 65537));
    CHECK(W.a.parts.empty() && W.c.cands.size() == 2 && W.c.cands[0].family == Family::Giant && !W.c.cands[1].giant_masks);
    CHECK(plan_cycle(F, cluster(1, 65536)).c.parts.empty());
    const CyclePlan X = plan_cycle(F, cluster(1, 544769, 2));
    CHECK(X.c.cands.empty() && std::string(X.c.exhausted) == "k_mem: a group wider than its giant row masks");
  }
  // ---- splits, and the composed names
  Inputs mix = cluster(5, 64);
  mix.parts[1].members = 2; mix.parts[2].jobs = 0; mix.parts[4] = Part{3, 20000, 2, false};
  const CyclePlan S = plan_cycle(F, mix);
  CHECK(S.split && !S.identity && !S.single() && S.a.parts == (std::vector<u32>{0, 3}) && S.b.parts == std::vector<u32>{1} && S.c.parts == std::vector<u32>{4});
  CHECK(S.b.second_stream && S.b.other_blocks == 0 && !S.a.second_stream && S.a.other_blocks == 1 + 1 && S.c.second_stream && S.c.other_blocks == 0 && S.c.max_np == 20000);
  CHECK(names(S.a) == "k_wide<1> x64 | k_pipe<1> | k_select<1>" && names(S.b) == "k_select<1>");
  CHECK(last_kernel_text(S, &S.a.cands[0], &S.b.cands[0], &S.c.cands[0]) ==
        "k_wide<1> x64 + k_select<1> on 1 of 5 partitions + k_mem (k_wide<1> home workgroup, sequential protocol over the HBM arrays) on 1 group(s) of up to 20000 slots");
  CHECK(kernel_of(S.a.cands[0]) == "k_wide<1>" && kernel_of(S.a.cands[1]) == "k_pipe<1>");   // the head of a split cycle's timing note
  mix.parts[4].jobs = 0;
  const CyclePlan S2 = plan_cycle(F, mix);
  CHECK(S2.split && S2.c.parts.empty() && S2.a.other_blocks == 1);
  CHECK(last_kernel_text(S2, &S2.a.cands[1], &S2.b.cands[0], nullptr) == "k_pipe<1> + k_select<1> on 1 of 5 partitions");
  mix.parts[1].jobs = 0;
  const CyclePlan S3 = plan_cycle(F, mix);   // one launch over the busy partitions
  CHECK(!S3.split && !S3.identity && S3.single() == &S3.a && last_kernel_text(S3, &S3.a.cands[0], nullptr, nullptr) == "k_wide<1> x64 on 2 busy of 5 partitions");
  const CyclePlan I = plan_cycle(F, cluster(3, 64));
  CHECK(I.identity && last_kernel_text(I, &I.a.cands[0], nullptr, nullptr) == "k_wide<1> x64");
  Inputs two = cluster(3, 64);
  two.parts[2].slots = 65537;   // every partition busy, two launches: no identity map
  const CyclePlan T = plan_cycle(F, two);
  CHECK(!T.split && !T.identity && T.single() == &T.a && T.a.other_blocks == 65 && T.c.cands[0].holds == 65);
  CHECK(last_kernel_text(T, &T.a.cands[0], nullptr, &T.c.cands[1]) ==
        "k_wide<1> x64 on 2 busy of 3 partitions + k_mem (k_wide<1> home workgroup, sequential protocol over the HBM arrays) on 1 group(s) of up to 65537 slots");
  two.helpers_unproven = true;   // ... planned again beside k_mem's one home workgroup
  const CyclePlan T2 = plan_cycle(F, two);
  CHECK(T2.a.other_blocks == 1 && T2.a.parts == T.a.parts && T2.c.parts == T.c.parts && names(T2.c) == "k_mem (k_wide<1> home workgroup, sequential protocol over the HBM arrays)");
  const CyclePlan C = plan_cycle(F, cluster(1, 65537));
  CHECK(last_kernel_text(C, nullptr, nullptr, &C.c.cands[0]) ==
        "k_giant (k_wide<1> home workgroup + 64 helper workgroups per partition, sequential protocol over the HBM arrays) on 1 group(s) of up to 65537 slots");
  Inputs idle = cluster(3, 64);
  for (Part& p : idle.parts) p.jobs = 0;
  const CyclePlan N = plan_cycle(F, idle);
  CHECK(!N.single() && !N.split && last_kernel_text(N, nullptr, nullptr, nullptr) == "none (no pending job reaches an ordered loop)");
  // ---- preemption
  {
    Inputs in = cluster(3, 64);
    in.parts[1].may_preempt = true;
    CHECK(plan_cycle(F, in).b.parts.empty());   // (not a cycle with preemption)
    in.pre_active = true;
    const CyclePlan P = plan_cycle(F, in);
    CHECK(P.split && P.b.parts == std::vector<u32>{1} && names(P.b) == "k_select<1>" && !P.unsupported);
    in.parts[1].slots = 37 * 448 + 1;
    const CyclePlan E = plan_cycle(F, in);
    CHECK(E.unsupported && E.error == "preemption among the jobs of a partition (or group of partitions sharing nodes) with more than 16576 (partition, node) slots");
  }
  // ---- the retry: no kernel whose workgroups wait for each other, whatever the switch
  for (Switch sw : {Switch::Unset, Switch::Wide, Switch::Wide8, Switch::Giant, Switch::Mem, Switch::Other}) {
    Inputs in = cluster(6, 64);
    in.parts[1].members = 2; in.parts[2].slots = 70000; in.parts[3] = Part{3, 200000, 2, false};
    in.sw = sw; in.protocol_off = true;
    const CyclePlan P = plan_cycle(F, in);
    CHECK(!has(P, Family::Wide) && !has(P, Family::Giant) && has(P, Family::Mem));
    for (const Launch* L : {&P.a, &P.b, &P.c}) for (const Candidate& c : L->cands) CHECK(!c.waits);
    in.protocol_off = false;
    CHECK((has(plan_cycle(F, in), Family::Giant) || sw == Switch::Mem) && (has(plan_cycle(F, in), Family::Wide) || sw == Switch::Giant));
  }
  // ---- experiment builds with one tile width: one candidate
  {
    Facts E = F;
    E.only_npl = 10;
    const CyclePlan P = plan_cycle(E, cluster(2, 4480));
    CHECK(names(P.a) == "k_select" && P.a.cands.size() == 1 && plan_cycle(E, cluster(2, 4481)).a.cands.empty());
  }
  if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
