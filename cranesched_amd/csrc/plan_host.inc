// The launch plan of a cycle: which partitions go to which of its (up to three) launches, and for every launch the ordered list of
// kernels that may serve it — family, build, tile width, extra home / helper workgroups, grid.  Pure arithmetic on the build's
// figures (Facts, filled by engine.hip from what the kernels export) and the pass's inputs (Inputs): no HIP, no getenv, no kernel
// symbol in here.  engine.hip walks the plan (run_resident_once); tests/cpp/plan_host_test.cpp compiles this file with g++ and holds
// it to the rules below row by row (tests/test_plan_host.py).  The one thing the plan cannot know is the runtime's occupancy answer:
// the launcher asks it for a candidate whose workgroups wait for each other and, on "not proven", takes the next candidate.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace cns_plan {

using u32 = uint32_t;
using u64 = uint64_t;

// CNS_SELECT_KERNEL, an A/B and test switch (read at every run).  Any set value wins over cns_config::kernel_pin.
//   unset   the default choice: per launch the widest k_wide build that fits, else k_pipe, else k_select; kernel_pin is honoured
//   legacy  k_select only;  pipe  k_pipe first, no k_wide
//   wide    k_wide wherever it fits (also in builds whose default is not k_wide);  wide32 | wide16 | wide8  ... its 32- / 16- / 8-wave build at most
//   giant   every partition and group without preemption on k_giant (k_mem where its helpers cannot run)
//   mem     the shapes of k_giant on k_mem: helpers off (19-word row masks above 143 360 slots)
//   any other word: the default choice with kernel_pin IGNORED (so do giant and mem for the partitions that stay on the ordinary kernels)
enum class Switch : uint8_t { Unset, Legacy, Pipe, Wide, Wide32, Wide16, Wide8, Giant, Mem, Other };
inline Switch parse_kernel_switch(const char* e) {
  static const struct { const char* word; Switch sw; } kWords[] = {{"legacy", Switch::Legacy}, {"pipe", Switch::Pipe},     {"wide", Switch::Wide},   {"wide32", Switch::Wide32},
                                                                  {"wide16", Switch::Wide16}, {"wide8", Switch::Wide8}, {"giant", Switch::Giant}, {"mem", Switch::Mem}};
  if (!e) return Switch::Unset;
  for (const auto& w : kWords) if (!strcmp(e, w.word)) return w.sw;
  return Switch::Other;
}
constexpr u32 kPinAuto = 0, kPinSelect = 1;   // cns_kernel_pin (engine.hip asserts the values)
constexpr u32 kGiantMinHelpers = 4;           // k_giant with fewer helper workgroups per partition is not worth its hand-off: k_mem (plan_serial_launch)

// ---- what the build says ------------------------------------------------------------------------------------------------------
struct Tiles {                        // a kernel's register tile: `lanes` nodes per row, instantiated for these rows per lane (ascending)
  u32 lanes = 0, block = 0;           // ... and its workgroup size
  std::vector<u32> widths;
  u32 slots() const { return widths.empty() ? 0u : lanes * widths.back(); }
  u32 width_for(u32 np) const { for (u32 w : widths) if (np <= lanes * w) return w; return 0; }   // the narrowest that holds np (0: none)
};
struct WideBuild {                    // one build of k_wide (wide_kernel.inc: WideInfo)
  u32 waves = 0, group = 0, max_parts = 0, aux_max = 0, last_in_lds_rows = 0;
  Tiles tiles;
  std::vector<u32> window_widths;     // the widths that also have a windows build (ascending)
};
struct Facts {
  WideBuild wide[4];                  // widest first: 64, 32, 16, 8 scanner waves per partition; k_mem / k_giant are the last one's
  Tiles select, pipe;
  u32 only_npl = 0;                   // experiment builds (-DCNS_ONLY_NPL): k_select at this one width is the only kernel of a plain launch
  u32 mem_slots = 0, giant_mem_slots = 0, giant_helpers_max = 0, giant_helper_budget = 0;
  bool default_wide = true, default_pipe = true;
};

// ---- what the pass says ---------------------------------------------------------------------------------------------------------
struct Part { u64 jobs = 0; u32 slots = 0, members = 1; bool may_preempt = false; };   // jobs that reach its ordered loop, (partition, node) slots,
                                                                                       // caller partitions it runs, a pending job's qos may preempt
struct Inputs {
  std::vector<Part> parts;            // every engine partition
  bool pre_active = false;            // a cycle with preemption
  u32 num_cus = 0, kernel_pin = kPinAuto;
  Switch sw = Switch::Unset;
  bool protocol_off = false;          // the retry after a protocol fault: no kernel whose workgroups wait for each other
  bool helpers_unproven = false;      // this pass's runtime could not prove k_giant's helpers co-resident: planned again without them
  u32 wide_window = 0;                // KParams::wide_window (>= 2: the windows build where there is one)
  int64_t aux_override = -1;          // CNS_WIDE_AUX (-1: unset)
};

// ---- the plan -------------------------------------------------------------------------------------------------------------------
enum class Family : uint8_t { Wide, Pipe, Select, Mem, Giant };
struct Candidate {
  Family family = Family::Select;
  u32 build = 0, waves = 0;           // k_wide: index into Facts::wide, its scanner waves
  u32 width = 0;                      // tile rows per lane (k_select 0: the experiment build's one kernel)
  bool windows = false;               // k_wide: the windows build
  bool giant_masks = false;           // k_mem: the 19-word instantiation
  u32 extra = 0;                      // k_wide: extra home workgroups per partition; k_giant: helper workgroups per partition
  u32 grid = 0, block = 0;
  u32 holds = 0;                      // workgroups that keep a CU while the cycle's other launches run
  bool waits = false;                 // its workgroups wait for each other: launched only with a proof that all are resident at once,
};                                    // and a protocol fault (code >= 20) of the pass is re-run without such kernels
struct Launch {
  std::vector<u32> parts;             // (empty: no such launch)
  u32 max_np = 0;                     // widest of them
  bool second_stream = false;
  u32 other_blocks = 0;               // workgroups of the cycle's other launches (they hold CUs while this one needs all of its own resident)
  std::vector<Candidate> cands;       // in order: the launcher takes the first that launches
  const char* exhausted = "";         // the error when none does
};
struct CyclePlan {
  Launch a, b, c;                     // plain partitions (k_wide / k_pipe / k_select) | shared groups and preempting partitions (k_select) | k_giant / k_mem
  u32 num_parts = 0;
  bool split = false;                 // a and b both run, b on the second stream
  bool identity = false;              // the single launch serves every partition: no part_map
  bool unsupported = false;           // CNS_ERR_UNSUPPORTED before anything is launched
  std::string error;
  const Launch* single() const { return split ? nullptr : !a.parts.empty() ? &a : !b.parts.empty() ? &b : nullptr; }
};

// One launch over partitions that neither share nodes nor run with preemption (`plain`): k_wide -> k_pipe<w> -> k_select<w>; any other: k_select<w>.
inline void plan_launch(const Facts& F, const Inputs& in, bool plain, Launch& L) {
  const u32 nparts = (u32)L.parts.size(), np = L.max_np;
  L.exhausted = "partition too large for the widest register tile";
  if (F.only_npl) {
    L.exhausted = "experiment build: partition too large for its one tile width";
    if (np <= F.select.lanes * F.only_npl) { Candidate c; c.grid = nparts; c.block = F.select.block; c.holds = nparts; L.cands.push_back(c); }
    return;
  }
  bool wide = plain && F.default_wide, pipe = plain && F.default_pipe;
  u32 first = 0;                      // (wide32 | wide16 | wide8 cap the build)
  switch (in.sw) {
    case Switch::Legacy: wide = pipe = false; break;
    case Switch::Pipe: wide = false; pipe = plain; break;
    case Switch::Wide: case Switch::Wide32: case Switch::Wide16: case Switch::Wide8: wide = pipe = plain; first = (u32)in.sw - (u32)Switch::Wide; break;
    case Switch::Unset:               // (cns_config::kernel_pin: a controller that shares its GPU; the environment variable wins)
      if (in.kernel_pin != kPinAuto) wide = false;
      if (in.kernel_pin == kPinSelect) pipe = false;
      break;
    default: break;
  }
  // k_wide (many CUs per partition) when every workgroup of the launch can be resident at once, one per CU, and the partitions fit its tile:
  // 64 scanner waves per partition (17 workgroups) for up to 8 partitions, 32 (9 workgroups) for up to 24, 16 (5) for up to 48, 8 (3) for up
  // to 80 — the widest build that fits.  A partitioned or smaller device falls to k_pipe; an unknown CU count is no proof, so no k_wide.
  const u32 groups = (nparts + 7u) / 8u;   // the workgroups of a partition share blockIdx % 8 (= the XCD, observed)
  for (u32 b = first; wide && !in.protocol_off && in.num_cus != 0 && b < 4; ++b) {
    const WideBuild& W = F.wide[b];
    if (nparts > W.max_parts || np > W.tiles.slots() || (u64)8u * groups * W.group + L.other_blocks > in.num_cus) continue;
    Candidate c;
    c.family = Family::Wide; c.build = b; c.waves = W.waves; c.block = W.tiles.block; c.waits = true;
    for (u32 w : W.window_widths) if (!c.width && in.wide_window >= 2u && np <= W.tiles.lanes * w) { c.width = w; c.windows = true; }
    if (!c.width) c.width = W.tiles.width_for(np);
    // Extra home workgroups per partition (wide_kernel.inc, "MORE THAN ONE HOME WORKGROUP PER PARTITION"): as many as the build allows, as long as
    // every workgroup of the launch still gets a CU of "its" XCD (32 each, `groups` partitions per XCD) and of the device (other launches of the
    // cycle hold theirs); none for tiles whose last-task table is not in LDS.  ONE extra home is the default: with two homes the scanners pace every
    // configuration measured (C5 184.6 -> 146.6 ms, C2 139.4 -> 114.2; a third and a fourth home: 146.3 / 114.2 — profiles/r06_ab_home_workgroups.txt).
    // CNS_WIDE_AUX=<n> sets the number (0: rounds 2-5's single home; up to the build's maximum: the parity tests run them all).
    u32 aux = std::min<u64>(in.aux_override < 0 ? 1 : in.aux_override, W.aux_max);
    if (np > W.tiles.lanes * W.last_in_lds_rows) aux = 0;
    while (aux > 0 && (groups * (W.group + aux) > 32u || (u64)8u * groups * (W.group + aux) + L.other_blocks > in.num_cus)) --aux;
    c.extra = aux;
    c.grid = c.holds = 8u * groups * (W.group + aux);
    L.cands.push_back(c);
    break;
  }
  // k_pipe (decoupled test / commit pipeline) for partitions its tile covers, k_select otherwise: one workgroup per partition, no co-residency needed
  const struct { bool use; Family family; const Tiles& t; } rest[] = {{pipe, Family::Pipe, F.pipe}, {true, Family::Select, F.select}};
  for (const auto& r : rest)
    if (const u32 w = r.use ? r.t.width_for(np) : 0u) {
      Candidate c;
      c.family = r.family; c.width = w; c.grid = c.holds = nparts; c.block = r.t.block;
      L.cands.push_back(c);
    }
}

// The launch on k_wide's home workgroup alone (KParams::serial_only): k_giant — helper workgroups that scan stripes of the slots; they and the
// home wait for each other — then k_mem, which is exact, slow and needs no co-residency: its two scanner workgroups per partition leave at once.
inline void plan_serial_launch(const Facts& F, const Inputs& in, bool giant_shape, Launch& L) {
  const u32 nparts = (u32)L.parts.size();
  const WideBuild& W = F.wide[3];
  L.exhausted = "k_mem: a group wider than its giant row masks";
  if (L.max_np > F.giant_mem_slots) return;   // (cns_set_nodes refuses such groups: never reached)
  // 64 helper workgroups per launch at most (8 per XCD): C4's k_wide launch beside it keeps its 8 x 17 workgroups
  const u32 nh = std::min(F.giant_helpers_max, F.giant_helper_budget / std::max(nparts, 1u));
  if ((giant_shape || in.sw == Switch::Giant) && in.sw != Switch::Mem && !in.protocol_off && !in.helpers_unproven && in.num_cus != 0 && nh >= kGiantMinHelpers) {
    Candidate c;
    c.family = Family::Giant; c.build = 3; c.waves = W.waves; c.width = 1; c.giant_masks = true; c.extra = nh; c.block = W.tiles.block; c.waits = true;
    c.grid = c.holds = nparts * (1u + nh);   // the home of partition i is block i
    L.cands.push_back(c);
  }
  Candidate c;
  c.family = Family::Mem; c.build = 3; c.waves = W.waves; c.width = 1; c.giant_masks = L.max_np > F.mem_slots; c.block = W.tiles.block;
  c.grid = 8u * ((nparts + 7u) / 8u) * W.group;
  c.holds = nparts;                           // its home workgroups
  L.cands.push_back(c);
}

// Which partitions need k_select: groups of partitions that share nodes (one time map per node, a cost per partition) and, in a cycle with
// preemption, the partitions that have a pending job whose qos may preempt anything (TryPreempt_ returns at JobScheduler.cpp:6384-6385 for
// every other job).  Everything else runs on k_wide / k_pipe IN THE SAME CYCLE, side by side on a second stream: partitions with disjoint node
// sets never interact (:6723-6732,6746-6761).  Only partitions that HAVE pending jobs get a scheduler (the reference builds NodeStates and a
// LocalScheduler only for the partitions some pending job names, JobScheduler.cpp:6516-6530,6571-6573,6723-6732): the launch, and with it the
// choice of the k_wide build (workgroups per partition), is sized by the busy partitions, not by the snapshot.  A group that is wider than
// k_select's register tile runs on k_wide's home workgroup alone (c): the ordinary "ALL partition over the whole cluster" layout of a large
// site; so does a partition that shares no node and is wider than k_wide's widest tile — c needs no co-residency, and what the ordinary kernels
// hold stays on them.  Such a partition, or a group wider than k_mem's ordinary masks, makes c a k_giant launch.
inline CyclePlan plan_cycle(const Facts& F, const Inputs& in) {
  CyclePlan P;
  P.num_parts = (u32)in.parts.size();
  bool giant_shape = false;
  auto add = [](Launch& L, u32 p, u32 np) { L.parts.push_back(p); L.max_np = std::max(L.max_np, np); };
  for (u32 p = 0; p < P.num_parts; ++p) {
    const Part& q = in.parts[p];
    if (q.jobs == 0) continue;
    const bool pre = in.pre_active && q.may_preempt, sel = q.members > 1 || pre;
    const bool giant = !sel && q.slots > F.wide[0].tiles.slots();
    giant_shape = giant_shape || giant || (sel && !pre && q.slots > F.mem_slots);
    if (giant || (in.sw == Switch::Giant && !pre)) add(P.c, p, q.slots);
    else if (sel && q.slots > F.select.slots()) {
      if (pre) {
        P.unsupported = true;
        P.error = "preemption among the jobs of a partition (or group of partitions sharing nodes) with more than " + std::to_string(F.select.slots()) + " (partition, node) slots";
        return P;
      }
      add(P.c, p, q.slots);
    } else add(sel ? P.b : P.a, p, q.slots);
  }
  u32 held = 0;                       // what c holds, were its first candidate to launch (else: Inputs::helpers_unproven)
  if (!P.c.parts.empty()) {
    P.c.second_stream = true;
    plan_serial_launch(F, in, giant_shape, P.c);
    if (!P.c.cands.empty()) held = P.c.cands[0].holds;
  }
  P.split = !P.a.parts.empty() && !P.b.parts.empty();
  P.identity = !P.split && P.single() && P.single()->parts.size() == P.num_parts;
  P.b.second_stream = P.split;        // b first: its few workgroups take their CUs
  P.b.other_blocks = P.split ? 0u : held;
  P.a.other_blocks = (P.split ? (u32)P.b.parts.size() : 0u) + held;
  if (!P.a.parts.empty()) plan_launch(F, in, true, P.a);
  if (!P.b.parts.empty()) plan_launch(F, in, false, P.b);
  return P;
}

// ---- names ----------------------------------------------------------------------------------------------------------------------
inline std::string kernel_of(const Candidate& c) {   // the kernel as a profile shows it
  const char* fam = c.family == Family::Wide ? "k_wide" : c.family == Family::Pipe ? "k_pipe" : c.family == Family::Select ? "k_select" : c.family == Family::Mem ? "k_mem" : "k_giant";
  return c.family <= Family::Select && c.width ? std::string(fam) + "<" + std::to_string(c.width) + ">" : std::string(fam);
}
inline std::string candidate_name(const Candidate& c) {
  switch (c.family) {
    case Family::Wide: return kernel_of(c) + (c.windows ? " windows x" : " x") + std::to_string(c.waves);   // (x64: cns::w64::k_wide in a profile, x32: cns::w32::k_wide, ...)
    case Family::Mem: return c.giant_masks ? "k_mem giant (k_wide<1> home workgroup, sequential protocol over the HBM arrays, 19-word row masks)"
                                           : "k_mem (k_wide<1> home workgroup, sequential protocol over the HBM arrays)";
    case Family::Giant: return "k_giant (k_wide<1> home workgroup + " + std::to_string(c.extra) + " helper workgroups per partition, sequential protocol over the HBM arrays)";
    default: return kernel_of(c);
  }
}
// cns_debug_last_kernel of a pass: the candidates that launched (null: no such launch).  Never empty: callers parse it.
inline std::string last_kernel_text(const CyclePlan& P, const Candidate* a, const Candidate* b, const Candidate* c) {
  const std::string of = " of " + std::to_string(P.num_parts) + " partitions";
  const std::string name_c = c ? candidate_name(*c) + " on " + std::to_string(P.c.parts.size()) + " group(s) of up to " + std::to_string(P.c.max_np) + " slots" : "";
  std::string s;
  if (P.split) s = candidate_name(*a) + " + " + candidate_name(*b) + " on " + std::to_string(P.b.parts.size()) + of;
  else if (const Launch* L = P.single()) s = candidate_name(a ? *a : *b) + (P.identity ? "" : " on " + std::to_string(L->parts.size()) + " busy" + of);
  else return c ? name_c : "none (no pending job reaches an ordered loop)";
  return c ? s + " + " + name_c : s;
}

}  // namespace cns_plan
