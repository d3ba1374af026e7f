// The snapshot layout of a cycle: what cns_set_nodes, cns_set_reservations and cns_set_running derive from the caller's arrays before
// anything goes to the device — the union-find over shared nodes, the refusals group by group, the slot list, the virtual partitions of
// the reservations, the node types, the tag ranges of a group's members, the running allocations grouped by slot.  Pure arithmetic on the
// ABI structs: no HIP, no handle, no error string but the one a builder returns.  Three values, three builders; a builder writes its
// result only when it succeeds, so a refused call leaves the caller's previous value as it was.  engine.hip holds the three values in
// cns_engine, uploads them and sizes the per-slot buffers; tests/cpp/snapshot_host_test.cpp compiles this file with g++ and compares it
// field by field with the walk it replaced (tests/test_snapshot_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "res_dev.h"

namespace cns_snapshot {

using cns::Res;
using cns::i64;
using cns::u32;
using cns::u64;

constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u32 kTlCap = 1008;          // entries of a node's time map (engine.hip asserts both against the kernels' constants)
constexpr u32 kMaxResvPerNode = 200;  // release + dip events of a node share the node block's upper half with the running allocations (k_init_nodes)

// The limits of a build.  Parameters, not constants: the CPU test reaches them with snapshots of a few nodes.
struct Caps {
  u32 part_slots, group_slots;   // the widest partition that shares no node (and the widest reservation), the widest group of partitions that share nodes
  u32 node_types;                // distinct res_total records of a snapshot (CNS_MAX_NODE_TYPES)
};
struct Status {
  int code = 0;                  // CNS_OK or a cns_status
  std::string msg;
  explicit operator bool() const { return code != 0; }
};

// cns_set_nodes.  Partitions connected through shared nodes form ONE engine partition (workgroup) that runs their jobs in queue order; a node
// then has one slot per member partition (one NodeState per craned, one cost per partition: JobScheduler.cpp:6585-6615, JobScheduler.h:498-516).
struct Layout {
  u32 N = 0, Pu = 0, P_real = 0, S_real = 0;  // nodes, partitions of the caller; engine partitions and their slots (without reservations)
  u32 max_np = 0;                             // slots of the widest engine partition
  bool shared = false;                        // some node belongs to several partitions
  bool wide_cores = false;                    // a node has a core id above 127: the results carry the core_w2 / core_w3 planes
  bool big_nodes = false;                     // any GRES or > 64 cores (48-byte node record in the traffic model)
  u64 all_gres = 0;                           // every bit of a defined GRES class
  Caps caps{};
  std::vector<u32> part_off, slot_node;       // [P_real + 1], [S_real]
  std::vector<u32> node_slot;                 // node -> its PRIMARY slot (the one whose NodeBlock holds the shared time map) or kNone
  std::vector<std::vector<u32>> node_slots;   // node -> all its slots
  std::vector<u32> orig_pos_slot;             // caller's part_nodes position -> slot or kNone
  std::vector<Res> node_total;                // res_total per node
  std::vector<u32> upart_eng, upart_size;     // caller's partition -> engine partition, its schedulable node count,
  std::vector<uint8_t> upart_tag, upart_refused, slot_tag;   // ... its member tag there, its cns_partition_status (!= 0: refused); slot -> tag
  std::vector<u32> eng_members;               // engine partition -> number of caller partitions it runs (> 1: they share nodes)
  // the slots of a group are its member partitions' lists one after the other: member t (its tag) owns [tag_off[b + t], tag_off[b + t + 1])
  // relative to the group's first slot, b = tag_base[group]
  std::vector<u32> tag_off, tag_base;
};

// cns_set_reservations.  Slots [0, S_real) are the partitions' nodes, slots [S_real, S) the virtual nodes of the reservations: one extra
// "partition" P_real + v per reservation v (JobScheduler.cpp:6657-6668), its nodes ascending.  Without reservations: the Layout's own lists.
struct ResvLayout {
  u32 V = 0, P = 0, S = 0, T = 0;             // reservations, engine partitions, slots, node types
  u32 max_np = 0;                             // Layout::max_np and big_nodes with THIS call's reservations counted in
  bool big_nodes = false;
  std::vector<u32> part_off, slot_node;       // [P + 1], [S]
  std::vector<Res> slot_total;                // res_total per slot (virtual slots: the reserved share)
  std::vector<i64> slot_end;                  // end of the slot's time map (INF, or the reservation's end)
  std::vector<i64> resv_start, resv_end;      // per reservation
  std::vector<u32> rv_off;                    // [S + 1] reservation entries touching a REAL slot
  std::vector<i64> rv_start, rv_endt;
  std::vector<Res> rv_res, type_total;        // ... and the T node types: first seen over the slots in ascending order
  std::vector<uint8_t> slot_type, slot_tag;
  // snapshots with shared nodes only: slot_tag (virtual slots: 0), every slot's primary slot and siblings, the tag ranges (one per virtual partition)
  std::vector<u32> slot_block, sib_off, sib, tag_base, tag_off;
  // the virtual slot of node n in reservation v (kNone: unknown reservation, or it does not list the node)
  u32 resv_slot(u32 P_real, u32 v, u32 n) const {
    if (v >= V) return kNone;
    const auto b = slot_node.begin() + part_off[P_real + v], e = slot_node.begin() + part_off[P_real + v + 1];
    const auto it = std::lower_bound(b, e, n);
    return it != e && *it == n ? (u32)(it - slot_node.begin()) : kNone;
  }
};

// cns_set_running.  Allocations grouped by SLOT, per slot in input order (the cost accumulation order): every slot of the node, or — for a
// job running inside a reservation (JobScheduler.cpp:6692-6707) — the reservation's virtual node.
struct RunLayout {
  u32 R = 0;                                  // running jobs
  std::vector<u32> rn_off, ent_job, ent_slot; // [S + 1]; entry -> running job, slot,
  std::vector<i64> rn_end;                    // ... end time as handed in,
  std::vector<Res> rn_res;                    // ... resources
};

// row i of a caller's SoA as a Res (the planes that may be NULL count as 0)
inline Res res_row(const int64_t* cpu, const uint64_t* mem, const uint64_t* clo, const uint64_t* chi, const uint64_t* c2, const uint64_t* c3,
                   const uint64_t* gres, u32 i) {
  Res r;
  r.cpu = cpu[i]; r.mem = mem[i]; r.clo = clo[i];
  r.chi = chi ? chi[i] : 0; r.c2 = c2 ? c2[i] : 0; r.c3 = c3 ? c3[i] : 0;
  r.gres = gres ? gres[i] : 0;
  return r;
}
template <class Soa>   // cns_resv_soa, cns_running_soa
inline Res alloc_row(const Soa& s, u32 a) {
  return res_row(s.alloc_cpu_raw, s.alloc_mem, s.alloc_core_lo, s.alloc_core_hi, s.alloc_core_w2, s.alloc_core_w3, s.alloc_gres, a);
}
// a node type is a distinct res_total record
using TypeKey = std::tuple<i64, u64, u64, u64, u64, u64, u64>;
inline TypeKey type_key(const Res& r) { return std::make_tuple(r.cpu, r.mem, r.clo, r.chi, r.gres, r.c2, r.c3); }

// `refused` (may be null) gets the statuses of the partitions on the two paths that compute them: success, and the failure because EVERY
// partition was refused (cns_group_set_nodes tells that one from a hard error by it).
inline Status build_layout(const cns_node_soa* nd, u64 all_gres, const Caps& caps, Layout& out, std::vector<uint8_t>* refused = nullptr) {
  Layout L;
  const u32 N = nd->num_nodes, P = nd->num_partitions;
  L.N = N; L.Pu = P; L.all_gres = all_gres; L.caps = caps;
  std::vector<Res>& total = L.node_total;
  total.resize(N);
  for (u32 n = 0; n < N; ++n) {
    total[n] = res_row(nd->cpu_total_raw, nd->mem_total, nd->core_lo, nd->core_hi, nd->core_w2, nd->core_w3, nd->gres_slots, n);
    if (total[n].c2 | total[n].c3) L.wide_cores = true;
    if (total[n].gres & ~all_gres) return {CNS_ERR_INVALID_ARG, "node GRES slot outside every class"};
    if (total[n].gres || total[n].chi) L.big_nodes = true;
  }
  L.big_nodes = L.big_nodes || L.wide_cores;
  // partitions: schedulable nodes only, ascending dense index (= canonical cost tie-break).  Partitions that share a
  // node are merged into one engine partition (union-find over the shared nodes); without sharing the engine
  // partitions are the caller's, one to one.
  std::vector<std::vector<std::pair<u32, u32>>> plist(P);  // per caller partition: (node, original position)
  std::vector<u32> uf(P);
  for (u32 p = 0; p < P; ++p) uf[p] = p;
  auto find = [&](u32 x) { while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; } return x; };
  auto join = [&](u32 x, u32 y) { const u32 a = find(x), b = find(y); if (a != b) uf[std::max(a, b)] = std::min(a, b); };
  std::vector<u32> first_part(N, kNone);
  // What lies outside the engine's limits refuses ONLY the partitions it touches — the group of partitions connected through shared
  // nodes that lists the node (the reference bounds none of this: CpuSet is a std::set<uint32_t>, GRES maps are unbounded,
  // PublicHeader.h:555-573,427-494): a node the caller flags as not expressible in this ABI's formats (cns_node_soa::unsupported:
  // a core id >= 256, more GRES slots than the 64-bit mask holds), a node whose cpu count does not fit, the 65th distinct res_total
  // record, a group wider than the widest tile.  Their jobs come back with CNS_REASON_ENGINE_REFUSED; the caller's CPU scheduler takes them.
  std::vector<uint8_t> part_bad(P, 0);
  for (u32 p = 0; p < P; ++p) {
    if (nd->part_offsets[p + 1] < nd->part_offsets[p]) return {CNS_ERR_INVALID_ARG, "part_offsets not monotone"};
    auto& lst = plist[p];
    for (u32 i = nd->part_offsets[p]; i < nd->part_offsets[p + 1]; ++i) {
      const u32 n = nd->part_nodes[i];
      if (n >= N) return {CNS_ERR_INVALID_ARG, "part_nodes entry >= num_nodes"};
      if (nd->schedulable && !nd->schedulable[n]) continue;  // JobScheduler.cpp:6595
      const bool unsup = nd->unsupported && nd->unsupported[n];
      if (unsup || total[n].cpu <= 0 || total[n].cpu >= 0x7FFFFFFEll) {
        part_bad[p] = unsup ? CNS_PART_REFUSED_NODE : CNS_PART_REFUSED_CPU;
        if (first_part[n] == kNone) first_part[n] = p;   // (the partitions that share this node go with it)
        else join(first_part[n], p);
        continue;
      }
      lst.emplace_back(n, i);
    }
    std::sort(lst.begin(), lst.end());
    for (size_t i = 1; i < lst.size(); ++i)
      if (lst[i].first == lst[i - 1].first) return {CNS_ERR_INVALID_ARG, "node listed twice in one partition"};
    for (auto& [n, pos] : lst) {
      if (first_part[n] == kNone) first_part[n] = p;
      else { L.shared = true; join(first_part[n], p); }
    }
  }
  L.upart_eng.resize(P); L.upart_size.resize(P); L.upart_tag.assign(P, 0);
  std::vector<std::vector<u32>> members;  // engine partition -> caller partitions, ascending
  {
    std::vector<u32> eng_of_root(P, kNone);
    for (u32 p = 0; p < P; ++p) {
      const u32 r = find(p);
      if (eng_of_root[r] == kNone) { eng_of_root[r] = (u32)members.size(); members.emplace_back(); }
      auto& m = members[L.upart_eng[p] = eng_of_root[r]];
      if (m.size() >= 255) return {CNS_ERR_UNSUPPORTED, "more than 255 partitions connected through shared nodes"};
      L.upart_tag[p] = (uint8_t)m.size();
      m.push_back(p);
      L.upart_size[p] = (u32)plist[p].size();
    }
  }
  const u32 PE = (u32)members.size();
  // ---- refusals, group by group (in engine-partition order: which group gets the last free node type is deterministic) ----
  L.upart_refused.assign(P, 0);
  {
    std::set<TypeKey> types;
    bool any_served = false;
    for (u32 e = 0; e < PE; ++e) {
      uint8_t why = 0;
      u32 npe = 0;
      for (u32 p : members[e]) { if (!why) why = part_bad[p]; npe += (u32)plist[p].size(); }
      if (!why && npe > (members[e].size() > 1 ? caps.group_slots : caps.part_slots)) why = CNS_PART_REFUSED_WIDTH;
      if (!why) {
        auto mine = types;
        for (u32 p : members[e])
          for (auto& [n, pos] : plist[p]) mine.insert(type_key(total[n]));
        if (mine.size() > caps.node_types) why = CNS_PART_REFUSED_TYPES;
        else types.swap(mine);
      }
      if (why)
        for (u32 p : members[e]) { L.upart_refused[p] = why; plist[p].clear(); L.upart_size[p] = 0; }
      any_served = any_served || !why;
    }
    if (refused) *refused = L.upart_refused;
    if (!any_served) return {CNS_ERR_UNSUPPORTED, "every partition of the snapshot is outside the engine's limits (a node flagged unsupported, a cpu count outside (0, 2^31-2), more than 64 distinct res_total records, or a group wider than the widest tile)"};
  }
  L.part_off.assign(PE + 1, 0); L.node_slot.assign(N, kNone); L.node_slots.resize(N);
  L.orig_pos_slot.assign(nd->part_offsets[P], kNone);
  L.tag_base.assign(PE, 0);
  for (u32 e = 0; e < PE; ++e) {
    const u32 first = L.part_off[e] = (u32)L.slot_node.size();
    L.tag_base[e] = (u32)L.tag_off.size();
    for (u32 p : members[e]) {
      L.tag_off.push_back((u32)L.slot_node.size() - first);
      for (auto& [n, pos] : plist[p]) {
        const u32 q = (u32)L.slot_node.size();
        if (L.node_slot[n] == kNone) L.node_slot[n] = q;
        L.node_slots[n].push_back(q);
        L.orig_pos_slot[pos] = q;
        L.slot_node.push_back(n);
        L.slot_tag.push_back(L.upart_tag[p]);
      }
    }
    L.tag_off.push_back((u32)L.slot_node.size() - first);
    L.max_np = std::max<u32>(L.max_np, (u32)L.slot_node.size() - first);
    L.eng_members.push_back((u32)members[e].size());
  }
  L.P_real = PE;
  L.S_real = L.part_off[PE] = (u32)L.slot_node.size();
  out = std::move(L);
  return {};
}

// rv == nullptr or no reservation: the layout of cns_set_nodes with its per-slot tables
inline Status build_resv(const Layout& L, const cns_resv_soa* rv, ResvLayout& out) {
  ResvLayout X;
  const u32 V = rv ? rv->num_resv : 0;
  if (V && (!rv->start_sec || !rv->end_sec || !rv->alloc_offsets || !rv->alloc_node || !rv->alloc_cpu_raw || !rv->alloc_mem || !rv->alloc_core_lo))
    return {CNS_ERR_INVALID_ARG, "cns_set_reservations: missing array"};
  X.V = V; X.max_np = L.max_np; X.big_nodes = L.big_nodes;
  X.part_off = L.part_off; X.slot_node = L.slot_node;
  X.slot_total.resize(L.S_real);
  for (u32 q = 0; q < L.S_real; ++q) X.slot_total[q] = L.node_total[L.slot_node[q]];
  X.slot_end.assign(L.S_real, INT64_MAX);
  std::vector<std::vector<std::tuple<i64, i64, Res>>> per_slot(V ? L.S_real : 0);  // reservation entries of the real slots
  for (u32 v = 0; v < V; ++v) {
    if (rv->alloc_offsets[v + 1] < rv->alloc_offsets[v]) return {CNS_ERR_INVALID_ARG, "reservation alloc_offsets not monotone"};
    std::vector<std::pair<u32, Res>> al;
    for (u32 a = rv->alloc_offsets[v]; a < rv->alloc_offsets[v + 1]; ++a) {
      const u32 n = rv->alloc_node[a];
      if (n >= L.N) return {CNS_ERR_INVALID_ARG, "reservation node >= num_nodes"};
      const Res r = alloc_row(*rv, a);
      if (r.gres & ~L.all_gres) return {CNS_ERR_INVALID_ARG, "reservation GRES slot outside every class"};
      if (r.cpu <= 0 || r.cpu >= 0x7FFFFFFEll) return {CNS_ERR_UNSUPPORTED, "reservation cpu share must be in (0, 2^31-2)"};
      al.emplace_back(n, r);
      if (r.gres || r.chi) X.big_nodes = true;
    }
    std::sort(al.begin(), al.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t i = 1; i < al.size(); ++i)
      if (al[i].first == al[i - 1].first) return {CNS_ERR_INVALID_ARG, "node listed twice in one reservation"};
    if (al.size() > L.caps.part_slots) return {CNS_ERR_UNSUPPORTED, "reservation over more than " + std::to_string(L.caps.part_slots) + " nodes"};
    for (auto& [n, r] : al) {   // a virtual node: its own NodeState (:6661-6664)
      X.slot_node.push_back(n);
      X.slot_total.push_back(r);
      X.slot_end.push_back(rv->end_sec[v]);
      for (u32 q : L.node_slots[n]) per_slot[q].emplace_back(rv->start_sec[v], rv->end_sec[v], r);   // every partition's slot of the node
    }
    X.part_off.push_back((u32)X.slot_node.size());
    X.resv_start.push_back(rv->start_sec[v]); X.resv_end.push_back(rv->end_sec[v]);
    X.max_np = std::max<u32>(X.max_np, (u32)al.size());
  }
  const u32 S = X.S = (u32)X.slot_node.size();
  X.P = L.P_real + V;
  X.rv_off.assign(S + 1, 0);
  for (u32 q = 0; q < (u32)per_slot.size(); ++q) {
    if (per_slot[q].size() > kMaxResvPerNode) return {CNS_ERR_UNSUPPORTED, "more than 200 reservations on one node"};
    for (auto& [st, en, r] : per_slot[q]) { X.rv_start.push_back(st); X.rv_endt.push_back(en); X.rv_res.push_back(r); }
    X.rv_off[q + 1] = (u32)X.rv_start.size();
  }
  for (u32 q = (u32)per_slot.size(); q < S; ++q) X.rv_off[q + 1] = X.rv_off[q];
  std::map<TypeKey, u32> tmap;
  X.slot_type.resize(S);
  for (u32 q = 0; q < S; ++q) {
    auto it = tmap.find(type_key(X.slot_total[q]));
    if (it == tmap.end()) {
      if (X.type_total.size() >= L.caps.node_types) return {CNS_ERR_UNSUPPORTED, "more than 64 distinct res_total records (nodes + reservation shares)"};
      it = tmap.emplace(type_key(X.slot_total[q]), (u32)X.type_total.size()).first;
      X.type_total.push_back(X.slot_total[q]);
    }
    X.slot_type[q] = (uint8_t)it->second;
  }
  X.T = (u32)X.type_total.size();
  if (L.shared) {
    X.slot_block.resize(S); X.sib_off.assign(S + 1, 0);
    for (u32 q = 0; q < S; ++q) {
      X.slot_block[q] = q;
      if (q < L.S_real) {
        const auto& all = L.node_slots[L.slot_node[q]];
        X.slot_block[q] = all.front();
        for (u32 o : all) if (o != q) X.sib.push_back(o);
      }
      X.sib_off[q + 1] = (u32)X.sib.size();
    }
    X.slot_tag = L.slot_tag;
    X.slot_tag.resize(S, 0);
    // the virtual partitions of reservations share nothing: one range over all of their slots (their jobs carry tag 0).  Read only by
    // k_mem (a reservation wider than k_wide's tile); the other kernels take a partition without shared nodes whole.
    X.tag_base = L.tag_base; X.tag_off = L.tag_off;
    for (u32 p = L.P_real; p < X.P; ++p) {
      X.tag_base.push_back((u32)X.tag_off.size());
      X.tag_off.push_back(0); X.tag_off.push_back(X.part_off[p + 1] - X.part_off[p]);
    }
  }
  out = std::move(X);
  return {};
}

// rn == nullptr or no running job: every slot empty
inline Status build_running(const Layout& L, const ResvLayout& X, const cns_running_soa* rn, RunLayout& out) {
  RunLayout U;
  const u32 S = X.S;
  U.rn_off.assign(S + 1, 0);
  if (rn && rn->num_jobs) {
    if (!rn->end_sec || !rn->alloc_offsets || !rn->alloc_node || !rn->alloc_cpu_raw || !rn->alloc_mem || !rn->alloc_core_lo)
      return {CNS_ERR_INVALID_ARG, "cns_set_running: missing array"};
    if (rn->alloc_offsets[rn->num_jobs] != rn->num_allocs) return {CNS_ERR_INVALID_ARG, "cns_set_running: num_allocs mismatch"};
    // the slots an allocation of job j on node n counts on: none for an unschedulable node (:6685-6686), a reservation that is not found
    // (:6693-6700) or does not list the node
    u32 one = kNone;
    auto slots_of = [&](u32 j, u32 n) -> std::pair<const u32*, const u32*> {
      const u32 v = rn->reservation ? rn->reservation[j] : CNS_RESV_NONE;
      if (v == CNS_RESV_NONE) return {L.node_slots[n].data(), L.node_slots[n].data() + L.node_slots[n].size()};
      one = X.resv_slot(L.P_real, v, n);
      return {&one, &one + (one != kNone)};
    };
    u32* const off = U.rn_off.data();
    for (u32 j = 0; j < rn->num_jobs; ++j)
      for (u32 a = rn->alloc_offsets[j]; a < rn->alloc_offsets[j + 1]; ++a) {
        const u32 n = rn->alloc_node[a];
        if (n >= L.N) return {CNS_ERR_INVALID_ARG, "running allocation on node >= num_nodes"};
        for (auto [q, e] = slots_of(j, n); q != e; ++q) off[*q + 1]++;
      }
    for (u32 q = 0; q < S; ++q) {
      const u32 nrv = X.rv_off[q + 1] - X.rv_off[q];
      if (nrv ? off[q + 1] + 2 * nrv + 2 > kTlCap / 2 : off[q + 1] + 2 > kTlCap)
        return {CNS_ERR_UNSUPPORTED, "too many running allocations / reservations on one node (1006, or 502 events with reservations)"};
      off[q + 1] += off[q];
    }
    U.rn_end.resize(off[S]); U.rn_res.resize(off[S]);
    U.ent_job.resize(off[S]); U.ent_slot.resize(off[S]);
    std::vector<u32> cur(U.rn_off.begin(), U.rn_off.end() - 1);
    for (u32 j = 0; j < rn->num_jobs; ++j)  // stable: per slot, input order (cost accumulation order)
      for (u32 a = rn->alloc_offsets[j]; a < rn->alloc_offsets[j + 1]; ++a) {
        const Res r = alloc_row(*rn, a);
        for (auto [q, e] = slots_of(j, rn->alloc_node[a]); q != e; ++q) {
          const u32 d = cur[*q]++;
          U.rn_end[d] = rn->end_sec[j]; U.rn_res[d] = r;
          U.ent_job[d] = j; U.ent_slot[d] = *q;
        }
      }
    U.R = rn->num_jobs;
  }
  out = std::move(U);
  return {};
}

}  // namespace cns_snapshot
