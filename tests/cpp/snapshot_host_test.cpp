// The snapshot layout (cranesched_amd/csrc/snapshot_host.inc: build_layout, build_resv, build_running) against the walk it replaced,
// written out below as it stood in engine.hip — cns_set_nodes, cns_set_reservations, cns_set_running and finalize_layout writing field by
// field into the loose members of the handle (here: struct Old), their uploads kept as plain copies, the build's limits as members so that
// snapshots of a few nodes reach them.  Seeded random snapshots and the hand-made ones at the limits; every field of the three layouts is
// compared exactly, and on a refused input the status and the message.  Two things the old walk did not promise are asserted on their own:
// a refused call leaves its output untouched, and max_np / big_nodes follow the reservations of the LAST call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/crane_gpu/node_select.h"
#include "../../cranesched_amd/csrc/snapshot_host.inc"

namespace sn = cns_snapshot;
using sn::Res;
using sn::i64;
using sn::u32;
using sn::u64;
constexpr u32 kNone = sn::kNone, kTlCap = sn::kTlCap;

static u64 g_s = 0x9E3779B97F4A7C15ull;
static u64 rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
static u32 below(u32 n) { return (u32)(rnd() % n); }
static bool chance(u32 pct) { return below(100) < pct; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_what.c_str()); exit(1); } } while (0)
static std::string g_what;
static std::map<std::string, int> g_seen;   // every message and scenario that was reached

// ===================================================== the walk as it stood ============================================================
struct Old {
  std::string err;
  u32 cap_part = 262144, cap_group = 524288, cap_types = CNS_MAX_NODE_TYPES;   // (kGiantPartSlots, kGiantGroupSlots, CNS_MAX_NODE_TYPES)
  struct { u32 num_classes = 0; u64 class_mask[8] = {}; } gres;
  u32 N = 0, P = 0, S = 0, T = 0, max_np = 0;
  bool big_nodes = false;
  std::vector<u32> part_off, slot_node, orig_pos_slot, node_slot;
  u32 Pu = 0;
  bool shared = false;
  std::vector<u32> upart_eng, upart_size;
  std::vector<uint8_t> refused_probe, upart_refused, upart_tag;
  std::vector<std::vector<u32>> node_slots;
  std::vector<uint8_t> slot_tag;
  bool have_nodes = false, have_jobs = false, have_run = false;
  u32 P_real = 0, S_real = 0, V = 0;
  std::vector<Res> node_total, slot_total;
  std::vector<i64> slot_end, resv_start, resv_end;
  std::vector<std::map<u32, u32>> resv_node_slot;
  std::vector<u32> rv_off;
  std::vector<i64> rv_start, rv_endt;
  std::vector<Res> rv_res;
  bool wide_cores = false;
  std::vector<u32> eng_members, tag_off, tag_base;
  u32 R = 0;
  std::vector<u32> ent_job, ent_slot;
  std::vector<i64> ent_end;
  // what went to the device
  std::vector<u32> d_slot_block, d_sib_off, d_sib, d_part_off, d_slot_node, d_rv_off, d_rn_off, d_tag_base, d_tag_off;
  std::vector<uint8_t> d_type_tag, d_slot_type;
  std::vector<Res> d_slot_total, d_type_total, d_rv_res, d_rn_res;
  std::vector<i64> d_slot_end, d_rv_start, d_rv_end, d_resv_se, d_rn_end;
  u32 width_cap(bool group) const { return group ? cap_group : cap_part; }
};
static int fail(Old* h, int code, const std::string& msg) { h->err = msg; return code; }
template <class T>
static int upload(Old*, std::vector<T>& dst, const std::vector<T>& v) { dst = v; return 0; }

static int finalize_layout(Old* h, const std::vector<Res>* virt_total = nullptr) {
  const u32 S = h->S;
  h->slot_total.resize(S);
  h->slot_end.assign(S, INT64_MAX);
  for (u32 q = 0; q < h->S_real; ++q) h->slot_total[q] = h->node_total[h->slot_node[q]];
  for (u32 q = h->S_real; q < S; ++q) h->slot_total[q] = (*virt_total)[q - h->S_real];
  for (u32 v = 0; v < h->V; ++v)
    for (u32 q = h->part_off[h->P_real + v]; q < h->part_off[h->P_real + v + 1]; ++q) h->slot_end[q] = h->resv_end[v];
  if (h->max_np > h->cap_group)
    return fail(h, CNS_ERR_UNSUPPORTED, "partition with more than " + std::to_string(h->cap_group) + " schedulable (partition, node) slots");
  std::map<std::tuple<i64, u64, u64, u64, u64, u64, u64>, u32> tmap;
  std::vector<Res> type_total;
  std::vector<uint8_t> slot_type(std::max<u32>(S, 1), 0);
  h->slot_tag.resize(S, 0);   // virtual (reservation) slots: tag 0
  for (u32 q = 0; q < S; ++q) {
    const Res& r = h->slot_total[q];
    auto key = std::make_tuple(r.cpu, r.mem, r.clo, r.chi, r.gres, r.c2, r.c3);
    auto it = tmap.find(key);
    if (it == tmap.end()) {
      if (type_total.size() >= h->cap_types)
        return fail(h, CNS_ERR_UNSUPPORTED, "more than 64 distinct res_total records (nodes + reservation shares)");
      it = tmap.emplace(key, (u32)type_total.size()).first;
      type_total.push_back(r);
    }
    slot_type[q] = (uint8_t)it->second;
  }
  h->T = (u32)type_total.size();
  if (h->shared) {
    std::vector<u32> slot_block(S), sib_off(S + 1, 0), sib;
    for (u32 q = 0; q < S; ++q) {
      slot_block[q] = q;
      if (q < h->S_real) {
        const auto& all = h->node_slots[h->slot_node[q]];
        slot_block[q] = all.front();
        for (u32 o : all) if (o != q) sib.push_back(o);
      }
      sib_off[q + 1] = (u32)sib.size();
    }
    if (sib.empty()) sib.push_back(0);
    if (int rc = upload(h, h->d_slot_block, slot_block)) return rc;
    if (int rc = upload(h, h->d_sib_off, sib_off)) return rc;
    if (int rc = upload(h, h->d_sib, sib)) return rc;
    if (int rc = upload(h, h->d_type_tag, h->slot_tag)) return rc;   // per slot: member partition inside the group
  }
  std::vector<i64> resv_se(2 * std::max<u32>(h->V, 1), 0);
  for (u32 v = 0; v < h->V; ++v) { resv_se[2 * v] = h->resv_start[v]; resv_se[2 * v + 1] = h->resv_end[v]; }
  if (int rc = upload(h, h->d_part_off, h->part_off)) return rc;
  if (int rc = upload(h, h->d_slot_node, h->slot_node)) return rc;
  if (int rc = upload(h, h->d_slot_total, h->slot_total)) return rc;
  if (int rc = upload(h, h->d_slot_end, h->slot_end)) return rc;
  if (int rc = upload(h, h->d_slot_type, slot_type)) return rc;
  if (int rc = upload(h, h->d_type_total, type_total)) return rc;
  if (int rc = upload(h, h->d_rv_off, h->rv_off)) return rc;
  {
    std::vector<i64> a = h->rv_start, b = h->rv_endt;
    std::vector<Res> c = h->rv_res;
    if (a.empty()) { a.push_back(0); b.push_back(0); c.push_back(Res{0, 0, 0, 0, 0, 0, 0}); }
    if (int rc = upload(h, h->d_rv_start, a)) return rc;
    if (int rc = upload(h, h->d_rv_end, b)) return rc;
    if (int rc = upload(h, h->d_rv_res, c)) return rc;
  }
  if (int rc = upload(h, h->d_resv_se, resv_se)) return rc;
  if (h->shared) {
    std::vector<u32> tb = h->tag_base, to = h->tag_off;
    tb.resize(std::max<size_t>(h->P, 1), 0);
    for (u32 p = h->P_real; p < h->P; ++p) { tb[p] = (u32)to.size(); to.push_back(0); to.push_back(h->part_off[p + 1] - h->part_off[p]); }
    if (int rc = upload(h, h->d_tag_base, tb)) return rc;
    if (int rc = upload(h, h->d_tag_off, to)) return rc;
  }
  // no running jobs until cns_set_running
  std::vector<u32> rn_off(S + 1, 0);
  if (int rc = upload(h, h->d_rn_off, rn_off)) return rc;
  return 0;
}

static int old_set_nodes(Old* h, const cns_node_soa* nd) {
  if (!h || !nd) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_nodes: null argument");
  if (!nd->cpu_total_raw || !nd->mem_total || !nd->core_lo || !nd->part_offsets || (!nd->part_nodes && nd->part_offsets[nd->num_partitions]))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_set_nodes: missing array");
  if (nd->num_nodes == 0 || nd->num_partitions == 0) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_nodes: empty cluster");
  h->have_nodes = h->have_jobs = h->have_run = false;
  const u32 N = nd->num_nodes;
  u32 P = nd->num_partitions;
  std::vector<Res> total(N);
  u64 all_gres = 0;
  for (u32 c = 0; c < h->gres.num_classes; ++c) all_gres |= h->gres.class_mask[c];
  bool big = false, wide = false;
  for (u32 n = 0; n < N; ++n) {
    total[n].cpu = nd->cpu_total_raw[n];
    total[n].mem = nd->mem_total[n];
    total[n].clo = nd->core_lo[n];
    total[n].chi = nd->core_hi ? nd->core_hi[n] : 0;
    total[n].c2 = nd->core_w2 ? nd->core_w2[n] : 0;
    total[n].c3 = nd->core_w3 ? nd->core_w3[n] : 0;
    if (total[n].c2 | total[n].c3) wide = true;
    total[n].gres = nd->gres_slots ? nd->gres_slots[n] : 0;
    if (total[n].gres & ~all_gres) return fail(h, CNS_ERR_INVALID_ARG, "node GRES slot outside every class");
    if (total[n].gres || total[n].chi) big = true;
  }
  const u32 total_pos = nd->part_offsets[P];
  std::vector<std::vector<std::pair<u32, u32>>> plist(P);  // per caller partition: (node, original position)
  std::vector<u32> uf(P);
  for (u32 p = 0; p < P; ++p) uf[p] = p;
  auto find = [&](u32 x) { while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; } return x; };
  std::vector<u32> first_part(N, kNone);
  bool shared = false;
  std::vector<uint8_t> part_bad(P, 0);
  for (u32 p = 0; p < P; ++p) {
    if (nd->part_offsets[p + 1] < nd->part_offsets[p]) return fail(h, CNS_ERR_INVALID_ARG, "part_offsets not monotone");
    auto& lst = plist[p];
    for (u32 i = nd->part_offsets[p]; i < nd->part_offsets[p + 1]; ++i) {
      u32 n = nd->part_nodes[i];
      if (n >= N) return fail(h, CNS_ERR_INVALID_ARG, "part_nodes entry >= num_nodes");
      if (nd->schedulable && !nd->schedulable[n]) continue;  // JobScheduler.cpp:6595
      if ((nd->unsupported && nd->unsupported[n]) || total[n].cpu <= 0 || total[n].cpu >= 0x7FFFFFFEll) {
        part_bad[p] = (nd->unsupported && nd->unsupported[n]) ? CNS_PART_REFUSED_NODE : CNS_PART_REFUSED_CPU;
        if (first_part[n] == kNone) first_part[n] = p;   // (the partitions that share this node go with it)
        else { u32 a = find(first_part[n]), b = find(p); if (a != b) uf[std::max(a, b)] = std::min(a, b); }
        continue;
      }
      lst.emplace_back(n, i);
    }
    std::sort(lst.begin(), lst.end());
    for (size_t i = 1; i < lst.size(); ++i)
      if (lst[i].first == lst[i - 1].first) return fail(h, CNS_ERR_INVALID_ARG, "node listed twice in one partition");
    for (auto& [n, pos] : lst) {
      if (first_part[n] == kNone) first_part[n] = p;
      else { shared = true; u32 a = find(first_part[n]), b = find(p); if (a != b) uf[std::max(a, b)] = std::min(a, b); }
    }
  }
  std::vector<u32> upart_eng(P), upart_size(P);
  std::vector<uint8_t> upart_tag(P, 0);
  std::vector<std::vector<u32>> members;  // engine partition -> caller partitions, ascending
  {
    std::vector<u32> eng_of_root(P, kNone);
    for (u32 p = 0; p < P; ++p) {
      const u32 r = find(p);
      if (eng_of_root[r] == kNone) { eng_of_root[r] = (u32)members.size(); members.emplace_back(); }
      upart_eng[p] = eng_of_root[r];
      if (members[upart_eng[p]].size() >= 255) return fail(h, CNS_ERR_UNSUPPORTED, "more than 255 partitions connected through shared nodes");
      upart_tag[p] = (uint8_t)members[upart_eng[p]].size();
      members[upart_eng[p]].push_back(p);
      upart_size[p] = (u32)plist[p].size();
    }
  }
  const u32 PE = (u32)members.size();
  std::vector<uint8_t> upart_refused(P, 0);
  {
    std::set<std::tuple<i64, u64, u64, u64, u64, u64, u64>> types;
    for (u32 e = 0; e < PE; ++e) {
      uint8_t why = 0;
      for (u32 p : members[e]) if (part_bad[p] && !why) why = part_bad[p];
      u32 npe = 0;
      for (u32 p : members[e]) npe += (u32)plist[p].size();
      const u32 cap = h->width_cap(members[e].size() > 1);
      if (!why && npe > cap) why = CNS_PART_REFUSED_WIDTH;
      if (!why) {
        auto mine = types;
        for (u32 p : members[e])
          for (auto& [n, pos] : plist[p]) mine.insert(std::make_tuple(total[n].cpu, total[n].mem, total[n].clo, total[n].chi, total[n].gres, total[n].c2, total[n].c3));
        if (mine.size() > h->cap_types) why = CNS_PART_REFUSED_TYPES;
        else types.swap(mine);
      }
      if (why)
        for (u32 p : members[e]) { upart_refused[p] = why; plist[p].clear(); upart_size[p] = 0; }
    }
    bool any_served = false;
    for (u32 p = 0; p < P; ++p) any_served = any_served || !upart_refused[p];
    h->refused_probe = upart_refused;
    if (!any_served) return fail(h, CNS_ERR_UNSUPPORTED, "every partition of the snapshot is outside the engine's limits (a node flagged unsupported, a cpu count outside (0, 2^31-2), more than 64 distinct res_total records, or a group wider than the widest tile)");
  }
  std::vector<u32> part_off(PE + 1, 0), slot_node, node_slot(N, kNone);
  std::vector<std::vector<u32>> node_slots(N);
  std::vector<uint8_t> slot_tag;
  std::vector<u32> orig_pos_slot(total_pos, kNone);
  u32 max_np = 0;
  for (u32 e = 0; e < PE; ++e) {
    part_off[e] = (u32)slot_node.size();
    for (u32 p : members[e])
      for (auto& [n, pos] : plist[p]) {
        const u32 q = (u32)slot_node.size();
        if (node_slot[n] == kNone) node_slot[n] = q;
        node_slots[n].push_back(q);
        orig_pos_slot[pos] = q;
        slot_node.push_back(n);
        slot_tag.push_back(upart_tag[p]);
      }
    max_np = std::max<u32>(max_np, (u32)slot_node.size() - part_off[e]);
  }
  part_off[PE] = (u32)slot_node.size();
  h->tag_off.clear(); h->tag_base.assign(PE, 0);
  for (u32 e = 0; e < PE; ++e) {
    h->tag_base[e] = (u32)h->tag_off.size();
    u32 o = 0;
    for (u32 p : members[e]) { h->tag_off.push_back(o); o += (u32)plist[p].size(); }
    h->tag_off.push_back(o);
  }
  const u32 S = (u32)slot_node.size();
  for (u32 e = 0; e < PE; ++e) {
    const u32 npe = part_off[e + 1] - part_off[e];
    const u32 cap = h->width_cap(members[e].size() > 1);
    if (npe > cap)
      return fail(h, CNS_ERR_UNSUPPORTED, (members[e].size() > 1 ? "group of partitions sharing nodes with more than " : "partition with more than ") +
                                              std::to_string(cap) + " schedulable (partition, node) slots");
  }
  h->Pu = P; h->shared = shared; h->upart_eng = upart_eng; h->upart_size = upart_size; h->upart_tag = upart_tag;
  h->upart_refused = upart_refused;
  h->eng_members.clear();
  for (const auto& m : members) h->eng_members.push_back((u32)m.size());
  h->node_slots = node_slots; h->slot_tag = slot_tag;
  P = PE;
  h->N = N; h->P = P; h->S = S; h->max_np = max_np; h->big_nodes = big || wide; h->wide_cores = wide;
  h->P_real = P; h->S_real = S; h->V = 0;
  h->part_off = part_off; h->slot_node = slot_node; h->node_slot = node_slot; h->orig_pos_slot = orig_pos_slot;
  h->node_total = total;
  h->resv_start.clear(); h->resv_end.clear(); h->resv_node_slot.clear();
  h->rv_off.assign(S + 1, 0); h->rv_start.clear(); h->rv_endt.clear(); h->rv_res.clear();
  if (int rc = finalize_layout(h)) return rc;
  h->have_nodes = true;
  return CNS_OK;
}

static int old_set_reservations(Old* h, const cns_resv_soa* rv) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_reservations: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_set_reservations before cns_set_nodes");
  h->have_jobs = h->have_run = false;
  const u32 V = rv ? rv->num_resv : 0;
  if (V && (!rv->start_sec || !rv->end_sec || !rv->alloc_offsets || !rv->alloc_node || !rv->alloc_cpu_raw ||
            !rv->alloc_mem || !rv->alloc_core_lo))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_set_reservations: missing array");
  h->P = h->P_real; h->S = h->S_real; h->V = V;
  h->part_off.resize(h->P_real + 1);
  h->slot_node.resize(h->S_real);
  h->resv_start.assign(V, 0); h->resv_end.assign(V, 0);
  h->resv_node_slot.assign(V, {});
  std::vector<std::vector<std::tuple<i64, i64, Res>>> per_slot(h->S_real);  // reservation entries of the real slots
  std::vector<Res> virt_total;
  u64 all_gres = 0;
  for (u32 c = 0; c < h->gres.num_classes; ++c) all_gres |= h->gres.class_mask[c];
  for (u32 v = 0; v < V; ++v) {
    h->resv_start[v] = rv->start_sec[v];
    h->resv_end[v] = rv->end_sec[v];
    if (rv->alloc_offsets[v + 1] < rv->alloc_offsets[v]) return fail(h, CNS_ERR_INVALID_ARG, "reservation alloc_offsets not monotone");
    std::vector<std::pair<u32, Res>> al;
    for (u32 a = rv->alloc_offsets[v]; a < rv->alloc_offsets[v + 1]; ++a) {
      const u32 n = rv->alloc_node[a];
      if (n >= h->N) return fail(h, CNS_ERR_INVALID_ARG, "reservation node >= num_nodes");
      Res r;
      r.cpu = rv->alloc_cpu_raw[a]; r.mem = rv->alloc_mem[a]; r.clo = rv->alloc_core_lo[a];
      r.chi = rv->alloc_core_hi ? rv->alloc_core_hi[a] : 0;
      r.c2 = rv->alloc_core_w2 ? rv->alloc_core_w2[a] : 0;
      r.c3 = rv->alloc_core_w3 ? rv->alloc_core_w3[a] : 0;
      r.gres = rv->alloc_gres ? rv->alloc_gres[a] : 0;
      if (r.gres & ~all_gres) return fail(h, CNS_ERR_INVALID_ARG, "reservation GRES slot outside every class");
      if (r.cpu <= 0 || r.cpu >= 0x7FFFFFFEll) return fail(h, CNS_ERR_UNSUPPORTED, "reservation cpu share must be in (0, 2^31-2)");
      al.emplace_back(n, r);
      if (r.gres || r.chi) h->big_nodes = true;
    }
    std::sort(al.begin(), al.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t i = 1; i < al.size(); ++i)
      if (al[i].first == al[i - 1].first) return fail(h, CNS_ERR_INVALID_ARG, "node listed twice in one reservation");
    if (al.size() > h->cap_part) return fail(h, CNS_ERR_UNSUPPORTED, "reservation over more than " + std::to_string(h->cap_part) + " nodes");
    for (auto& [n, r] : al) {
      h->resv_node_slot[v][n] = (u32)h->slot_node.size();  // virtual node: its own NodeState (:6661-6664)
      h->slot_node.push_back(n);
      virt_total.push_back(r);
      for (u32 q : h->node_slots[n]) per_slot[q].emplace_back(rv->start_sec[v], rv->end_sec[v], r);   // every partition's slot of the node
    }
    h->part_off.push_back((u32)h->slot_node.size());
    h->max_np = std::max<u32>(h->max_np, (u32)al.size());
  }
  h->P = h->P_real + V;
  h->S = (u32)h->slot_node.size();
  h->rv_off.assign(h->S + 1, 0); h->rv_start.clear(); h->rv_endt.clear(); h->rv_res.clear();
  for (u32 q = 0; q < h->S_real; ++q) {
    if (per_slot[q].size() > 200) return fail(h, CNS_ERR_UNSUPPORTED, "more than 200 reservations on one node");
    for (auto& [st, en, r] : per_slot[q]) { h->rv_start.push_back(st); h->rv_endt.push_back(en); h->rv_res.push_back(r); }
    h->rv_off[q + 1] = (u32)h->rv_start.size();
  }
  for (u32 q = h->S_real; q < h->S; ++q) h->rv_off[q + 1] = h->rv_off[q];
  if (int rc = finalize_layout(h, &virt_total)) return rc;
  std::vector<u32> rn_off(h->S + 1, 0);
  if (int rc = upload(h, h->d_rn_off, rn_off)) return rc;
  return CNS_OK;
}

static int old_set_running(Old* h, const cns_running_soa* rn) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_running: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_set_running before cns_set_nodes");
  const u32 N = h->N, S = h->S;
  static const std::vector<u32> kNoSlots;
  std::vector<u32> one(1);
  auto slots_of = [&](u32 job, u32 n) -> const std::vector<u32>& {
    const u32 v = rn->reservation ? rn->reservation[job] : CNS_RESV_NONE;
    if (v == CNS_RESV_NONE) return h->node_slots[n];  // empty: unschedulable node, ignored (:6685-6686)
    if (v >= h->V) return kNoSlots;                    // reservation not found (:6693-6700)
    auto it = h->resv_node_slot[v].find(n);
    if (it == h->resv_node_slot[v].end()) return kNoSlots;
    one[0] = it->second;
    return one;
  };
  std::vector<u32> rn_off(S + 1, 0);
  std::vector<i64> rn_end;
  std::vector<Res> rn_res;
  if (rn && rn->num_jobs) {
    if (!rn->end_sec || !rn->alloc_offsets || !rn->alloc_node || !rn->alloc_cpu_raw || !rn->alloc_mem || !rn->alloc_core_lo)
      return fail(h, CNS_ERR_INVALID_ARG, "cns_set_running: missing array");
    const u32 A = rn->alloc_offsets[rn->num_jobs];
    if (A != rn->num_allocs) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_running: num_allocs mismatch");
    for (u32 j = 0; j < rn->num_jobs; ++j)
      for (u32 a = rn->alloc_offsets[j]; a < rn->alloc_offsets[j + 1]; ++a) {
        const u32 n = rn->alloc_node[a];
        if (n >= N) return fail(h, CNS_ERR_INVALID_ARG, "running allocation on node >= num_nodes");
        for (u32 q : slots_of(j, n)) rn_off[q + 1]++;
      }
    for (u32 q = 0; q < S; ++q) {
      const u32 nrv = h->rv_off[q + 1] - h->rv_off[q];
      if (nrv ? rn_off[q + 1] + 2 * nrv + 2 > kTlCap / 2 : rn_off[q + 1] + 2 > kTlCap)
        return fail(h, CNS_ERR_UNSUPPORTED, "too many running allocations / reservations on one node (1006, or 502 events with reservations)");
      rn_off[q + 1] += rn_off[q];
    }
    rn_end.resize(rn_off[S]);
    rn_res.resize(rn_off[S]);
    h->ent_job.assign(rn_off[S], 0);
    h->ent_slot.assign(rn_off[S], 0);
    std::vector<u32> cur(rn_off.begin(), rn_off.end() - 1);
    for (u32 j = 0; j < rn->num_jobs; ++j)  // stable: per slot, input order (cost accumulation order)
      for (u32 a = rn->alloc_offsets[j]; a < rn->alloc_offsets[j + 1]; ++a) {
        Res r;
        r.cpu = rn->alloc_cpu_raw[a];
        r.mem = rn->alloc_mem[a];
        r.clo = rn->alloc_core_lo[a];
        r.chi = rn->alloc_core_hi ? rn->alloc_core_hi[a] : 0;
        r.c2 = rn->alloc_core_w2 ? rn->alloc_core_w2[a] : 0;
        r.c3 = rn->alloc_core_w3 ? rn->alloc_core_w3[a] : 0;
        r.gres = rn->alloc_gres ? rn->alloc_gres[a] : 0;
        for (u32 q : slots_of(j, rn->alloc_node[a])) {
          u32 d = cur[q]++;
          rn_end[d] = rn->end_sec[j];
          rn_res[d] = r;
          h->ent_job[d] = j;
          h->ent_slot[d] = q;
        }
      }
  }
  if (!(rn && rn->num_jobs)) { h->ent_job.clear(); h->ent_slot.clear(); }
  h->R = rn ? rn->num_jobs : 0;
  h->ent_end = rn_end;
  if (int rc = upload(h, h->d_rn_off, rn_off)) return rc;
  if (rn_end.empty()) { rn_end.push_back(0); rn_res.push_back(Res{0, 0, 0, 0, 0, 0, 0}); }
  if (int rc = upload(h, h->d_rn_end, rn_end)) return rc;
  if (int rc = upload(h, h->d_rn_res, rn_res)) return rc;
  h->have_run = false;
  return CNS_OK;
}

// ===================================================== comparing ====================================================================
namespace cns { static bool operator==(const Res& a, const Res& b) { return !memcmp(&a, &b, sizeof(Res)); } }
template <class T>
static std::vector<T> some(std::vector<T> v) { if (v.empty()) v.push_back(T{}); return v; }   // (the old walk uploaded one zero element for an empty table)

#define LAYOUT_FIELDS(X) X(N) X(Pu) X(P_real) X(S_real) X(max_np) X(shared) X(wide_cores) X(big_nodes) X(all_gres) X(part_off) X(slot_node) X(node_slot) \
  X(node_slots) X(slot_tag) X(orig_pos_slot) X(node_total) X(upart_eng) X(upart_size) X(upart_tag) X(upart_refused) X(eng_members) X(tag_off) X(tag_base)
#define RESV_FIELDS(X) X(V) X(P) X(S) X(T) X(max_np) X(big_nodes) X(part_off) X(slot_node) X(slot_total) X(slot_end) X(resv_start) X(resv_end) X(rv_off) \
  X(rv_start) X(rv_endt) X(rv_res) X(slot_type) X(type_total) X(slot_block) X(sib_off) X(sib) X(tag_base) X(tag_off) X(slot_tag)
#define RUN_FIELDS(X) X(R) X(rn_off) X(rn_end) X(rn_res) X(ent_job) X(ent_slot)
#define SAME(f) && a.f == b.f
static bool same(const sn::Layout& a, const sn::Layout& b) {
  return a.caps.part_slots == b.caps.part_slots && a.caps.group_slots == b.caps.group_slots && a.caps.node_types == b.caps.node_types LAYOUT_FIELDS(SAME);
}
static bool same(const sn::ResvLayout& a, const sn::ResvLayout& b) { return true RESV_FIELDS(SAME); }
static bool same(const sn::RunLayout& a, const sn::RunLayout& b) { return true RUN_FIELDS(SAME); }

// the Layout against the handle right after the old cns_set_nodes
static void check_layout(const Old& o, const sn::Layout& L) {
  CHECK(L.N == o.N && L.Pu == o.Pu && L.P_real == o.P_real && L.S_real == o.S_real && L.P_real == o.P && L.S_real == o.S);
  CHECK(L.max_np == o.max_np && L.shared == o.shared && L.wide_cores == o.wide_cores && L.big_nodes == o.big_nodes);
  CHECK(L.part_off == o.part_off && L.slot_node == o.slot_node && L.node_slot == o.node_slot && L.node_slots == o.node_slots);
  CHECK(L.slot_tag == o.slot_tag && L.orig_pos_slot == o.orig_pos_slot && L.node_total == o.node_total);
  CHECK(L.upart_eng == o.upart_eng && L.upart_size == o.upart_size && L.upart_tag == o.upart_tag && L.upart_refused == o.upart_refused);
  CHECK(L.eng_members == o.eng_members && L.tag_off == o.tag_off && L.tag_base == o.tag_base);
}
// the ResvLayout against the handle after the old cns_set_nodes (V == 0) or cns_set_reservations
static void check_resv(const Old& o, const sn::Layout& L, const sn::ResvLayout& X) {
  CHECK(X.V == o.V && X.P == o.P && X.S == o.S && X.T == o.T && X.max_np == o.max_np && X.big_nodes == o.big_nodes);
  CHECK(X.part_off == o.part_off && X.slot_node == o.slot_node && X.slot_total == o.slot_total && X.slot_end == o.slot_end);
  CHECK(X.part_off == o.d_part_off && X.slot_node == o.d_slot_node && X.slot_total == o.d_slot_total && X.slot_end == o.d_slot_end);
  CHECK(X.resv_start == o.resv_start && X.resv_end == o.resv_end);
  CHECK(X.rv_off == o.rv_off && X.rv_start == o.rv_start && X.rv_endt == o.rv_endt && X.rv_res == o.rv_res);
  CHECK(X.rv_off == o.d_rv_off && some(X.rv_start) == o.d_rv_start && some(X.rv_endt) == o.d_rv_end && some(X.rv_res) == o.d_rv_res);
  CHECK(some(X.slot_type) == o.d_slot_type && X.type_total == o.d_type_total);
  for (u32 v = 0; v < X.V + 2; ++v)   // (two unknown reservations behind the last one)
    for (u32 n = 0; n < L.N; ++n) {
      u32 want = kNone;
      if (v < o.V) { auto it = o.resv_node_slot[v].find(n); if (it != o.resv_node_slot[v].end()) want = it->second; }
      CHECK(X.resv_slot(L.P_real, v, n) == want);
    }
  if (L.shared) {
    CHECK(X.slot_block == o.d_slot_block && X.sib_off == o.d_sib_off && some(X.sib) == o.d_sib && X.slot_tag == o.d_type_tag && X.slot_tag == o.slot_tag);
    CHECK(X.tag_base == o.d_tag_base && X.tag_off == o.d_tag_off);
  } else {
    CHECK(X.slot_block.empty() && X.sib_off.empty() && X.sib.empty() && X.slot_tag.empty() && X.tag_base.empty() && X.tag_off.empty());
  }
  CHECK(o.d_rn_off == std::vector<u32>(X.S + 1, 0));
}
static void check_run(const Old& o, const sn::RunLayout& U) {
  CHECK(U.R == o.R && U.rn_off == o.d_rn_off && U.rn_end == o.ent_end && some(U.rn_end) == o.d_rn_end && some(U.rn_res) == o.d_rn_res);
  CHECK(U.ent_job == o.ent_job && U.ent_slot == o.ent_slot);
}

// ===================================================== snapshots ====================================================================
struct Nodes {
  std::vector<i64> cpu;
  std::vector<u64> mem, clo, chi, c2, c3, gres;
  std::vector<uint8_t> sched, unsup;
  std::vector<u32> poff, pnodes;
  u64 all_gres = 0;
  sn::Caps caps{262144, 524288, CNS_MAX_NODE_TYPES};
  bool with_chi = true, with_wide = false, with_gres = true;
  cns_node_soa soa() const {
    cns_node_soa s{};
    s.num_nodes = (u32)cpu.size(); s.num_partitions = (u32)poff.size() - 1;
    s.cpu_total_raw = cpu.data(); s.mem_total = mem.data(); s.core_lo = clo.data();
    s.core_hi = with_chi ? chi.data() : nullptr; s.core_w2 = with_wide ? c2.data() : nullptr; s.core_w3 = with_wide ? c3.data() : nullptr;
    s.gres_slots = with_gres ? gres.data() : nullptr;
    s.schedulable = sched.data(); s.unsupported = unsup.data();
    s.part_offsets = poff.data(); s.part_nodes = pnodes.data();
    return s;
  }
  void resize(u32 N) {
    cpu.assign(N, 8 * 256); mem.assign(N, 1ull << 30); clo.assign(N, 0xFF); chi.assign(N, 0); c2.assign(N, 0); c3.assign(N, 0); gres.assign(N, 0);
    sched.assign(N, 1); unsup.assign(N, 0); poff.assign(1, 0); pnodes.clear();
  }
  void part(std::vector<u32> nodes) { pnodes.insert(pnodes.end(), nodes.begin(), nodes.end()); poff.push_back((u32)pnodes.size()); }
};
struct Allocs {   // a reservation set or a running set
  std::vector<i64> t0, t1, cpu;
  std::vector<u32> off{0}, node, resv;
  std::vector<u64> mem, clo, chi, c2, c3, gres;
  bool with_chi = true, with_wide = true, with_gres = true, with_resv = true;
  u32 num_allocs_delta = 0;
  void add(u32 n, i64 c, u64 g = 0, u64 hi = 0, u64 w2 = 0) {
    node.push_back(n); cpu.push_back(c); mem.push_back(1ull << 20); clo.push_back(1); chi.push_back(hi); c2.push_back(w2); c3.push_back(0); gres.push_back(g);
  }
  void close(i64 a, i64 b, u32 rv = CNS_RESV_NONE) { off.push_back((u32)node.size()); t0.push_back(a); t1.push_back(b); resv.push_back(rv); }
  cns_resv_soa resv_soa() const {
    cns_resv_soa s{};
    s.num_resv = (u32)t0.size(); s.num_allocs = (u32)node.size();
    s.start_sec = t0.data(); s.end_sec = t1.data(); s.alloc_offsets = off.data(); s.alloc_node = node.data(); s.alloc_cpu_raw = cpu.data();
    s.alloc_mem = mem.data(); s.alloc_core_lo = clo.data(); s.alloc_core_hi = with_chi ? chi.data() : nullptr;
    s.alloc_gres = with_gres ? gres.data() : nullptr; s.alloc_core_w2 = with_wide ? c2.data() : nullptr; s.alloc_core_w3 = with_wide ? c3.data() : nullptr;
    return s;
  }
  cns_running_soa run_soa() const {
    cns_running_soa s{};
    s.num_jobs = (u32)t1.size(); s.num_allocs = (u32)node.size() + num_allocs_delta;
    s.end_sec = t1.data(); s.alloc_offsets = off.data(); s.alloc_node = node.data(); s.alloc_cpu_raw = cpu.data();
    s.alloc_mem = mem.data(); s.alloc_core_lo = clo.data(); s.alloc_core_hi = with_chi ? chi.data() : nullptr;
    s.alloc_gres = with_gres ? gres.data() : nullptr; s.reservation = with_resv ? resv.data() : nullptr;
    s.alloc_core_w2 = with_wide ? c2.data() : nullptr; s.alloc_core_w3 = with_wide ? c3.data() : nullptr;
    return s;
  }
};

static Old fresh(const Nodes& nd) {
  Old o;
  o.cap_part = nd.caps.part_slots; o.cap_group = nd.caps.group_slots; o.cap_types = nd.caps.node_types;
  o.gres.num_classes = 1; o.gres.class_mask[0] = nd.all_gres;
  return o;
}
static sn::Layout sentinel_layout() { sn::Layout L; L.N = 0xDEAD; L.part_off = {7, 7, 7}; L.node_slots = {{1}, {2, 3}}; return L; }
static sn::ResvLayout sentinel_resv() { sn::ResvLayout X; X.V = 0xDEAD; X.slot_node = {9, 9}; X.slot_type = {5}; return X; }
static sn::RunLayout sentinel_run() { sn::RunLayout U; U.R = 0xDEAD; U.rn_off = {4, 4}; U.ent_job = {8}; return U; }

// Both walks over one node snapshot.  False: refused by both, with the same status and message.
static bool both_nodes(const Nodes& nd, Old& o, sn::Layout& L, sn::ResvLayout& X, const char* expect = nullptr) {
  const cns_node_soa s = nd.soa();
  o = fresh(nd);
  const int rc = old_set_nodes(&o, &s);
  sn::Layout got = sentinel_layout();
  std::vector<uint8_t> refused{42};
  const sn::Status st = sn::build_layout(&s, nd.all_gres, nd.caps, got, &refused);
  CHECK(st.code == rc);
  if (expect) CHECK(rc != 0 && o.err == expect);
  if (rc != 0) {
    CHECK(st.msg == o.err);
    CHECK(same(got, sentinel_layout()));
    if (o.err.rfind("every partition", 0) == 0) CHECK(refused == o.refused_probe && refused.size() == s.num_partitions);
    else CHECK(refused == std::vector<uint8_t>{42});
    g_seen[o.err]++;
    return false;
  }
  CHECK(refused == o.refused_probe && refused == got.upart_refused);
  check_layout(o, got);
  sn::ResvLayout x = sentinel_resv();
  CHECK(!sn::build_resv(got, nullptr, x));
  check_resv(o, got, x);
  for (uint8_t why : got.upart_refused) if (why) g_seen["status " + std::to_string(why) + " beside a served partition"]++;
  if (got.shared) g_seen["shared"]++; else g_seen["disjoint"]++;
  for (u32 m : got.eng_members) if (m >= 3) g_seen["three or more partitions in one group"]++;
  L = std::move(got); X = std::move(x);
  return true;
}
// ... over one reservation set on top of a node snapshot both accepted (the old handle is a copy: a refused old call leaves it half-written)
static bool both_resv(const Old& o0, const sn::Layout& L, const Allocs& rv, Old& o, sn::ResvLayout& X, const char* expect = nullptr) {
  const cns_resv_soa s = rv.resv_soa();
  o = o0;
  const int rc = old_set_reservations(&o, &s);
  sn::ResvLayout got = sentinel_resv();
  const sn::Status st = sn::build_resv(L, &s, got);
  CHECK(st.code == rc);
  if (expect) CHECK(rc != 0 && o.err == expect);
  if (rc != 0) {
    CHECK(st.msg == o.err);
    CHECK(same(got, sentinel_resv()));
    g_seen[o.err]++;
    return false;
  }
  check_resv(o, L, got);
  X = std::move(got);
  return true;
}
static bool both_run(const Old& o0, const sn::Layout& L, const sn::ResvLayout& X, const Allocs& rn, const char* expect = nullptr) {
  const cns_running_soa s = rn.run_soa();
  Old o = o0;
  const int rc = old_set_running(&o, &s);
  sn::RunLayout got = sentinel_run();
  const sn::Status st = sn::build_running(L, X, &s, got);
  CHECK(st.code == rc);
  if (expect) CHECK(rc != 0 && o.err == expect);
  if (rc != 0) {
    CHECK(st.msg == o.err);
    CHECK(same(got, sentinel_run()));
    g_seen[o.err]++;
    return false;
  }
  check_run(o, got);
  return true;
}

static const u64 kGresBits = 0xFF0Full;
static Nodes random_nodes() {
  Nodes nd;
  const u32 N = 1 + below(64), P = 1 + below(12), mode = below(4);   // 0 disjoint, 1 chains, 2 / 3 random overlap
  nd.resize(N);
  nd.all_gres = kGresBits;
  nd.with_chi = chance(70); nd.with_wide = chance(30); nd.with_gres = chance(70);
  const u32 kinds = chance(20) ? 70 : 1 + below(5);   // (70: more distinct records than the engine carries types)
  for (u32 n = 0; n < N; ++n) {
    const u32 k = below(kinds);
    nd.cpu[n] = (4 + k) * 256; nd.mem[n] = (1ull << 30) + k;
    if (chance(15)) nd.chi[n] = 3;
    if (chance(15)) nd.gres[n] = 0x0F;
    if (chance(10)) nd.c2[n] = 1;
    nd.sched[n] = chance(85);
  }
  if (chance(25)) nd.unsup[below(N)] = 1;
  if (chance(25)) { const i64 bad[] = {0, -256, 0x7FFFFFFEll}; nd.cpu[below(N)] = bad[below(3)]; }
  if (chance(10)) for (u32 n = 0; n < N; ++n) if (chance(60)) nd.unsup[n] = 1;   // (towards: every partition refused)
  if (chance(30)) { nd.caps.part_slots = 1 + below(8); nd.caps.group_slots = nd.caps.part_slots + below(8); }
  if (chance(30)) nd.caps.node_types = 1 + below(4);
  u32 next = 0;
  for (u32 p = 0; p < P; ++p) {
    std::vector<u32> lst;
    if (mode == 0) {
      const u32 take = std::min(N - next, below(N / P + 2));
      for (u32 i = 0; i < take; ++i) lst.push_back(next++);
    } else if (mode == 1) {   // p and p + 1 share a node, every third link is left open
      const u32 take = std::min(N - next, 1 + below(N / P + 1));
      if (p && p % 3 && next) lst.push_back(next - 1);
      for (u32 i = 0; i < take; ++i) lst.push_back(next++);
    } else {
      for (u32 n = 0; n < N; ++n) if (chance(mode == 2 ? 12 : 40)) lst.push_back(n);
    }
    for (size_t i = lst.size(); i > 1; --i) std::swap(lst[i - 1], lst[below((u32)i)]);   // (the caller's order is not ascending)
    nd.part(lst);
  }
  if (nd.pnodes.empty()) nd.pnodes.push_back(0);
  // the INVALID_ARG paths, one at a time
  switch (below(25)) {
    case 0: nd.gres[below(N)] |= 1ull << 40; nd.with_gres = true; break;
    case 1: if (P > 1 && nd.poff[1] > 0) std::swap(nd.poff[0], nd.poff[1]); break;
    case 2: nd.pnodes[below((u32)nd.pnodes.size())] = N + below(3); break;
    case 3: if (nd.poff[1] - nd.poff[0] >= 2) { nd.pnodes[1] = nd.pnodes[0]; } break;
    default: break;
  }
  return nd;
}
static Allocs random_resv(const sn::Layout& L) {
  Allocs rv;
  const u32 V = below(7);
  rv.with_chi = chance(70); rv.with_wide = chance(50); rv.with_gres = chance(70);
  for (u32 v = 0; v < V; ++v) {
    for (u32 n = 0; n < L.N; ++n)
      if (chance(20)) rv.add(n, (1 + below(3)) * 256, chance(20) ? 0x03 : 0, chance(20) ? 1 : 0, chance(15) ? 1 : 0);
    const i64 st = 1000 + below(500);
    rv.close(st, st + 1 + below(500));
  }
  if (rv.node.empty()) return rv;
  const u32 a = below((u32)rv.node.size());
  switch (below(30)) {
    case 0: rv.node[a] = L.N + below(2); break;
    case 1: rv.gres[a] = 1ull << 50; rv.with_gres = true; break;
    case 2: { const i64 bad[] = {0, -1, 0x7FFFFFFEll}; rv.cpu[a] = bad[below(3)]; break; }
    case 3: if (rv.off[1] >= 2) rv.node[1] = rv.node[0]; break;
    case 4: if (V > 1 && rv.off[1] > 0) std::swap(rv.off[0], rv.off[1]); break;
    default: break;
  }
  return rv;
}
static Allocs random_run(const sn::Layout& L, const sn::ResvLayout& X) {
  Allocs rn;
  const u32 R = below(41);
  rn.with_chi = chance(70); rn.with_wide = chance(50); rn.with_gres = chance(70); rn.with_resv = chance(80);
  for (u32 j = 0; j < R; ++j) {
    const u32 k = 1 + below(3);
    u32 v = CNS_RESV_NONE;
    if (chance(40)) v = chance(25) ? X.V + below(3) : (X.V ? below(X.V) : 0);   // an unknown reservation; one that may not list the node
    for (u32 i = 0; i < k; ++i) {
      u32 n = below(L.N);
      if (v < X.V && chance(70) && X.part_off[L.P_real + v + 1] > X.part_off[L.P_real + v])   // a node the reservation does list
        n = X.slot_node[X.part_off[L.P_real + v] + below(X.part_off[L.P_real + v + 1] - X.part_off[L.P_real + v])];
      rn.add(n, 256, chance(20) ? 1 : 0, chance(20) ? 2 : 0, chance(10) ? 4 : 0);
      if (rn.with_resv) {
        if (v == CNS_RESV_NONE && L.node_slots[n].empty()) g_seen["running job on an unschedulable node"]++;
        if (v != CNS_RESV_NONE && v >= X.V) g_seen["running job in an unknown reservation"]++;
        if (v < X.V && X.resv_slot(L.P_real, v, n) == kNone) g_seen["running job in a reservation that does not list the node"]++;
        if (v < X.V && X.resv_slot(L.P_real, v, n) != kNone) g_seen["running job inside a reservation"]++;
      }
    }
    rn.close(0, 2000 + below(1000), v);
  }
  if (R) switch (below(30)) {
    case 0: rn.num_allocs_delta = 1; break;
    case 1: rn.node[below((u32)rn.node.size())] = L.N; break;
    default: break;
  }
  return rn;
}

// ===================================================== the hand-made cases ===========================================================
static void case_type_order() {
  // one type free and two groups that each bring a new record: the group that comes first gets it, the one behind it is refused
  for (int swap = 0; swap < 2; ++swap) {
    Nodes nd; nd.resize(4); nd.caps.node_types = 2;
    nd.cpu = {256, 256, 512, 768};
    nd.part({0, 1});
    nd.part({swap ? 3u : 2u}); nd.part({swap ? 2u : 3u});
    Old o; sn::Layout L; sn::ResvLayout X;
    g_what = "type order";
    CHECK(both_nodes(nd, o, L, X));
    CHECK((L.upart_refused == std::vector<uint8_t>{0, 0, 3}));
    CHECK(X.T == 2 && X.type_total[0].cpu == 256 && X.type_total[1].cpu == (swap ? 768 : 512) && (X.slot_node == std::vector<u32>{0, 1, swap ? 3u : 2u}));
    g_seen["which group gets the last free type"]++;
  }
  {   // a refused group between two served ones: the earlier group keeps its type numbers, the later one continues them
    Nodes nd; nd.resize(5); nd.caps.part_slots = 1; nd.caps.group_slots = 8;
    nd.cpu = {256, 512, 512, 768, 256};
    nd.part({0}); nd.part({1, 2}); nd.part({3});
    Old o; sn::Layout L; sn::ResvLayout X;
    g_what = "width between";
    CHECK(both_nodes(nd, o, L, X));
    CHECK((L.upart_refused == std::vector<uint8_t>{0, 4, 0}) && X.T == 2 && X.type_total[1].cpu == 768 && (X.slot_type == std::vector<uint8_t>{0, 1}));
  }
}
static void case_connected(u32 P, bool ok) {
  Nodes nd; nd.resize(4);
  for (u32 p = 0; p < P; ++p) nd.part({0, 1 + p % 3});
  Old o; sn::Layout L; sn::ResvLayout X;
  g_what = "connected " + std::to_string(P);
  CHECK(both_nodes(nd, o, L, X, ok ? nullptr : "more than 255 partitions connected through shared nodes") == ok);
  if (ok) { CHECK(L.P_real == 1 && L.eng_members[0] == 255 && L.upart_tag[254] == 254 && L.node_slots[0].size() == 255); g_seen["255 partitions connected"]++; }
}
static void case_every_refused() {
  Nodes nd; nd.resize(4); nd.unsup[0] = 1; nd.cpu[2] = 0;
  nd.part({0, 1}); nd.part({2}); nd.part({1, 3});
  Old o; sn::Layout L; sn::ResvLayout X;
  g_what = "every refused";
  CHECK(!both_nodes(nd, o, L, X, "every partition of the snapshot is outside the engine's limits (a node flagged unsupported, a cpu count outside (0, 2^31-2), more than 64 distinct res_total records, or a group wider than the widest tile)"));
  CHECK((o.refused_probe == std::vector<uint8_t>{1, 2, 1}));
  // a refusal touches its connected group and no other
  Nodes n2; n2.resize(5); n2.unsup[0] = 1; n2.cpu[2] = 0x7FFFFFFEll;
  n2.part({0, 1}); n2.part({2}); n2.part({1, 3}); n2.part({4});
  CHECK(both_nodes(n2, o, L, X));
  CHECK((L.upart_refused == std::vector<uint8_t>{1, 2, 1, 0}) && L.S_real == 1);
}
static void case_resv_limits() {
  Nodes nd; nd.resize(3); nd.all_gres = kGresBits;
  nd.sched[2] = 0;
  nd.part({0, 1, 2}); nd.part({1});   // node 1 has two slots
  Old o0; sn::Layout L; sn::ResvLayout X0;
  g_what = "resv limits";
  CHECK(both_nodes(nd, o0, L, X0));
  for (u32 V : {200u, 201u}) {
    Allocs rv;
    for (u32 v = 0; v < V; ++v) { rv.add(1, 256); if (v % 50 == 0) rv.add(2, 256); rv.close(100 + v, 5000 + v); }
    Old o; sn::ResvLayout X;
    CHECK(both_resv(o0, L, rv, o, X, V == 200 ? nullptr : "more than 200 reservations on one node") == (V == 200));
    if (V == 200) {   // entries on every slot of the node
      for (u32 q : L.node_slots[1]) CHECK(X.rv_off[q + 1] - X.rv_off[q] == 200);
      CHECK(L.node_slots[1].size() == 2 && X.rv_off[1] == 0);
      g_seen["200 reservations on a shared node"]++;
    }
  }
  {   // the widest reservation, and the type cap over nodes + reservation shares
    Nodes n2 = nd; n2.caps.part_slots = 2; n2.caps.group_slots = 4; n2.caps.node_types = 2;
    Old p0; sn::Layout L2; sn::ResvLayout Y0;
    CHECK(both_nodes(n2, p0, L2, Y0));
    Allocs wide; wide.add(0, 256); wide.add(2, 256); wide.add(1, 256); wide.close(1, 2);
    Old o; sn::ResvLayout X;
    CHECK(!both_resv(p0, L2, wide, o, X, "reservation over more than 2 nodes"));
    Allocs types; types.add(0, 256); types.add(1, 512); types.close(1, 2);
    CHECK(!both_resv(p0, L2, types, o, X, "more than 64 distinct res_total records (nodes + reservation shares)"));
    Allocs fits; fits.add(0, 256, 0x3, 1, 1); fits.add(2, 256, 0x3, 1, 1); fits.close(1, 2);
    CHECK(both_resv(p0, L2, fits, o, X));
    CHECK(X.T == 2 && X.big_nodes && !L2.big_nodes && X.max_np == 3);
  }
  {   // a missing array
    Allocs rv; rv.add(0, 256); rv.close(1, 2);
    cns_resv_soa s = rv.resv_soa(); s.alloc_mem = nullptr;
    Old o = o0; sn::ResvLayout X = sentinel_resv();
    const int rc = old_set_reservations(&o, &s);
    const sn::Status st = sn::build_resv(L, &s, X);
    CHECK(rc == CNS_ERR_INVALID_ARG && st.code == rc && st.msg == o.err && o.err == "cns_set_reservations: missing array" && same(X, sentinel_resv()));
    g_seen[o.err]++;
  }
}
static void case_run_limits() {
  Nodes nd; nd.resize(2);
  nd.part({0, 1});
  Old o0; sn::Layout L; sn::ResvLayout X0;
  g_what = "run limits";
  CHECK(both_nodes(nd, o0, L, X0));
  Allocs rv; rv.add(1, 256); rv.close(100, 200);
  Old o1; sn::ResvLayout X1;
  CHECK(both_resv(o0, L, rv, o1, X1));
  // (rn + 2 <= kTlCap without reservations on the slot; rn + 2 * nrv + 2 <= kTlCap / 2 with; the reservation's own virtual slot has none)
  struct { u32 node, resv, count; bool ok; } rows[] = {{0, CNS_RESV_NONE, kTlCap - 2, true}, {0, CNS_RESV_NONE, kTlCap - 1, false}, {1, CNS_RESV_NONE, kTlCap / 2 - 4, true},
                                                       {1, CNS_RESV_NONE, kTlCap / 2 - 3, false}, {1, 0, kTlCap - 2, true}, {1, 0, kTlCap - 1, false}};
  for (const auto& r : rows) {
    Allocs rn;
    for (u32 i = 0; i < r.count; ++i) rn.add(r.node, 256);
    rn.close(0, 3000, r.resv);
    CHECK(both_run(o1, L, X1, rn, r.ok ? nullptr : "too many running allocations / reservations on one node (1006, or 502 events with reservations)") == r.ok);
  }
  g_seen["kTlCap with and without reservations"]++;
  {
    Allocs rn; rn.add(0, 256); rn.close(0, 1);
    cns_running_soa s = rn.run_soa(); s.alloc_node = nullptr;
    Old o = o1; sn::RunLayout U = sentinel_run();
    const int rc = old_set_running(&o, &s);
    const sn::Status st = sn::build_running(L, X1, &s, U);
    CHECK(rc == CNS_ERR_INVALID_ARG && st.code == rc && st.msg == o.err && o.err == "cns_set_running: missing array" && same(U, sentinel_run()));
    g_seen[o.err]++;
    // no running set at all: every slot empty, in both walks
    Old e = o1; sn::RunLayout none = sentinel_run();
    CHECK(old_set_running(&e, nullptr) == 0 && !sn::build_running(L, X1, nullptr, none));
    check_run(e, none);
    CHECK(none.R == 0 && none.rn_off == std::vector<u32>(X1.S + 1, 0) && none.ent_job.empty());
  }
}
// THE ONE INTENDED DIFFERENCE from the old walk: max_np and big_nodes follow the reservations of the last call.  The old handle kept the
// widest reservation and the GRES / core flags of every earlier cns_set_reservations until the next cns_set_nodes.
static void case_sticky() {
  Nodes nd; nd.resize(6); nd.all_gres = kGresBits;
  nd.part({0, 1}); nd.part({2});
  Old o; sn::Layout L; sn::ResvLayout X0;
  g_what = "sticky";
  CHECK(both_nodes(nd, o, L, X0));
  CHECK(L.max_np == 2 && !L.big_nodes);
  Allocs wide;
  for (u32 n = 0; n < 6; ++n) wide.add(n, 256, 0x1, 1);
  wide.close(10, 20);
  const cns_resv_soa s = wide.resv_soa();
  sn::ResvLayout X;
  CHECK(old_set_reservations(&o, &s) == 0 && !sn::build_resv(L, &s, X));
  CHECK(X.max_np == 6 && X.big_nodes && o.max_np == 6 && o.big_nodes);
  CHECK(old_set_reservations(&o, nullptr) == 0 && !sn::build_resv(L, nullptr, X));
  CHECK(X.max_np == L.max_np && X.big_nodes == L.big_nodes && X.max_np == 2 && !X.big_nodes);   // the plain layout's
  CHECK(o.max_np == 6 && o.big_nodes);                                                         // (the old walk: still the wide reservation's)
  CHECK(same(X, X0));
}

int main(int argc, char** argv) {
  const u32 cases = argc > 1 ? (u32)atoi(argv[1]) : 3000;
  case_type_order();
  case_connected(255, true);
  case_connected(256, false);
  case_every_refused();
  case_resv_limits();
  case_run_limits();
  case_sticky();
  for (u32 c = 0; c < cases; ++c) {
    g_what = "random case " + std::to_string(c);
    const Nodes nd = random_nodes();
    Old o0; sn::Layout L; sn::ResvLayout X0;
    if (!both_nodes(nd, o0, L, X0)) continue;
    for (u32 n = 0; n < L.N; ++n)
      if (!nd.sched[n])
        for (u32 p = 0; p < L.Pu; ++p)
          if (L.eng_members[L.upart_eng[p]] > 1 && std::find(nd.pnodes.begin() + nd.poff[p], nd.pnodes.begin() + nd.poff[p + 1], n) != nd.pnodes.begin() + nd.poff[p + 1])
            g_seen["unschedulable node inside a shared group"]++;
    for (int round = 0; round < 2; ++round) {
      const Allocs rv = random_resv(L);
      Old o1; sn::ResvLayout X1;
      if (!both_resv(o0, L, rv, o1, X1)) continue;
      for (u32 a = 0; a < rv.node.size(); ++a) {
        if (L.node_slots[rv.node[a]].size() > 1) g_seen["reservation on a shared node"]++;
        if (rv.with_gres && rv.gres[a]) g_seen["reservation with GRES"]++;
        if ((rv.with_chi && rv.chi[a]) || (rv.with_wide && rv.c2[a])) g_seen["reservation with a chi / c2 plane"]++;
      }
      for (int k = 0; k < 2; ++k) both_run(o1, L, X1, random_run(L, X1));
    }
  }
  const char* must[] = {
      "disjoint", "shared", "three or more partitions in one group", "unschedulable node inside a shared group", "status 1 beside a served partition",
      "status 2 beside a served partition", "status 3 beside a served partition", "status 4 beside a served partition", "which group gets the last free type",
      "every partition of the snapshot is outside the engine's limits (a node flagged unsupported, a cpu count outside (0, 2^31-2), more than 64 distinct res_total records, or a group wider than the widest tile)",
      "255 partitions connected", "more than 255 partitions connected through shared nodes", "reservation on a shared node", "200 reservations on a shared node",
      "more than 200 reservations on one node", "reservation with GRES", "reservation with a chi / c2 plane", "running job on an unschedulable node",
      "running job in an unknown reservation", "running job in a reservation that does not list the node", "running job inside a reservation",
      "kTlCap with and without reservations", "too many running allocations / reservations on one node (1006, or 502 events with reservations)",
      // every INVALID_ARG path of the three builders (and the remaining UNSUPPORTED ones)
      "node GRES slot outside every class", "part_offsets not monotone", "part_nodes entry >= num_nodes", "node listed twice in one partition",
      "cns_set_reservations: missing array", "reservation alloc_offsets not monotone", "reservation node >= num_nodes", "reservation GRES slot outside every class",
      "reservation cpu share must be in (0, 2^31-2)", "node listed twice in one reservation", "reservation over more than 2 nodes",
      "more than 64 distinct res_total records (nodes + reservation shares)", "cns_set_running: missing array", "cns_set_running: num_allocs mismatch",
      "running allocation on node >= num_nodes"};
  for (const char* m : must)
    if (!g_seen.count(m)) { printf("FAILED: never reached: %s\n", m); return 1; }
  if (argc > 2) for (const auto& kv : g_seen) printf("%6d  %s\n", kv.second, kv.first.c_str());
  printf("ok\n");
  return 0;
}
