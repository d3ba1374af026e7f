// Multi-GPU inside the product (include/crane_gpu/node_select.h, "several devices"): included by engine.hip.
//
// The reference owns the algorithm through ONE object, built at one place and called once per cycle
// (JobScheduler.cpp:158-159,1441); independent LocalSchedulers per partition are its natural shards (:6723-6732,6746-6761).
// Two forms of the same thing:
//   * cns_group — ONE process drives N devices (what the C++ adapter uses: GpuNodeSelectionAlgo(std::vector<int> devices)): one engine
//     per device, the groups of partitions connected through shared nodes dealt round robin (group g -> device g % N: the plan of
//     cranesched_amd/sharding.py, now here), every device's shard uploaded and run on its own host thread, the packed results
//     all-gathered on the devices, downloaded ONCE from the first device and scattered back into queue order.
//   * cns_comm_* + cns_allgather_results — one process PER device (bench.py under torch.distributed.run): the same all-gather over a
//     communicator the caller bootstraps (rank 0's id shipped by whatever the caller has: MPI, a file, torch's store).
// The collective is RCCL's ncclAllGather (ring over xGMI: per-link bound, one call per cycle, in place) whenever every rank has its own
// device.  RCCL refuses two ranks on one device; a group built over a repeated ordinal ({0, 0}: how the path is tested on a one-GPU box)
// therefore moves the same bytes with device-to-device copies instead and says so (cns_group_info::gather_mode).
#include <thread>

namespace {

#define NCCLCHK_H(h, call)                                                                                   \
  do {                                                                                                       \
    ncclResult_t _r = (call);                                                                                \
    if (_r != ncclSuccess) return fail(h, CNS_ERR_HIP, std::string(#call) + ": " + ncclGetErrorString(_r)); \
  } while (0)

}  // namespace

struct cns_group {
  std::vector<cns_engine*> eng;
  std::vector<int> devices;
  bool distinct = true;              // every engine on its own device -> RCCL; else device-to-device copies
  std::vector<ncclComm_t> comms;
  std::string err;
  // the plan of the current snapshot
  u32 P = 0, N = 0, V = 0;
  std::vector<u32> part_dev, part_local;       // caller's partition -> device, -> its index in that device's snapshot
  std::vector<std::vector<u32>> dev_parts;     // device -> caller's partitions, ascending
  std::vector<u32> active;                     // devices that own a partition they can serve (more devices than groups of partitions: the others idle;
                                               // a device whose whole share is outside the engine's limits serves nothing: part_status)
  std::vector<uint8_t> part_status;            // caller's partition -> cns_partition_status (cns_group_get_partition_status)
  u64 batch = 0;                               // cns_config::scheduled_batch_size: applied ONCE over the whole queue (the engines run without one)
  // per-device job shards of the last cycle
  struct Shard {
    std::vector<u64> idx;                      // shard job -> queue index
    std::vector<u32> partition, node_num, ntasks, tmin, tmax, incl_nodes, excl_nodes, reservation;
    std::vector<i64> time_limit, node_cpu, task_cpu;
    std::vector<u64> node_mem, task_mem, incl_off, excl_off;
    std::vector<uint8_t> exclusive, gres_total, gres_spec, skip;
    int status = 0;
    double upload_ms = 0, run_ms = 0;
  };
  std::vector<Shard> shard;
  std::vector<DevBuf> d_gather;                // device d: N x slot bytes
  void* h_gather = nullptr;                    // page-locked host copy of the first device's gathered buffer
  size_t h_gather_cap = 0;
  cns_group_info info{};
};

namespace {

int gfail(cns_group* g, int code, const std::string& msg) {
  if (g) g->err = msg; else g_create_error = msg;
  return code;
}

// partitions connected through shared nodes (the union-find of cns_set_nodes / sharding.partition_groups): groups ascending by first member
std::vector<std::vector<u32>> partition_groups(const cns_node_soa* nd) {
  const u32 P = nd->num_partitions;
  std::vector<u32> uf(P);
  for (u32 p = 0; p < P; ++p) uf[p] = p;
  auto find = [&](u32 x) { while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; } return x; };
  std::vector<u32> first(nd->num_nodes, kNone);
  for (u32 p = 0; p < P; ++p)
    for (u32 x = nd->part_offsets[p]; x < nd->part_offsets[p + 1]; ++x) {
      const u32 n = nd->part_nodes[x];
      if (n >= nd->num_nodes) continue;   // (cns_set_nodes reports it)
      if (first[n] == kNone) first[n] = p;
      else { const u32 a = find(first[n]), b = find(p); if (a != b) uf[std::max(a, b)] = std::min(a, b); }
    }
  std::map<u32, std::vector<u32>> groups;
  for (u32 p = 0; p < P; ++p) groups[find(p)].push_back(p);
  std::vector<std::vector<u32>> out;
  for (auto& kv : groups) out.push_back(kv.second);
  return out;
}

}  // namespace

extern "C" {

int cns_comm_unique_id(uint8_t* id) {
  if (!id) return fail(nullptr, CNS_ERR_INVALID_ARG, "cns_comm_unique_id: null argument");
  static_assert(sizeof(ncclUniqueId) <= CNS_COMM_ID_BYTES, "ncclUniqueId fits the ABI's id");
  ncclUniqueId u;
  NCCLCHK_H(nullptr, ncclGetUniqueId(&u));
  memset(id, 0, CNS_COMM_ID_BYTES);
  memcpy(id, &u, sizeof u);
  return CNS_OK;
}

int cns_comm_init_rank(cns_handle* h, uint32_t nranks, uint32_t rank, const uint8_t* id) {
  if (!h || !id || nranks == 0 || rank >= nranks) return fail(h, CNS_ERR_INVALID_ARG, "cns_comm_init_rank: bad argument");
  if (h->comm) { (void)ncclCommDestroy((ncclComm_t)h->comm); h->comm = nullptr; }
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  ncclComm_t c = nullptr;
  NCCLCHK_H(h, ncclCommInitRank(&c, (int)nranks, u, (int)rank));
  h->comm = c; h->comm_nranks = nranks; h->comm_rank = rank;
  return CNS_OK;
}

int cns_comm_destroy(cns_handle* h) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_comm_destroy: null handle");
  if (h->comm) { (void)ncclCommDestroy((ncclComm_t)h->comm); h->comm = nullptr; }
  h->comm_nranks = 0; h->comm_rank = 0;
  return CNS_OK;
}

int cns_results_layout(const cns_handle* h, cns_results_offsets* out) {
  if (!h || !out) return fail(const_cast<cns_handle*>(h), CNS_ERR_INVALID_ARG, "cns_results_layout: null argument");
  if (!h->have_jobs) return fail(const_cast<cns_handle*>(h), CNS_ERR_STATE, "cns_results_layout before cns_upload_jobs");
  out->num_jobs = h->q.J; out->num_places = h->q.places; out->wide_cores = h->lay.wide_cores ? 1u : 0u;
  out->start_sec = h->q.ro.start; out->cpu_raw = h->q.ro.cpu; out->mem = h->q.ro.mem; out->core_lo = h->q.ro.clo; out->core_hi = h->q.ro.chi;
  out->gres = h->q.ro.gres; out->node_idx = h->q.ro.node; out->ntasks = h->q.ro.ntasks; out->reason = h->q.ro.reason;
  out->core_w2 = h->q.ro.c2; out->core_w3 = h->q.ro.c3; out->total_bytes = h->q.ro.total;
  return CNS_OK;
}

// every rank's packed results, padded to slot_bytes, rank r at [r * slot_bytes): ONE in-place ncclAllGather on the engine's stream
int cns_allgather_results(cns_handle* h, uint64_t slot_bytes, void** gathered) {
  if (!h || !gathered) return fail(h, CNS_ERR_INVALID_ARG, "cns_allgather_results: null argument");
  if (!h->comm) return fail(h, CNS_ERR_STATE, "cns_allgather_results before cns_comm_init_rank");
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_allgather_results before a successful run");
  if (slot_bytes < h->q.ro.total || (slot_bytes & 15u)) return fail(h, CNS_ERR_INVALID_ARG, "cns_allgather_results: slot_bytes below this rank's results, or not a multiple of 16");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_gather.ensure((size_t)slot_bytes * h->comm_nranks));
  char* mine = h->d_gather.as<char>() + (size_t)slot_bytes * h->comm_rank;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  HIPCHK(h, hipMemcpyAsync(mine, h->q.results.p, h->q.ro.total, hipMemcpyDeviceToDevice, h->stream));
  NCCLCHK_H(h, ncclAllGather(mine, h->d_gather.p, (size_t)slot_bytes, ncclUint8, (ncclComm_t)h->comm, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->gather_ms = ms;
  h->gather_bytes = (u64)slot_bytes * h->comm_nranks;
  *gathered = h->d_gather.p;
  return CNS_OK;
}

int cns_download_gathered(cns_handle* h, void* dst, uint64_t bytes) {
  if (!h || !dst) return fail(h, CNS_ERR_INVALID_ARG, "cns_download_gathered: null argument");
  if (!h->d_gather.p || bytes > h->gather_bytes) return fail(h, CNS_ERR_STATE, "cns_download_gathered: nothing gathered, or more bytes than were gathered");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(dst, h->d_gather.p, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return CNS_OK;
}

int cns_gather_timing(const cns_handle* h, double* ms, uint64_t* bytes) {
  if (!h) return CNS_ERR_INVALID_ARG;
  if (ms) *ms = h->gather_ms;
  if (bytes) *bytes = h->gather_bytes;
  return CNS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// cns_group
// ---------------------------------------------------------------------------------------------------------------------
const char* cns_group_last_error(const cns_group* g) { return g ? g->err.c_str() : g_create_error.c_str(); }

void cns_group_destroy(cns_group* g) {
  if (!g) return;
  for (ncclComm_t c : g->comms) if (c) (void)ncclCommDestroy(c);
  for (size_t d = 0; d < g->eng.size(); ++d) {
    if (g->eng[d]) { (void)hipSetDevice(g->eng[d]->device); g->d_gather[d].release(); cns_destroy(g->eng[d]); }
  }
  if (g->h_gather) (void)hipHostFree(g->h_gather);
  delete g;
}

int cns_group_create(const cns_config* cfg, const int32_t* devices, uint32_t n, cns_group** out) {
  if (!cfg || !devices || n == 0 || !out) return gfail(nullptr, CNS_ERR_INVALID_ARG, "cns_group_create: null argument or no device");
  *out = nullptr;
  cns_group* g = new (std::nothrow) cns_group;
  if (!g) return gfail(nullptr, CNS_ERR_HIP, "cns_group_create: out of memory");
  g->eng.assign(n, nullptr); g->d_gather = std::vector<DevBuf>(n); g->shard.resize(n);
  g->devices.assign(devices, devices + n);
  std::set<int> seen(g->devices.begin(), g->devices.end());
  g->distinct = seen.size() == n;
  for (uint32_t d = 0; d < n; ++d) {
    cns_config c = *cfg;
    c.device = devices[d];
    // BasicPriority::GetOrderedJobPtrVec (JobScheduler.h:185-200) cuts the ONE ordered queue at ScheduledBatchSize; an engine that applied the
    // limit to its shard would let up to N x limit jobs through: cns_group_select cuts the queue before it deals it
    c.scheduled_batch_size = 0;
    const int st = cns_create(&c, &g->eng[d]);
    if (st != 0) { const std::string e = cns_last_error(nullptr); cns_group_destroy(g); return gfail(nullptr, st, "cns_group_create: device " + std::to_string(devices[d]) + ": " + e); }
  }
  if (g->distinct) {   // one communicator per engine, all in this process (ncclCommInitAll)
    g->comms.assign(n, nullptr);
    const ncclResult_t r = ncclCommInitAll(g->comms.data(), (int)n, g->devices.data());
    if (r != ncclSuccess) { const std::string e = ncclGetErrorString(r); g->comms.clear(); cns_group_destroy(g); return gfail(nullptr, CNS_ERR_HIP, "cns_group_create: ncclCommInitAll: " + e); }
  }
  memset(&g->info, 0, sizeof g->info);
  g->info.num_devices = n;
  g->info.gather_mode = g->distinct ? CNS_GATHER_RCCL : CNS_GATHER_DEVICE_COPIES;
  g->batch = cfg->scheduled_batch_size;
  *out = g;
  return CNS_OK;
}

uint32_t cns_group_size(const cns_group* g) { return g ? (uint32_t)g->eng.size() : 0u; }
cns_handle* cns_group_handle(cns_group* g, uint32_t d) { return (g && d < g->eng.size()) ? g->eng[d] : nullptr; }

int cns_group_set_nodes(cns_group* g, const cns_node_soa* nd) {
  if (!g || !nd || !nd->part_offsets || (!nd->part_nodes && nd->part_offsets[nd->num_partitions] != 0))
    return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_set_nodes: null argument");
  const u32 n = (u32)g->eng.size(), P = nd->num_partitions;
  const auto groups = partition_groups(nd);
  g->P = P; g->N = nd->num_nodes;
  g->part_dev.assign(P, 0); g->part_local.assign(P, 0);
  g->dev_parts.assign(n, {});
  for (size_t gi = 0; gi < groups.size(); ++gi)
    for (u32 p : groups[gi]) { g->part_dev[p] = (u32)(gi % n); g->dev_parts[gi % n].push_back(p); }
  g->active.clear();
  g->part_status.assign(P, CNS_PART_SERVED);
  for (u32 d = 0; d < n; ++d) {
    if (g->dev_parts[d].empty()) continue;   // (fewer groups than devices: nothing to run there)
    std::sort(g->dev_parts[d].begin(), g->dev_parts[d].end());
    // the device's snapshot: every node (indices stay global: placements need no translation), only its partitions, renumbered
    std::vector<u32> po(1, 0), pn;
    for (size_t l = 0; l < g->dev_parts[d].size(); ++l) {
      const u32 p = g->dev_parts[d][l];
      g->part_local[p] = (u32)l;
      pn.insert(pn.end(), nd->part_nodes + nd->part_offsets[p], nd->part_nodes + nd->part_offsets[p + 1]);
      po.push_back((u32)pn.size());
    }
    if (pn.empty()) pn.push_back(0);
    cns_node_soa sub = *nd;
    sub.num_partitions = (u32)g->dev_parts[d].size();
    sub.part_offsets = po.data(); sub.part_nodes = pn.data();
    const int st = cns_set_nodes(g->eng[d], &sub);
    if (st == CNS_ERR_UNSUPPORTED && g->eng[d]->refused_probe.size() == g->dev_parts[d].size()) {
      // EVERY partition dealt to this device is outside the engine's limits.  On one device the same snapshot serves the other partitions and
      // refuses these (CNS_REASON_ENGINE_REFUSED): so here — the device serves nothing this cycle, its jobs go back to the caller's CPU scheduler
      for (size_t l = 0; l < g->dev_parts[d].size(); ++l) g->part_status[g->dev_parts[d][l]] = g->eng[d]->refused_probe[l];
      continue;
    }
    if (st != 0) return gfail(g, st, "device " + std::to_string(g->devices[d]) + ": " + cns_last_error(g->eng[d]));
    g->active.push_back(d);
    for (size_t l = 0; l < g->dev_parts[d].size(); ++l) g->part_status[g->dev_parts[d][l]] = g->eng[d]->lay.upart_refused[l];
  }
  g->V = 0;
  if (g->active.empty()) return gfail(g, CNS_ERR_UNSUPPORTED, "every partition of the snapshot is outside the engine's limits on every device");
  return CNS_OK;
}

int cns_group_set_reservations(cns_group* g, const cns_resv_soa* rv) {
  if (!g) return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_set_reservations: null group");
  // every device gets every reservation (a reservation carves its share out of the real nodes' time maps whichever partition lists
  // them); the jobs submitted TO reservation v run on device v % N (cns_group_select)
  for (u32 d : g->active) {
    const int st = cns_set_reservations(g->eng[d], rv);
    if (st != 0) return gfail(g, st, "device " + std::to_string(g->devices[d]) + ": " + cns_last_error(g->eng[d]));
  }
  g->V = rv ? rv->num_resv : 0;
  return CNS_OK;
}

int cns_group_set_running(cns_group* g, const cns_running_soa* rn) {
  if (!g) return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_set_running: null group");
  // every device gets the whole running set, in its order (the initial fp64 cost is accumulated in this order, JobScheduler.h:508-510):
  // allocations on nodes none of the device's partitions lists have no slot there and are dropped by cns_set_running itself
  for (u32 d : g->active) {
    const int st = cns_set_running(g->eng[d], rn);
    if (st != 0) return gfail(g, st, "device " + std::to_string(g->devices[d]) + ": " + cns_last_error(g->eng[d]));
  }
  return CNS_OK;
}

int cns_group_select(cns_group* g, int64_t now, const cns_job_soa* jb, cns_placement_soa* out) {
  if (!g || !jb || !out) return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_select: null argument");
  if (!out->start_sec || !out->reason || !out->place_offsets || !out->node_idx || !out->ntasks || !out->cpu_raw || !out->mem ||
      !out->core_lo || !out->core_hi || !out->gres)
    return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_select: missing result array");
  const u32 n = (u32)g->eng.size(), na = (u32)g->active.size();
  if (na == 0) return gfail(g, CNS_ERR_STATE, "cns_group_select before cns_group_set_nodes");
  const u64 J = jb->num_jobs;
  const auto t0 = std::chrono::steady_clock::now();
  // ---- deal the queue: job -> the device of its partition (of its reservation), order preserved ---------------------------------
  // (an empty queue may come with null job arrays — an adapter's never-filled vectors — as cns_select accepts them: every device then
  // runs an empty shard, exactly as one engine runs an empty queue, and the result is all empty)
  if (J && (!jb->partition || !jb->node_num || !jb->ntasks || !jb->ntasks_per_node_min || !jb->ntasks_per_node_max || !jb->time_limit_sec || !jb->node_mem ||
            !jb->task_cpu_raw || !jb->task_mem || (jb->incl_offsets && !jb->incl_nodes && jb->incl_offsets[J] != 0) ||
            (jb->excl_offsets && !jb->excl_nodes && jb->excl_offsets[J] != 0)))
    return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_select: a required job array is missing (or node-list offsets without the lists)");
  for (auto& s : g->shard) s = cns_group::Shard{};
  std::vector<u32> jdev;
  try { jdev.resize(J); } catch (...) { return gfail(g, CNS_ERR_HIP, "cns_group_select: out of memory"); }
  constexpr u32 kDevBatch = 0xFFFFFFFFu, kDevRefused = 0xFFFFFFFEu;   // decided here: behind the batch limit | a partition no device serves
  const u64 batch = g->batch ? std::min<u64>(g->batch, J) : J;      // BasicPriority: the first min(J, limit) jobs of the ordered queue
  std::vector<uint8_t> dev_active(n, 0);
  for (u32 d : g->active) dev_active[d] = 1;
  u64 places = 0;
  for (u64 j = 0; j < J; ++j) {
    const u32 rv = jb->reservation ? jb->reservation[j] : CNS_RESV_NONE;
    const u32 p = jb->partition[j];
    u32 d;
    if (j >= batch) d = kDevBatch;
    else if (rv != CNS_RESV_NONE) d = g->active[rv % na];         // (an unknown reservation: any device reports "Reservation Not Found")
    else if (p >= g->P) d = g->active[j % na];                    // (an unknown partition: any device reports "Partition Not Found")
    else d = dev_active[g->part_dev[p]] ? g->part_dev[p] : ((jb->skip && jb->skip[j]) ? g->active[j % na] : kDevRefused);   // (a skipped job keeps its own reason)
    jdev[j] = d;
    places += jb->node_num[j];
  }
  if (out->place_capacity < places) return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_select: place_capacity too small");
  out->place_offsets[0] = 0;
  for (u64 j = 0; j < J; ++j) out->place_offsets[j + 1] = out->place_offsets[j] + jb->node_num[j];
  auto pack = [&](u32 d) {
    cns_group::Shard& s = g->shard[d];
    for (u64 j = 0; j < J; ++j) if (jdev[j] == d) s.idx.push_back(j);
    const size_t m = s.idx.size();
    s.partition.resize(m); s.time_limit.resize(m); s.node_mem.resize(m); s.task_cpu.resize(m); s.task_mem.resize(m);
    s.node_num.resize(m); s.ntasks.resize(m); s.tmin.resize(m); s.tmax.resize(m);
    if (jb->node_cpu_raw) s.node_cpu.resize(m);
    if (jb->exclusive) s.exclusive.resize(m);
    if (jb->gres_total) s.gres_total.resize(m * CNS_MAX_GRES_NAMES);
    if (jb->gres_spec) s.gres_spec.resize(m * CNS_MAX_GRES_CLASSES);
    if (jb->skip) s.skip.resize(m);
    if (jb->reservation) s.reservation.resize(m);
    if (jb->incl_offsets) s.incl_off.assign(m + 1, 0);
    if (jb->excl_offsets) s.excl_off.assign(m + 1, 0);
    for (size_t x = 0; x < m; ++x) {
      const u64 j = s.idx[x];
      const u32 p = jb->partition[j];
      s.partition[x] = p < g->P ? g->part_local[p] : 0xFFFFFFFFu;   // (renumbered with the device's snapshot; unknown stays unknown)
      s.time_limit[x] = jb->time_limit_sec[j]; s.node_mem[x] = jb->node_mem[j];
      s.task_cpu[x] = jb->task_cpu_raw[j]; s.task_mem[x] = jb->task_mem[j];
      s.node_num[x] = jb->node_num[j]; s.ntasks[x] = jb->ntasks[j];
      s.tmin[x] = jb->ntasks_per_node_min[j]; s.tmax[x] = jb->ntasks_per_node_max[j];
      if (jb->node_cpu_raw) s.node_cpu[x] = jb->node_cpu_raw[j];
      if (jb->exclusive) s.exclusive[x] = jb->exclusive[j];
      if (jb->gres_total) memcpy(&s.gres_total[x * CNS_MAX_GRES_NAMES], jb->gres_total + j * CNS_MAX_GRES_NAMES, CNS_MAX_GRES_NAMES);
      if (jb->gres_spec) memcpy(&s.gres_spec[x * CNS_MAX_GRES_CLASSES], jb->gres_spec + j * CNS_MAX_GRES_CLASSES, CNS_MAX_GRES_CLASSES);
      if (jb->skip) s.skip[x] = jb->skip[j];
      if (jb->reservation) s.reservation[x] = jb->reservation[j];
      if (jb->incl_offsets) {
        s.incl_nodes.insert(s.incl_nodes.end(), jb->incl_nodes + jb->incl_offsets[j], jb->incl_nodes + jb->incl_offsets[j + 1]);
        s.incl_off[x + 1] = s.incl_nodes.size();
      }
      if (jb->excl_offsets) {
        s.excl_nodes.insert(s.excl_nodes.end(), jb->excl_nodes + jb->excl_offsets[j], jb->excl_nodes + jb->excl_offsets[j + 1]);
        s.excl_off[x + 1] = s.excl_nodes.size();
      }
    }
    if (s.incl_nodes.empty()) s.incl_nodes.push_back(0);
    if (s.excl_nodes.empty()) s.excl_nodes.push_back(0);
  };
  // ---- every device: pack its shard, upload, run — on its own host thread ------------------------------------------------------------
  std::vector<uint8_t> is_active(n, 0);
  for (u32 d : g->active) is_active[d] = 1;
  auto work = [&](u32 d) {
    cns_group::Shard& s = g->shard[d];
    if (!is_active[d]) return;
    pack(d);
    cns_job_soa js{};
    js.num_jobs = s.idx.size();
    js.partition = s.partition.data(); js.time_limit_sec = s.time_limit.data(); js.node_cpu_raw = jb->node_cpu_raw ? s.node_cpu.data() : nullptr;
    js.node_mem = s.node_mem.data(); js.task_cpu_raw = s.task_cpu.data(); js.task_mem = s.task_mem.data(); js.node_num = s.node_num.data();
    js.ntasks = s.ntasks.data(); js.ntasks_per_node_min = s.tmin.data(); js.ntasks_per_node_max = s.tmax.data();
    js.exclusive = jb->exclusive ? s.exclusive.data() : nullptr;
    js.gres_total = jb->gres_total ? s.gres_total.data() : nullptr; js.gres_spec = jb->gres_spec ? s.gres_spec.data() : nullptr;
    js.incl_offsets = jb->incl_offsets ? s.incl_off.data() : nullptr; js.incl_nodes = s.incl_nodes.data();
    js.excl_offsets = jb->excl_offsets ? s.excl_off.data() : nullptr; js.excl_nodes = s.excl_nodes.data();
    js.skip = jb->skip ? s.skip.data() : nullptr; js.reservation = jb->reservation ? s.reservation.data() : nullptr;
    const auto a = std::chrono::steady_clock::now();
    s.status = cns_upload_jobs(g->eng[d], &js);
    const auto b = std::chrono::steady_clock::now();
    if (s.status == 0) s.status = cns_run_resident(g->eng[d], now);
    const auto c = std::chrono::steady_clock::now();
    s.upload_ms = std::chrono::duration<double, std::milli>(b - a).count();
    s.run_ms = std::chrono::duration<double, std::milli>(c - b).count();
  };
  // (nothing throws through the C ABI: a worker that runs out of memory reports it as its shard's status; a thread that cannot be
  // started leaves its device — and the ones behind it — to the calling thread)
  auto guarded = [&](auto&& f, u32 d) {
    try { f(d); } catch (...) { g->shard[d].status = CNS_ERR_HIP; }
  };
  auto on_threads = [&](auto&& f) {
    std::vector<std::thread> th;
    u32 started = 1;
    try {
      th.reserve(n);
      for (; started < n; ++started) th.emplace_back([&, d = started] { guarded(f, d); });
    } catch (...) {
    }
    guarded(f, 0);
    for (u32 d = started; d < n; ++d) guarded(f, d);
    for (auto& t : th) t.join();
  };
  on_threads(work);
  for (u32 d = 0; d < n; ++d)
    if (g->shard[d].status != 0) return gfail(g, g->shard[d].status, "device " + std::to_string(g->devices[d]) + ": " + cns_last_error(g->eng[d]));
  const auto t1 = std::chrono::steady_clock::now();
  // ---- all-gather of the packed results on the devices: rank d's buffer at [d * slot) of every device's gather buffer -------------------
  size_t slot = 16;
  std::vector<size_t> rbytes(n, 0);   // (an idle device contributes an empty slot)
  for (u32 d : g->active) { rbytes[d] = g->eng[d]->q.ro.total; slot = std::max(slot, align16(rbytes[d])); }
  for (u32 d = 0; d < n; ++d) {
    cns_engine* h = g->eng[d];
    if (hipSetDevice(h->device) != hipSuccess || g->d_gather[d].ensure(slot * n) != hipSuccess) return gfail(g, CNS_ERR_HIP, "cns_group_select: gather buffer allocation failed");
    if (rbytes[d] && hipMemcpyAsync(g->d_gather[d].as<char>() + slot * d, h->q.results.p, rbytes[d], hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      return gfail(g, CNS_ERR_HIP, "cns_group_select: staging copy failed");
  }
  if (g->distinct) {
    ncclResult_t r = ncclGroupStart();
    for (u32 d = 0; d < n && r == ncclSuccess; ++d)
      r = ncclAllGather(g->d_gather[d].as<char>() + slot * d, g->d_gather[d].p, slot, ncclUint8, g->comms[d], g->eng[d]->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess) return gfail(g, CNS_ERR_HIP, std::string("cns_group_select: ncclAllGather: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
  } else {   // (a repeated device ordinal: RCCL refuses two ranks on one device — the same bytes by device-to-device copies)
    for (u32 d = 0; d < n; ++d) if (hipSetDevice(g->eng[d]->device) != hipSuccess || hipStreamSynchronize(g->eng[d]->stream) != hipSuccess) return gfail(g, CNS_ERR_HIP, "cns_group_select: stream sync failed");
    for (u32 dst = 0; dst < n; ++dst)
      for (u32 src = 0; src < n; ++src) {
        if (src == dst || !rbytes[src]) continue;
        if (hipMemcpyPeerAsync(g->d_gather[dst].as<char>() + slot * src, g->eng[dst]->device, g->eng[src]->q.results.p, g->eng[src]->device,
                               rbytes[src], g->eng[dst]->stream) != hipSuccess)
          return gfail(g, CNS_ERR_HIP, "cns_group_select: device-to-device copy failed");
      }
  }
  for (u32 d = 0; d < n; ++d)
    if (hipSetDevice(g->eng[d]->device) != hipSuccess || hipStreamSynchronize(g->eng[d]->stream) != hipSuccess) return gfail(g, CNS_ERR_HIP, "cns_group_select: all-gather did not complete");
  const auto t2 = std::chrono::steady_clock::now();
  // ---- ONE download (the first device holds everything) and the scatter back into queue order --------------------------------------------
  if (g->h_gather_cap < slot * n) {
    if (g->h_gather) (void)hipHostFree(g->h_gather);
    g->h_gather = nullptr; g->h_gather_cap = 0;
    if (hipHostMalloc(&g->h_gather, slot * n, hipHostMallocDefault) != hipSuccess) return gfail(g, CNS_ERR_HIP, "cns_group_select: host buffer allocation failed");
    g->h_gather_cap = slot * n;
  }
  {
    cns_engine* h0 = g->eng[0];
    if (hipSetDevice(h0->device) != hipSuccess || hipMemcpyAsync(g->h_gather, g->d_gather[0].p, slot * n, hipMemcpyDeviceToHost, h0->stream) != hipSuccess ||
        hipStreamSynchronize(h0->stream) != hipSuccess)
      return gfail(g, CNS_ERR_HIP, "cns_group_select: download of the gathered results failed");
  }
  const auto t3 = std::chrono::steady_clock::now();
  bool any_wide = false;
  for (u32 d : g->active) any_wide = any_wide || g->eng[d]->lay.wide_cores;
  if (any_wide && (!out->core_w2 || !out->core_w3)) return gfail(g, CNS_ERR_INVALID_ARG, "cns_group_select: the snapshot has nodes with core ids above 127: core_w2 / core_w3 are required");
  auto scatter = [&](u32 d) {
    if (!is_active[d]) return;
    const cns_engine* h = g->eng[d];
    const cns_group::Shard& s = g->shard[d];
    const char* rb = (const char*)g->h_gather + slot * d;
    const i64* st = (const i64*)(rb + h->q.ro.start);
    const uint8_t* rs = (const uint8_t*)(rb + h->q.ro.reason);
    const i64* cpu = (const i64*)(rb + h->q.ro.cpu);
    const u64 *mem = (const u64*)(rb + h->q.ro.mem), *lo = (const u64*)(rb + h->q.ro.clo), *hi = (const u64*)(rb + h->q.ro.chi), *gr = (const u64*)(rb + h->q.ro.gres);
    const u64 *w2 = (const u64*)(rb + h->q.ro.c2), *w3 = (const u64*)(rb + h->q.ro.c3);
    const u32 *nd = (const u32*)(rb + h->q.ro.node), *nt = (const u32*)(rb + h->q.ro.ntasks);
    u64 src = 0;
    for (size_t x = 0; x < s.idx.size(); ++x) {
      const u64 j = s.idx[x];
      out->start_sec[j] = st[x]; out->reason[j] = rs[x];
      const u64 dst = out->place_offsets[j], k = jb->node_num[j];
      for (u64 i = 0; i < k; ++i) {
        out->node_idx[dst + i] = nd[src + i]; out->ntasks[dst + i] = nt[src + i]; out->cpu_raw[dst + i] = cpu[src + i]; out->mem[dst + i] = mem[src + i];
        out->core_lo[dst + i] = lo[src + i]; out->core_hi[dst + i] = hi[src + i]; out->gres[dst + i] = gr[src + i];
        if (out->core_w2) out->core_w2[dst + i] = h->lay.wide_cores ? w2[src + i] : 0;
        if (out->core_w3) out->core_w3[dst + i] = h->lay.wide_cores ? w3[src + i] : 0;
      }
      src += k;
    }
  };
  on_threads(scatter);
  // ... and the jobs decided here: behind the batch limit ("Priority", JobScheduler.h:196-198), or of a partition whose device serves nothing
  for (u64 j = 0; j < J; ++j) {
    if (jdev[j] < kDevRefused) continue;
    out->start_sec[j] = 0;
    out->reason[j] = jdev[j] == kDevBatch ? CNS_REASON_PRIORITY : CNS_REASON_ENGINE_REFUSED;
    const u64 dst = out->place_offsets[j], k = jb->node_num[j];
    for (u64 i = 0; i < k; ++i) {
      out->node_idx[dst + i] = CNS_NODE_NONE; out->ntasks[dst + i] = 0; out->cpu_raw[dst + i] = 0; out->mem[dst + i] = 0;
      out->core_lo[dst + i] = 0; out->core_hi[dst + i] = 0; out->gres[dst + i] = 0;
      if (out->core_w2) out->core_w2[dst + i] = 0;
      if (out->core_w3) out->core_w3[dst + i] = 0;
    }
  }
  const auto t4 = std::chrono::steady_clock::now();
  cns_group_info& I = g->info;
  I.num_devices = n;
  I.gather_mode = g->distinct ? CNS_GATHER_RCCL : CNS_GATHER_DEVICE_COPIES;
  I.shards_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  I.allgather_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
  I.download_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
  I.scatter_ms = std::chrono::duration<double, std::milli>(t4 - t3).count();
  I.slot_bytes = slot;
  I.max_select_ms = 0;
  for (u32 d : g->active) I.max_select_ms = std::max(I.max_select_ms, g->eng[d]->timing.select_ms);
  return CNS_OK;
}

int cns_group_get_info(const cns_group* g, cns_group_info* out) {
  if (!g || !out) return CNS_ERR_INVALID_ARG;
  *out = g->info;
  return CNS_OK;
}

int cns_group_get_partition_status(const cns_group* g, uint8_t* status, uint32_t capacity) {
  if (!g || !status) return CNS_ERR_INVALID_ARG;
  if (g->part_status.empty() && g->P == 0) return CNS_ERR_STATE;
  if (capacity < g->P) return CNS_ERR_INVALID_ARG;
  for (u32 p = 0; p < g->P; ++p) status[p] = g->part_status[p];
  return CNS_OK;
}

uint32_t cns_group_device_of_partition(const cns_group* g, uint32_t partition) {
  return (g && partition < g->P) ? g->part_dev[partition] : 0xFFFFFFFFu;
}

}  // extern "C"
