// Host side of include/crane_gpu_valid/validity.h.  Included by engine.hip inside extern "C".
// Host work: validation of the lists (sorted per job on the way: a node twice shows as two equal neighbours), the job indices grouped by
// partition (a counting sort over chunks of the queue on the host threads of jobs_host.inc), the chunk table, the buffers.  Every test of
// a job against a node or a partition runs on the device (valid_kernels.inc).  Everything lives in cns_engine::d_vd and the vd_* copies of
// the caller's node arrays that cns_set_nodes keeps: no flag and no buffer of a cycle, a probe or a reservation what-if is read or
// written, except the node lists of the reservations (cns_engine::rlay, read).  No CPU fallback.

constexpr u64 kVdMaxJobs = 0xFFFFFFF0ull;   // 2^32 - 16 jobs of one call (DESIGN.md 8): job indices and grouped positions are 32-bit

// what cns_set_nodes keeps for this call: the caller's arrays as they came (every listed node, schedulable or not)
static void valid_keep_nodes(cns_handle* h, const cns_node_soa* nd) {
  const u32 N = nd->num_nodes, P = nd->num_partitions;
  h->vd_cpu.assign(nd->cpu_total_raw, nd->cpu_total_raw + N);
  h->vd_mem.assign(nd->mem_total, nd->mem_total + N);
  if (nd->gres_slots) h->vd_gres.assign(nd->gres_slots, nd->gres_slots + N); else h->vd_gres.clear();
  if (nd->unsupported) h->vd_unsup.assign(nd->unsupported, nd->unsupported + N); else h->vd_unsup.clear();
  h->vd_poff.assign(nd->part_offsets, nd->part_offsets + P + 1);
  h->vd_pnodes.assign(nd->part_nodes + nd->part_offsets[0], nd->part_nodes + nd->part_offsets[P]);
  for (u32& o : h->vd_poff) o -= nd->part_offsets[0];
  h->vd_tab_have = h->vd_rv_have = false;
}

static int valid_build_tables(cns_handle* h) {
  const u32 N = (u32)h->vd_cpu.size(), P = (u32)h->vd_poff.size() - 1;
  for (u32 n = 0; n < N; ++n)
    if (h->vd_cpu[n] < 0) return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: node " + std::to_string(n) + ": cpu_total_raw < 0");
  if ((u64)h->vd_poff[P] > 0xFFFFFFFFull - 2 * kVdTile) return fail(h, CNS_ERR_UNSUPPORTED, "cns_validate_jobs: more than 2^32 - 513 (partition, node) entries");
  std::vector<u32> pn(h->vd_pnodes.size());   // craned_ids is a set (:7354): ascending here, which is also the membership table of the list paths
  if (const auto v = cns_csr::sort_lists(h->vd_poff.data(), h->vd_pnodes.data(), pn.data(), 0, P); v.what != cns_csr::Lists::Ok)
    return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: partition " + std::to_string(v.list) + " lists node " + std::to_string(v.value) + " twice");
  DevBuf* B = h->d_vd;
  if (int rc = upload(h, B[VD_NCPU], h->vd_cpu)) return rc;
  if (int rc = upload(h, B[VD_NMEM], h->vd_mem)) return rc;
  if (int rc = upload(h, B[VD_NGRES], h->vd_gres)) return rc;
  if (int rc = upload(h, B[VD_NUNSUP], h->vd_unsup)) return rc;
  if (int rc = upload(h, B[VD_POFF], h->vd_poff)) return rc;
  if (int rc = upload(h, B[VD_PNODES], pn)) return rc;
  HIPCHK(h, B[VD_NODE].ensure((size_t)N * sizeof(VdNode)));
  HIPCHK(h, B[VD_TOTAL].ensure((size_t)P * sizeof(VdTotal)));
  hipLaunchKernelGGL(k_valid_prep, dim3((N + kVdBlock - 1) / kVdBlock), dim3(kVdBlock), 0, h->stream, N, (const i64*)B[VD_NCPU].as<i64>(),
                     (const u64*)B[VD_NMEM].as<u64>(), h->vd_gres.empty() ? (const u64*)nullptr : (const u64*)B[VD_NGRES].as<u64>(),
                     h->vd_unsup.empty() ? (const uint8_t*)nullptr : (const uint8_t*)B[VD_NUNSUP].as<uint8_t>(), h->gres, B[VD_NODE].as<VdNode>());
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_valid_totals, dim3(P), dim3(kVdBlock), 0, h->stream, P, (const u32*)B[VD_POFF].as<u32>(), (const u32*)B[VD_PNODES].as<u32>(),
                     (const VdNode*)B[VD_NODE].as<VdNode>(), B[VD_TOTAL].as<VdTotal>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the sorted lists are a local vector)
  h->vd_tab_have = true;
  return CNS_OK;
}

// the nodes of every reservation of the last cns_set_reservations, ascending (:7339-7342)
static int valid_build_resv(cns_handle* h) {
  const cns_snapshot::ResvLayout& X = h->rlay;   // (the slots of reservation v's virtual partition are its nodes, ascending)
  const u32 V = X.V, first = h->lay.S_real;
  std::vector<u32> off((size_t)V + 1, 0), nodes(X.slot_node.begin() + first, X.slot_node.end());
  for (u32 v = 0; v < V; ++v) off[(size_t)v + 1] = X.part_off[h->lay.P_real + v + 1] - first;
  if (int rc = upload(h, h->d_vd[VD_RVOFF], off)) return rc;
  if (int rc = upload(h, h->d_vd[VD_RVNODES], nodes)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->vd_V = V;
  h->vd_rv_have = true;
  return CNS_OK;
}

// the jobs [beg, end) of one list CSR of the call: offsets checked, every job's entries copied sorted, a node twice refused
static bool valid_lists_ok(const u64* off, const u32* src, u32* dst, u64 beg, u64 end) {
  return cns_csr::first_decrease(off + beg, end - beg) == end - beg && cns_csr::sort_lists(off, src, dst, beg, end).what == cns_csr::Lists::Ok;
}

static int validate_impl(cns_handle* h, const cns_job_soa* jb, const cns_validity_out* out, double* kernel_ms) {
  const u64 J = jb->num_jobs;
  if (!jb->partition || !jb->node_mem || !jb->task_cpu_raw || !jb->task_mem || !jb->node_num || !jb->ntasks)
    return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: missing array");
  if (!out->code || !out->eligible) return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: missing result array");
  const bool has_incl = jb->incl_offsets && jb->incl_offsets[J] != 0, has_excl = jb->excl_offsets && jb->excl_offsets[J] != 0;
  if ((has_incl && !jb->incl_nodes) || (has_excl && !jb->excl_nodes)) return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: list offsets without the list");
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->vd_tab_have)
    if (int rc = valid_build_tables(h)) return rc;
  if (!h->vd_rv_have)
    if (int rc = valid_build_resv(h)) return rc;
  const u32 N = (u32)h->vd_cpu.size(), P = (u32)h->vd_poff.size() - 1;

  // ---- the validating pass: lists sorted and checked, jobs counted per partition (bin P: no such partition), then placed ----
  std::vector<u32> incl_sorted(has_incl ? (size_t)jb->incl_offsets[J] : 0), excl_sorted(has_excl ? (size_t)jb->excl_offsets[J] : 0);
  std::vector<u32> order((size_t)J);
  const u32 threads = cns_jobs_host::threads_for(J, h->host_threads);
  std::vector<cns_jobs_host::Chunk> chunks(threads);
  for (u32 c = 0; c < threads; ++c) { chunks[c].beg = J * c / threads; chunks[c].end = J * (c + 1) / threads; }
  cns_jobs_host::for_chunks(chunks, [&](cns_jobs_host::Chunk& c, uint32_t) {
    c.cnt.assign((size_t)P + 1, 0);
    for (u64 j = c.beg; j < c.end; ++j) c.cnt[std::min<u32>(jb->partition[j], P)]++;
    if ((has_incl && !valid_lists_ok(jb->incl_offsets, jb->incl_nodes, incl_sorted.data(), c.beg, c.end)) ||
        (has_excl && !valid_lists_ok(jb->excl_offsets, jb->excl_nodes, excl_sorted.data(), c.beg, c.end)))
      c.bad_job = c.beg;
  });
  for (const auto& c : chunks)
    if (c.bad_job != ~0ull) return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: a list names a node twice, or list offsets decrease");
  std::vector<u64> pj_off((size_t)P + 2, 0);
  for (const auto& c : chunks)
    for (u32 p = 0; p <= P; ++p) pj_off[(size_t)p + 1] += c.cnt[p];
  for (u32 p = 0; p <= P; ++p) pj_off[(size_t)p + 1] += pj_off[p];
  {
    std::vector<u64> cur(pj_off.begin(), pj_off.end() - 1);
    for (auto& c : chunks)
      for (u32 p = 0; p <= P; ++p) { const u64 n = c.cnt[p]; c.cnt[p] = cur[p]; cur[p] += n; }
  }
  cns_jobs_host::for_chunks(chunks, [&](cns_jobs_host::Chunk& c, uint32_t) {
    for (u64 j = c.beg; j < c.end; ++j) order[c.cnt[std::min<u32>(jb->partition[j], P)]++] = (u32)j;
  });
  std::vector<VdChunkRec> recs;
  for (u32 p = 0; p <= P; ++p)
    for (u64 f = pj_off[p]; f < pj_off[(size_t)p + 1]; f += kVdChunk)
      recs.push_back(VdChunkRec{p < P ? p : kVdNoPart, (u32)f, (u32)std::min<u64>(kVdChunk, pj_off[(size_t)p + 1] - f), 0u});

  // ---- the caller's job arrays as they are, the call's tables, the results ----
  DevBuf* B = h->d_vd;
  if (int rc = stage(h, B[VD_JNCPU], jb->node_cpu_raw, (size_t)J * 8)) return rc;
  if (int rc = stage(h, B[VD_JNMEM], jb->node_mem, (size_t)J * 8)) return rc;
  if (int rc = stage(h, B[VD_JTCPU], jb->task_cpu_raw, (size_t)J * 8)) return rc;
  if (int rc = stage(h, B[VD_JTMEM], jb->task_mem, (size_t)J * 8)) return rc;
  if (int rc = stage(h, B[VD_JK], jb->node_num, (size_t)J * 4)) return rc;
  if (int rc = stage(h, B[VD_JNT], jb->ntasks, (size_t)J * 4)) return rc;
  if (int rc = stage(h, B[VD_JGT], jb->gres_total, (size_t)J * CNS_MAX_GRES_NAMES)) return rc;
  if (int rc = stage(h, B[VD_JGS], jb->gres_spec, (size_t)J * CNS_MAX_GRES_CLASSES)) return rc;
  if (int rc = stage(h, B[VD_JRSV], jb->reservation, (size_t)J * 4)) return rc;
  if (has_incl) {
    if (int rc = stage(h, B[VD_IOFF], jb->incl_offsets, ((size_t)J + 1) * 8)) return rc;
    if (int rc = stage(h, B[VD_INCL], incl_sorted.data(), incl_sorted.size() * 4)) return rc;
  }
  if (has_excl) {
    if (int rc = stage(h, B[VD_EOFF], jb->excl_offsets, ((size_t)J + 1) * 8)) return rc;
    if (int rc = stage(h, B[VD_EXCL], excl_sorted.data(), excl_sorted.size() * 4)) return rc;
  }
  if (int rc = stage(h, B[VD_ORDER], order.data(), (size_t)J * 4)) return rc;
  if (int rc = stage(h, B[VD_CHUNKS], recs.data(), recs.size() * sizeof(VdChunkRec))) return rc;
  HIPCHK(h, B[VD_CODE].ensure((size_t)J));
  HIPCHK(h, B[VD_ELIG].ensure((size_t)J * 4));
  VdParams A{};
  A.N = N; A.P = P; A.V = h->vd_V;
  A.node = B[VD_NODE].as<VdNode>(); A.total = B[VD_TOTAL].as<VdTotal>(); A.part_off = B[VD_POFF].as<u32>(); A.part_nodes = B[VD_PNODES].as<u32>();
  A.rv_off = B[VD_RVOFF].as<u32>(); A.rv_nodes = B[VD_RVNODES].as<u32>();
  A.node_cpu = jb->node_cpu_raw ? B[VD_JNCPU].as<i64>() : nullptr; A.node_mem = B[VD_JNMEM].as<u64>();
  A.task_cpu = B[VD_JTCPU].as<i64>(); A.task_mem = B[VD_JTMEM].as<u64>(); A.node_num = B[VD_JK].as<u32>(); A.ntasks = B[VD_JNT].as<u32>();
  A.gres_total = jb->gres_total ? B[VD_JGT].as<u32>() : nullptr; A.gres_spec = jb->gres_spec ? B[VD_JGS].as<u64>() : nullptr;
  A.reservation = jb->reservation ? B[VD_JRSV].as<u32>() : nullptr;
  A.incl_off = has_incl ? B[VD_IOFF].as<u64>() : nullptr; A.incl = has_incl ? B[VD_INCL].as<u32>() : nullptr;
  A.excl_off = has_excl ? B[VD_EOFF].as<u64>() : nullptr; A.excl = has_excl ? B[VD_EXCL].as<u32>() : nullptr;
  A.order = B[VD_ORDER].as<u32>(); A.chunks = B[VD_CHUNKS].as<VdChunkRec>();
  A.code = B[VD_CODE].as<uint8_t>(); A.eligible = B[VD_ELIG].as<u32>();
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  hipLaunchKernelGGL(k_valid_walk, dim3((unsigned)recs.size()), dim3(kVdBlock), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipMemcpyAsync(out->code, A.code, (size_t)J, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out->eligible, A.eligible, (size_t)J * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (kernel_ms) *kernel_ms = ms;
  return CNS_OK;
}

int cns_validate_jobs(cns_handle* h, const cns_job_soa* jobs, const cns_validity_out* out, double* kernel_ms) {
  if (!h || !jobs) return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: null argument");
  if (kernel_ms) *kernel_ms = 0.0;
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_validate_jobs before cns_set_nodes");
  if (jobs->num_jobs == 0) return CNS_OK;   // nothing asked, nothing written
  if (jobs->num_jobs > kVdMaxJobs) return fail(h, CNS_ERR_UNSUPPORTED, "cns_validate_jobs: more than 2^32 - 16 jobs in one call");
  if (!out) return fail(h, CNS_ERR_INVALID_ARG, "cns_validate_jobs: null result");
  const int rc = validate_impl(h, jobs, out, kernel_ms);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_validate_shape(uint32_t* node_tile, uint32_t* job_chunk) {
  if (node_tile) *node_tile = kVdTile;
  if (job_chunk) *job_chunk = kVdChunk;
  return CNS_OK;
}
