// Host side of include/crane_gpu_probe/probe.h.  Included by engine.hip inside extern "C".
// Host work: validation, the pre-checks and the routing of cns_upload_jobs (jobs_host.inc, never cut by scheduled_batch_size), the
// buffers.  The records are packed and derived by the cycle's own k_pack_jobs / k_prep_jobs; every test runs in k_probe
// (probe_kernel.inc).  Everything a probe call writes on the device lies in buffers of its own (cns_engine::d_pb): the cycle's job
// table, result buffer, fault word and timing are not touched.  No CPU fallback.

static int probe_state(cns_handle* h, const char* who) {
  if (!h->have_run) return fail(h, CNS_ERR_STATE, std::string(who) + " before a successful cycle (cns_select / cns_run_resident), or after the snapshot or the queue changed");
  if (h->run_preempt)
    return fail(h, CNS_ERR_UNSUPPORTED, std::string(who) + " after a cycle with preemption (cns_select_preempt, enabled): a probe that may itself preempt is not served");
  return 0;
}

static int probe_upload_impl(cns_handle* h, const cns_job_soa* jb) {
  const u64 J = jb->num_jobs;
  if (J && (!jb->partition || !jb->time_limit_sec || !jb->node_mem || !jb->task_cpu_raw || !jb->task_mem ||
            !jb->node_num || !jb->ntasks || !jb->ntasks_per_node_min || !jb->ntasks_per_node_max))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_upload: missing array");
  if (J > 0xFFFFFFF0ull) return fail(h, CNS_ERR_UNSUPPORTED, "more than 2^32-16 probes");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_pb;
  DevBuf* rb_ = B + PB_RAW0;
  if (int rc = stage(h, rb_[0], jb->time_limit_sec, J * 8)) return rc;
  if (jb->node_cpu_raw) { if (int rc = stage(h, rb_[1], jb->node_cpu_raw, J * 8)) return rc; }
  if (int rc = stage(h, rb_[2], jb->node_mem, J * 8)) return rc;
  if (int rc = stage(h, rb_[3], jb->task_cpu_raw, J * 8)) return rc;
  if (int rc = stage(h, rb_[4], jb->task_mem, J * 8)) return rc;
  if (int rc = stage(h, rb_[5], jb->node_num, J * 4)) return rc;
  if (int rc = stage(h, rb_[6], jb->ntasks, J * 4)) return rc;
  if (int rc = stage(h, rb_[7], jb->ntasks_per_node_min, J * 4)) return rc;
  if (int rc = stage(h, rb_[8], jb->ntasks_per_node_max, J * 4)) return rc;
  if (jb->exclusive) { if (int rc = stage(h, rb_[9], jb->exclusive, J)) return rc; }
  if (jb->gres_total) { if (int rc = stage(h, rb_[10], jb->gres_total, J * CNS_MAX_GRES_NAMES)) return rc; }
  if (jb->gres_spec) { if (int rc = stage(h, rb_[11], jb->gres_spec, J * CNS_MAX_GRES_CLASSES)) return rc; }
  if (jb->incl_offsets) { if (int rc = stage(h, rb_[12], jb->incl_offsets, (J + 1) * 8)) return rc; }
  if (jb->excl_offsets) { if (int rc = stage(h, rb_[13], jb->excl_offsets, (J + 1) * 8)) return rc; }
  const u64 n_incl = jb->incl_offsets ? jb->incl_offsets[J] : 0, n_excl = jb->excl_offsets ? jb->excl_offsets[J] : 0;
  if ((n_incl && !jb->incl_nodes) || (n_excl && !jb->excl_nodes)) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_upload: include / exclude offsets without node lists");
  HIPCHK(h, B[PB_INCL].ensure(std::max<u64>(n_incl, 1) * 4));
  HIPCHK(h, B[PB_EXCL].ensure(std::max<u64>(n_excl, 1) * 4));
  if (int rc = stage(h, B[PB_INCL], jb->incl_nodes, n_incl * 4)) return rc;
  if (int rc = stage(h, B[PB_EXCL], jb->excl_nodes, n_excl * 4)) return rc;
  // the pre-checks and the routing of the ordered loop (JobScheduler.cpp:6744-6761), as for the cycle's queue — but no probe is cut
  namespace jh = cns_jobs_host;
  std::vector<uint8_t> reason(std::max<u64>(J, 1), 0), jtag(std::max<u64>(J, 1), 0);
  std::vector<u32> job_part((size_t)std::max<u64>(J, 1), kNone);
  std::vector<u64> place_off((size_t)J + 1, 0);
  jh::Route R;
  R.P = h->rlay.P; R.Pu = h->lay.Pu; R.P_real = h->lay.P_real; R.V = h->rlay.V;
  R.upart_refused = h->lay.upart_refused.data(); R.upart_eng = h->lay.upart_eng.data(); R.upart_size = h->lay.upart_size.data();
  R.upart_tag = h->lay.upart_tag.data(); R.part_off = h->rlay.part_off.data();
  R.s_node = h->rlay.big_nodes ? 48 : 32; R.gres_classes = h->gres.num_classes; R.batch = J;
  jh::Out O;
  O.reason = reason.data(); O.job_part = job_part.data(); O.place_off = place_off.data();
  O.jtag = h->lay.shared ? jtag.data() : nullptr;
  std::vector<jh::Chunk> chunks;
  {
    std::string perr;
    if (const int rc = jh::pass1(jb, R, O, chunks, jh::threads_for(J, h->host_threads), &perr)) return fail(h, rc, "probe " + perr);
  }
  const u64 Jg = O.Jg, places = O.places;
  std::vector<u32> grouped((size_t)std::max<u64>(Jg, 1), 0);
  O.grouped = grouped.data();
  jh::pass2(jb, O, chunks);
  // per record of the grouped table: its engine partition; and the widest node_num (the heap scratch of a workgroup)
  std::vector<u32> part_of((size_t)std::max<u64>(Jg, 1), 0);
  u32 kmax = 1;
  for (u64 i = 0; i < Jg; ++i) { part_of[(size_t)i] = job_part[grouped[(size_t)i]]; kmax = std::max(kmax, jb->node_num[grouped[(size_t)i]]); }
  if (int rc = stage(h, rb_[14], place_off.data(), (J + 1) * 8)) return rc;
  if (int rc = stage(h, rb_[15], grouped.data(), grouped.size() * 4)) return rc;
  if (h->lay.shared) { if (int rc = stage(h, B[PB_JTAG], jtag.data(), jtag.size())) return rc; }
  if (int rc = stage(h, B[PB_PART], part_of.data(), part_of.size() * 4)) return rc;
  if (int rc = stage(h, B[PB_REASON], reason.data(), reason.size())) return rc;
  HIPCHK(h, B[PB_JOBS].ensure((size_t)std::max<u64>(Jg, 1) * kJobRecDwords * 4));
  if (Jg) {
    PackParams K{};
    K.Jg = Jg; K.grouped = rb_[15].as<u32>();
    K.L = rb_[0].as<i64>(); K.ncpu = jb->node_cpu_raw ? rb_[1].as<i64>() : nullptr; K.nmem = rb_[2].as<u64>();
    K.tcpu = rb_[3].as<i64>(); K.tmem = rb_[4].as<u64>(); K.k = rb_[5].as<u32>(); K.ntasks = rb_[6].as<u32>();
    K.tmin = rb_[7].as<u32>(); K.tmax = rb_[8].as<u32>();
    K.excl = jb->exclusive ? rb_[9].as<uint8_t>() : nullptr;
    K.gtot = jb->gres_total ? rb_[10].as<uint8_t>() : nullptr; K.gspec = jb->gres_spec ? rb_[11].as<uint8_t>() : nullptr;
    K.incl_off = jb->incl_offsets ? rb_[12].as<u64>() : nullptr; K.excl_off = jb->excl_offsets ? rb_[13].as<u64>() : nullptr;
    K.place_off = rb_[14].as<u64>(); K.jobrec = B[PB_JOBS].as<u32>();
    K.tag = h->lay.shared ? B[PB_JTAG].as<uint8_t>() : nullptr;
    hipLaunchKernelGGL(k_pack_jobs, dim3((unsigned)((Jg + 255) / 256)), dim3(256), 0, h->stream, K);
    HIPCHK(h, hipGetLastError());
  }
  // results: the layout of the cycle's packed buffer, in a buffer of the probes' own
  cns_engine::ResOff& r = h->pro;
  size_t ro = 0;
  auto rsec = [&](size_t elem, u64 n) { size_t x = ro; ro = align16(ro + elem * (size_t)std::max<u64>(n, 1)); return x; };
  r.start = rsec(8, J); r.cpu = rsec(8, places); r.mem = rsec(8, places); r.clo = rsec(8, places);
  r.chi = rsec(8, places); r.gres = rsec(8, places); r.node = rsec(4, places); r.ntasks = rsec(4, places);
  r.reason = rsec(1, J);
  r.c2 = r.c3 = ro;
  if (h->lay.wide_cores) { r.c2 = rsec(8, places); r.c3 = rsec(8, places); }
  r.total = ro;
  HIPCHK(h, B[PB_RESULTS].ensure(ro));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the staging vectors above end with this scope)
  h->pJ = J; h->pJg = Jg; h->pplaces = places; h->pkmax = kmax;
  h->probe_place_off = std::move(place_off);
  h->have_probes = true;
  return CNS_OK;
}

// The caller owns its arrays again when the call is back, on every path (as cns_upload_jobs).
int cns_probe_upload(cns_handle* h, const cns_job_soa* jb) {
  if (!h || !jb) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_upload: null argument");
  if (int rc = probe_state(h, "cns_probe_upload")) return rc;
  h->have_probes = h->probes_answered = false;
  const int rc = probe_upload_impl(h, jb);
  if (rc != 0) drain(h);
  return rc;
}

int cns_probe_run_resident(cns_handle* h, double* kernel_ms) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_run_resident: null handle");
  if (int rc = probe_state(h, "cns_probe_run_resident")) return rc;
  if (!h->have_probes) return fail(h, CNS_ERR_STATE, "cns_probe_run_resident before cns_probe_upload");
  if (kernel_ms) *kernel_ms = 0.0;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_pb;
  // the cycle's parameter block at the cycle's `now`, with the probes' job table, result arrays, scratch and fault word
  KParams K;
  fill_params(h, K, h->last_now);
  char* rb = B[PB_RESULTS].as<char>();
  const cns_engine::ResOff& ro = h->pro;
  K.pj_off = nullptr; K.jobrec = B[PB_JOBS].as<u32>(); K.incl_nodes = B[PB_INCL].as<u32>(); K.excl_nodes = B[PB_EXCL].as<u32>();
  K.o_start = (i64*)(rb + ro.start); K.o_cpu = (i64*)(rb + ro.cpu); K.o_mem = (u64*)(rb + ro.mem); K.o_clo = (u64*)(rb + ro.clo);
  K.o_chi = (u64*)(rb + ro.chi); K.o_gres = (u64*)(rb + ro.gres); K.o_node = (u32*)(rb + ro.node); K.o_ntasks = (u32*)(rb + ro.ntasks);
  K.o_reason = (uint8_t*)(rb + ro.reason);
  K.o_c2 = h->lay.wide_cores ? (u64*)(rb + ro.c2) : nullptr; K.o_c3 = h->lay.wide_cores ? (u64*)(rb + ro.c3) : nullptr;
  K.bf_j = nullptr; K.g_upd = nullptr; K.prof = nullptr; K.wide_ctl = nullptr; K.wide_last = nullptr; K.giant_ctl = nullptr;
  K.f_len = nullptr;                         // (kept by one commit path only: the block header has the length)
  K.general_only = 0; K.serial_only = 0; K.part_map = nullptr; K.launch_parts = 0; K.pre = PreParams{};
  const u64 pl = std::max<u64>(h->pplaces, 1), J = std::max<u64>(h->pJ, 1);
  HIPCHK(h, hipMemsetAsync(rb + ro.start, 0, ro.node - ro.start, h->stream));
  HIPCHK(h, hipMemsetAsync(rb + ro.node, 0xFF, 4 * pl, h->stream));   // CNS_NODE_NONE
  HIPCHK(h, hipMemsetAsync(rb + ro.ntasks, 0, 4 * pl, h->stream));
  if (h->lay.wide_cores) HIPCHK(h, hipMemsetAsync(rb + ro.c2, 0, ro.total - ro.c2, h->stream));
  HIPCHK(h, hipMemcpyAsync(rb + ro.reason, B[PB_REASON].p, J, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, B[PB_FAULT].ensure(16));
  HIPCHK(h, hipMemsetAsync(B[PB_FAULT].p, 0, 16, h->stream));
  K.fault = B[PB_FAULT].as<u32>();
  float ms = 0;
  if (h->pJg) {
    // Persistent one-wave workgroups, as many as the device holds at once (the runtime's occupancy figure for this kernel x its compute
    // units), never more than there are probes; the heap scratch is per RESIDENT workgroup: min(widest partition, widest node_num) + 1.
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_probe, kProbeBlock, 0) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    const u64 resident = (u64)std::max(per_cu, 1) * std::max<u32>(h->num_cus, 1);
    const u32 stride = std::min<u32>(h->rlay.max_np, h->pkmax) + 1u;
    u64 grid = std::min<u64>(h->pJg, resident);
    const u64 scratch_cap = 1ull << 30;       // ... and at most 1 GiB of it (a probe over thousands of nodes of a giant partition)
    grid = std::max<u64>(1, std::min<u64>(grid, scratch_cap / ((u64)stride * sizeof(HeapEnt))));
    HIPCHK(h, B[PB_HEAP].ensure((size_t)grid * stride * sizeof(HeapEnt)));
    K.heap = B[PB_HEAP].as<HeapEnt>();
    HIPCHK(h, B[PB_CTR].ensure(16));
    HIPCHK(h, hipMemsetAsync(B[PB_CTR].p, 0, 16, h->stream));
    HIPCHK(h, B[PB_PARAMS].ensure(sizeof(KParams)));
    HIPCHK(h, hipMemcpyAsync(B[PB_PARAMS].p, &K, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_prep_jobs, dim3((unsigned)((h->pJg + 255) / 256)), dim3(256), 0, h->stream, B[PB_PARAMS].as<KParams>(), (u64)h->pJg);
    HIPCHK(h, hipGetLastError());
    ProbeParams Q{};
    Q.nq = h->pJg; Q.part = B[PB_PART].as<u32>(); Q.counter = B[PB_CTR].as<u32>(); Q.heap_stride = stride;
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(k_probe, dim3((unsigned)grid), dim3(kProbeBlock), 0, h->stream, (const KParams*)B[PB_PARAMS].as<KParams>(), Q);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  } else {
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  u32 fault[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpy(fault, B[PB_FAULT].p, 16, hipMemcpyDeviceToHost));
  if (fault[0])
    return fail(h, CNS_ERR_DEVICE_FAULT, "device invariant violated: code " + std::to_string(fault[0]) + " probe " + std::to_string(fault[1]) +
                                             " aux " + std::to_string(fault[2]) + "," + std::to_string(fault[3]) + " (k_probe)");
  h->probe_ms = ms;
  h->probes_answered = true;
  if (kernel_ms) *kernel_ms = ms;
  return CNS_OK;
}

int cns_probe_download(cns_handle* h, cns_placement_soa* out) {
  if (!h || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_download: null argument");
  if (int rc = probe_state(h, "cns_probe_download")) return rc;
  if (!h->have_probes || !h->probes_answered) return fail(h, CNS_ERR_STATE, "cns_probe_download before cns_probe_run_resident");
  const size_t J = (size_t)h->pJ, pl = (size_t)h->pplaces;
  if (J == 0) return CNS_OK;
  if (out->place_capacity < h->pplaces) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_download: place_capacity too small");
  if (!out->start_sec || !out->reason || !out->place_offsets || !out->node_idx || !out->ntasks || !out->cpu_raw ||
      !out->mem || !out->core_lo || !out->core_hi || !out->gres)
    return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_download: missing result array");
  if (h->lay.wide_cores && (!out->core_w2 || !out->core_w3))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_download: the snapshot has nodes with core ids above 127: core_w2 / core_w3 are required");
  HIPCHK(h, hipSetDevice(h->device));
  const char* rb = h->d_pb[PB_RESULTS].as<char>();
  const cns_engine::ResOff& ro = h->pro;
  auto get = [&](void* dst, size_t off, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dst, rb + off, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
  };
  HIPCHK(h, get(out->start_sec, ro.start, 8 * J));
  HIPCHK(h, get(out->reason, ro.reason, J));
  HIPCHK(h, get(out->cpu_raw, ro.cpu, 8 * pl));
  HIPCHK(h, get(out->mem, ro.mem, 8 * pl));
  HIPCHK(h, get(out->core_lo, ro.clo, 8 * pl));
  HIPCHK(h, get(out->core_hi, ro.chi, 8 * pl));
  HIPCHK(h, get(out->gres, ro.gres, 8 * pl));
  if (h->lay.wide_cores) {
    HIPCHK(h, get(out->core_w2, ro.c2, 8 * pl));
    HIPCHK(h, get(out->core_w3, ro.c3, 8 * pl));
  } else {
    if (out->core_w2 && pl) memset(out->core_w2, 0, 8 * pl);
    if (out->core_w3 && pl) memset(out->core_w3, 0, 8 * pl);
  }
  HIPCHK(h, get(out->node_idx, ro.node, 4 * pl));
  HIPCHK(h, get(out->ntasks, ro.ntasks, 4 * pl));
  memcpy(out->place_offsets, h->probe_place_off.data(), 8 * (J + 1));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return CNS_OK;
}

int cns_probe(cns_handle* h, const cns_job_soa* probes, cns_placement_soa* out, double* kernel_ms) {
  if (!h || !probes) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe: null argument");
  if (kernel_ms) *kernel_ms = 0.0;
  if (int rc = probe_state(h, "cns_probe")) return rc;
  if (probes->num_jobs == 0) return CNS_OK;   // nothing asked, nothing written
  if (!out) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe: null result");
  if (int rc = cns_probe_upload(h, probes)) return rc;
  if (int rc = cns_probe_run_resident(h, kernel_ms)) return rc;
  return cns_probe_download(h, out);
}
