// Host side of include/crane_gpu_probe/probe.h.  Included by engine.hip inside extern "C".
// Host work: validation, the pre-checks and the routing of cns_upload_jobs (jobs_host.inc, never cut by scheduled_batch_size), the
// buffers.  The records are packed and derived by the cycle's own k_pack_jobs / k_prep_jobs, through the steps the queue takes
// (job_table.inc) on a table of the probes' own; every test runs in k_probe (probe_kernel.inc).  Everything a probe call writes on the
// device lies in buffers of its own (cns_engine::pt, d_pb): the cycle's job table, result buffer, fault word and timing are not
// touched.  No CPU fallback.

static int probe_state(cns_handle* h, const char* who) {
  if (!h->have_run) return fail(h, CNS_ERR_STATE, std::string(who) + " before a successful cycle (cns_select / cns_run_resident), or after the snapshot or the queue changed");
  if (h->run_preempt)
    return fail(h, CNS_ERR_UNSUPPORTED, std::string(who) + " after a cycle with preemption (cns_select_preempt, enabled): a probe that may itself preempt is not served");
  return 0;
}

static int probe_upload_impl(cns_handle* h, const cns_job_soa* jb) {
  if (int rc = table_check(h, jb, kProbeMsgs)) return rc;
  if (int rc = table_lists_check(h, jb, kProbeMsgs)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  JobTable& T = h->pt;
  if (int rc = table_stage(h, T, jb)) return rc;
  // the pre-checks and the routing of the ordered loop (JobScheduler.cpp:6744-6761), as for the cycle's queue — but no probe is cut
  cns_jobs_host::Out O;
  if (int rc = table_route(h, T, jb, jb->num_jobs, "probe ", O)) return rc;
  // per record of the grouped table: its engine partition; and the widest node_num (the heap scratch of a workgroup)
  std::vector<u32> part_of((size_t)std::max<u64>(O.Jg, 1), 0);
  u32 kmax = 1;
  for (u64 i = 0; i < O.Jg; ++i) { part_of[(size_t)i] = T.job_part[O.grouped[i]]; kmax = std::max(kmax, jb->node_num[O.grouped[i]]); }
  if (int rc = upload(h, h->d_pb[PB_PART], part_of)) return rc;
  if (int rc = table_layout(h, T, jb, O)) return rc;   // the layout of the cycle's packed buffer, in a buffer of the probes' own
  if (int rc = table_pack(h, T, jb)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (part_of ends with this scope)
  h->pkmax = kmax;
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
  table_bind(h, h->pt, K);
  K.pj_off = nullptr;
  K.bf_j = nullptr; K.g_upd = nullptr; K.prof = nullptr; K.wide_ctl = nullptr; K.wide_last = nullptr; K.giant_ctl = nullptr;
  K.f_len = nullptr;                         // (kept by one commit path only: the block header has the length)
  K.general_only = 0; K.serial_only = 0; K.part_map = nullptr; K.launch_parts = 0; K.pre = PreParams{};
  if (int rc = table_reset(h, h->pt)) return rc;
  HIPCHK(h, B[PB_FAULT].ensure(16));
  HIPCHK(h, hipMemsetAsync(B[PB_FAULT].p, 0, 16, h->stream));
  K.fault = B[PB_FAULT].as<u32>();
  float ms = 0;
  u64 grid = 0;
  u32 stride = 0;
  if (h->pt.Jg) {
    // Persistent one-wave workgroups, as many as the device holds at once (the runtime's occupancy figure for this kernel x its compute
    // units), never more than there are probes; the heap scratch is per RESIDENT workgroup and capped: probe_plan_host.inc.
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_probe, kProbeBlock, 0) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    const cns_probe_plan::Plan L = cns_probe_plan::plan(cns_probe_plan::resident(per_cu, h->num_cus), h->pt.Jg, h->rlay.max_np, h->pkmax, (uint32_t)sizeof(HeapEnt),
                                                        cns_probe_plan::scratch_cap());
    grid = L.grid; stride = L.stride;
    HIPCHK(h, B[PB_HEAP].ensure((size_t)L.bytes));
    K.heap = B[PB_HEAP].as<HeapEnt>();
    HIPCHK(h, B[PB_CTR].ensure(16));
    HIPCHK(h, hipMemsetAsync(B[PB_CTR].p, 0, 16, h->stream));
    HIPCHK(h, B[PB_PARAMS].ensure(sizeof(KParams)));
    HIPCHK(h, hipMemcpyAsync(B[PB_PARAMS].p, &K, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_prep_jobs, dim3((unsigned)((h->pt.Jg + 255) / 256)), dim3(256), 0, h->stream, B[PB_PARAMS].as<KParams>(), (u64)h->pt.Jg);
    HIPCHK(h, hipGetLastError());
    ProbeParams Q{};
    Q.nq = h->pt.Jg; Q.part = B[PB_PART].as<u32>(); Q.counter = B[PB_CTR].as<u32>(); Q.heap_stride = stride;
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
  h->probe_grid = grid; h->probe_stride = stride;
  h->probes_answered = true;
  if (kernel_ms) *kernel_ms = ms;
  return CNS_OK;
}

int cns_probe_download(cns_handle* h, cns_placement_soa* out) {
  if (!h || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_probe_download: null argument");
  if (int rc = probe_state(h, "cns_probe_download")) return rc;
  if (!h->have_probes || !h->probes_answered) return fail(h, CNS_ERR_STATE, "cns_probe_download before cns_probe_run_resident");
  if (h->pt.J == 0) return CNS_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = table_download(h, h->pt, out, kProbeMsgs)) return rc;
  table_offsets(h->pt, out);
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

int cns_probe_shape(cns_probe_shape_info* out) {
  if (!out) return CNS_ERR_INVALID_ARG;
  cns_probe_shape_info s{};
  s.block = (u32)kProbeBlock;
  s.dip_cpu_sat = kDipCpuSat; s.dip_mem_sat = kDipMemSat; s.dip_gres_sat = kDipGresSat;
  s.gres_classes = (u32)kMaxClasses; s.gres_names = (u32)kMaxNames;
  s.max_types = CNS_MAX_NODE_TYPES;
  s.heap_ent_bytes = (u32)sizeof(HeapEnt);
  s.loff_clamp = kProbeLoffClamp;
  s.scratch_cap = cns_probe_plan::kScratchCap;
  *out = s;
  return CNS_OK;
}

int cns_debug_get_probe_plan(cns_handle* h, uint64_t* grid, uint32_t* stride) {
  if (!h || !grid || !stride) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_probe_plan: null argument");
  if (!h->have_probes || !h->probes_answered) return fail(h, CNS_ERR_STATE, "cns_debug_get_probe_plan before cns_probe_run_resident");
  *grid = h->probe_grid; *stride = h->probe_stride;
  return CNS_OK;
}

int cns_debug_get_dips(cns_handle* h, uint32_t* dip_t, uint32_t* dip_cm, uint32_t* dip_g) {
  if (!h || !dip_t || !dip_cm || !dip_g) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_dips: null argument");
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_debug_get_dips before a successful run");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = h->rlay.S;
  std::vector<u32> t(std::max<size_t>(S, 1)), cm(t.size()), g(t.size());
  HIPCHK(h, hipMemcpy(t.data(), h->d_dipt.p, S * sizeof(u32), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(cm.data(), h->d_dipcm.p, S * sizeof(u32), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(g.data(), h->d_dipg.p, S * sizeof(u32), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < h->lay.orig_pos_slot.size(); ++i) {   // slot order as cns_debug_get_costs; a slot the engine does not keep: no dip
    const u32 q = h->lay.orig_pos_slot[i];
    dip_t[i] = q == kNone ? 0xFFFFFFFFu : t[q];
    dip_cm[i] = q == kNone ? 0u : cm[q];
    dip_g[i] = q == kNone ? 0u : g[q];
  }
  return CNS_OK;
}
