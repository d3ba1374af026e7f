// Host side of include/crane_gpu_gate/pending_gate.h.  Included by engine.hip inside extern "C".
// Host work: the input rules (gate_check_host.inc: one pass over the caller's arrays, no HIP in there), the buffers, the uploads, the
// launches.  Every event and every job is decided on the device (gate_kernels.inc).  Everything the call reads or writes on the device
// lives in cns_engine::d_gate; it needs no snapshot and no cycle.  No CPU fallback.

static int gate_impl(cns_handle* h, i64 now, const cns_gate_jobs* jb, const cns_gate_events* ev, const cns_gate_out* out, double* kernel_ms) {
  cns_gate::Sizes S;
  if (const cns_gate::Verdict v = cns_gate::check(jb, ev, out, &S)) return fail(h, v.code, v.msg);
  const u64 J = S.J, D = S.D, E = S.E;
  u64 counts[18];   // [16] jobs per code, [16] claimed entries, [17] events without their job
  memset(counts, 0, sizeof counts);
  u32 total = 0;
  float ms = 0;
  if (J) {
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf* B = h->d_gate;
    HIPCHK(h, B[GT_COUNTS].ensure(sizeof counts));
    HIPCHK(h, hipMemsetAsync(B[GT_COUNTS].p, 0, sizeof counts, h->stream));
    const bool claims = E && D;   // an event can claim an entry
    if (int rc = stage(h, B[GT_JOBID], jb->job_id, (size_t)J * 4)) return rc;
    if (jb->held) { if (int rc = stage(h, B[GT_HELD], jb->held, (size_t)J)) return rc; }
    if (jb->begin_sec) { if (int rc = stage(h, B[GT_BEGIN], jb->begin_sec, (size_t)J * 8)) return rc; }
    if (S.has_deps) {
      if (int rc = stage(h, B[GT_ISOR], jb->dep_is_or, (size_t)J)) return rc;
      if (int rc = stage(h, B[GT_READY], jb->dep_ready_sec, (size_t)J * 8)) return rc;
    }
    if (D) {
      if (int rc = stage(h, B[GT_DEPOFF], jb->dep_offsets, ((size_t)J + 1) * 8)) return rc;
      if (int rc = stage(h, B[GT_DEPJOB], jb->dep_job, (size_t)D * 4)) return rc;
      if (int rc = stage(h, B[GT_DELAY], jb->dep_delay_sec, (size_t)D * 8)) return rc;
    }
    if (S.has_array) {
      if (int rc = stage(h, B[GT_AP], jb->array_parent, (size_t)J)) return rc;
      if (int rc = stage(h, B[GT_APFLAGS], jb->ap_flags, (size_t)J)) return rc;
      if (int rc = stage(h, B[GT_APDEAD], jb->ap_deadline_sec, (size_t)J * 8)) return rc;
      if (int rc = stage(h, B[GT_APRUN], jb->ap_running, (size_t)J * 8)) return rc;
      if (int rc = stage(h, B[GT_APLIM], jb->ap_run_limit, (size_t)J * 8)) return rc;
    }
    if (E) {
      if (int rc = stage(h, B[GT_EVDEPENDENT], ev->dependent_job_id, (size_t)E * 4)) return rc;
      if (int rc = stage(h, B[GT_EVDEPENDEE], ev->dependee_job_id, (size_t)E * 4)) return rc;
      if (int rc = stage(h, B[GT_EVSEC], ev->event_sec, (size_t)E * 8)) return rc;
    }
    const unsigned grid = (unsigned)((J + kGateChunk - 1) / kGateChunk);
    const u32 waves = grid * (kGateBlock / 64);
    if (claims) HIPCHK(h, B[GT_FIRST].ensure((size_t)D * 4));
    HIPCHK(h, B[GT_CODE].ensure((size_t)J));
    HIPCHK(h, B[GT_READYOUT].ensure((size_t)J * 8));
    HIPCHK(h, B[GT_ERASED].ensure((size_t)D));
    HIPCHK(h, B[GT_WAVES].ensure((size_t)waves * 4));
    HIPCHK(h, B[GT_TOTAL].ensure(4));
    HIPCHK(h, B[GT_PENDING].ensure((size_t)J * 4));
    GateParams P{};
    P.J = J; P.D = (u32)D; P.E = (u32)E; P.now = now;
    P.job_id = B[GT_JOBID].as<u32>();
    P.held = jb->held ? B[GT_HELD].as<uint8_t>() : nullptr;
    P.begin = jb->begin_sec ? B[GT_BEGIN].as<i64>() : nullptr;
    P.is_or = S.has_deps ? B[GT_ISOR].as<uint8_t>() : nullptr; P.ready = B[GT_READY].as<i64>();
    P.dep_off = D ? B[GT_DEPOFF].as<u64>() : nullptr; P.dep_job = B[GT_DEPJOB].as<u32>(); P.dep_delay = B[GT_DELAY].as<u64>();
    P.array_parent = S.has_array ? B[GT_AP].as<uint8_t>() : nullptr;
    P.ap_flags = B[GT_APFLAGS].as<uint8_t>(); P.ap_deadline = B[GT_APDEAD].as<i64>(); P.ap_running = B[GT_APRUN].as<u64>(); P.ap_limit = B[GT_APLIM].as<u64>();
    P.ev_dependent = B[GT_EVDEPENDENT].as<u32>(); P.ev_dependee = B[GT_EVDEPENDEE].as<u32>(); P.ev_sec = B[GT_EVSEC].as<i64>();
    P.first_ev = claims ? B[GT_FIRST].as<u32>() : nullptr;
    P.code = B[GT_CODE].as<uint8_t>(); P.ready_out = B[GT_READYOUT].as<i64>(); P.erased = B[GT_ERASED].as<uint8_t>();
    P.wave_count = B[GT_WAVES].as<u32>(); P.pending = B[GT_PENDING].as<u32>();
    P.counts = B[GT_COUNTS].as<unsigned long long>();
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    if (claims) HIPCHK(h, hipMemsetAsync(P.first_ev, 0xFF, (size_t)D * 4, h->stream));
    if (E) {
      hipLaunchKernelGGL(k_gate_events, dim3((unsigned)((E + kGateBlock - 1) / kGateBlock)), dim3(kGateBlock), 0, h->stream, P);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_gate_jobs, dim3(grid), dim3(kGateBlock), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    scan_counts(h->stream, P.wave_count, waves, B[GT_TOTAL].as<u32>());
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gate_scatter, dim3(grid), dim3(kGateBlock), 0, h->stream, (const uint8_t*)P.code, J, (const u32*)P.wave_count, P.pending);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipMemcpyAsync(out->code, P.code, (size_t)J, hipMemcpyDeviceToHost, h->stream));
    if (out->ready_sec) HIPCHK(h, hipMemcpyAsync(out->ready_sec, P.ready_out, (size_t)J * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->dep_erased && D) HIPCHK(h, hipMemcpyAsync(out->dep_erased, P.erased, (size_t)D, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(counts, B[GT_COUNTS].p, sizeof counts, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&total, B[GT_TOTAL].p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (total > J) return fail(h, CNS_ERR_HIP, "cns_gate_pending: the compaction counted more rows than the queue has");
    if (total) {   // the list's length is known only now: the tail of out->pending is not touched
      HIPCHK(h, hipMemcpyAsync(out->pending, P.pending, (size_t)total * 4, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  } else {
    counts[17] = E;   // an empty pending map: no event finds its job (:1363)
  }
  *out->num_pending = total;
  if (out->counts) memcpy(out->counts, counts, 16 * sizeof(u64));
  if (out->ev_stats) {   // a repeat finds its entry in the list as uploaded, and erased in the reference: no such dependency
    out->ev_stats[0] = counts[16]; out->ev_stats[1] = counts[17]; out->ev_stats[2] = E - counts[16] - counts[17];
  }
  if (kernel_ms) *kernel_ms = ms;
  return CNS_OK;
}

int cns_gate_pending(cns_handle* h, int64_t now_sec, const cns_gate_jobs* jobs, const cns_gate_events* ev, const cns_gate_out* out, double* kernel_ms) {
  if (!h || !jobs || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_gate_pending: null argument");
  if (kernel_ms) *kernel_ms = 0.0;
  const int rc = gate_impl(h, now_sec, jobs, ev, out, kernel_ms);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_gate_shape(uint32_t* job_chunk, uint32_t* lane_max_deps, uint32_t* scan_span) {
  if (job_chunk) *job_chunk = kGateChunk;
  if (lane_max_deps) *lane_max_deps = kGateLaneMax;
  if (scan_span) *scan_span = kGateScanSpan;
  return CNS_OK;
}
