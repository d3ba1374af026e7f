// Host side of include/crane_gpu_commit/commit_check.h.  Included by engine.hip inside extern "C".
// Host work: validation of the caller's lists in the pass that copies them (every affected reservation's node list sorted on the way: a
// node twice shows as two equal neighbours, and membership on the device is a bisection), the reservation -> affected-slot table, the
// buffers.  Every test of a job against a node, a reservation or a running job runs on the device (commit_kernels.inc), on the
// cycle's results where they are: the queue's JobTable, cns_engine::q (results: start, reason, the node of every record; and
// raw[JR_PLACE_OFF]: the place offsets), both read only.  Everything the call writes lives in cns_engine::d_cc.  No CPU fallback.

static int commit_impl(cns_handle* h, const cns_commit_events* ev, const cns_commit_jobs* jb, const cns_commit_out* out, double* kernel_ms) {
  const u64 J = jb->num_jobs;
  const u32 N = h->lay.N, V = h->rlay.V;
  const u32 E = ev ? ev->num_node_events : 0, A = ev ? ev->num_affected_resv : 0;
  if (J && (!jb->time_limit_sec || !out->code)) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: missing array");

  // ---- node events: offsets ascending, nodes of the snapshot ----
  u64 entries = 0;
  if (E) {
    if (!ev->ev_time_sec || !ev->ev_offsets) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: node events without times or offsets");
    if (const u64 e = cns_csr::first_decrease(ev->ev_offsets, E); e < E)   // (this call reports a decrease before the first offset)
      return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ev_offsets decrease at event " + std::to_string(e));
    if (ev->ev_offsets[0] != 0) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ev_offsets[0] != 0");
    entries = ev->ev_offsets[E];
    if (entries && !ev->ev_nodes) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ev_offsets without ev_nodes");
    if (entries > 0xFFFFFF00ull) return fail(h, CNS_ERR_UNSUPPORTED, "cns_commit_check: more than 2^32 - 256 (event, node) entries");
    for (u64 x = 0; x < entries; ++x)
      if (ev->ev_nodes[x] >= N) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ev_nodes[" + std::to_string(x) + "] is no node of the snapshot");
  }
  // ---- affected reservations: distinct indices of the cycle's table, node lists sorted, a node once ----
  std::vector<u32> slot, ar_sorted;
  if (A) {
    if (!ev->ar_resv || !ev->ar_exists || !ev->ar_end_sec || !ev->ar_offsets) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: affected reservations with a missing array");
    const auto ao = cns_csr::check_offsets(ev->ar_offsets, A);
    if (ao.what == cns_csr::Offsets::FirstNot0) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ar_offsets[0] != 0");
    if (ao.what == cns_csr::Offsets::Decreases) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ar_offsets decrease at entry " + std::to_string(ao.index));
    const u64 L = ev->ar_offsets[A];
    if (L && !ev->ar_nodes) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ar_offsets without ar_nodes");
    slot.assign(V, kCcNoSlot);
    for (u32 a = 0; a < A; ++a) {
      const u32 v = ev->ar_resv[a];
      if (v >= V) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: ar_resv[" + std::to_string(a) + "] is no reservation of the cycle");
      if (slot[v] != kCcNoSlot) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: reservation " + std::to_string(v) + " is named twice in ar_resv");
      slot[v] = a;
    }
    ar_sorted.resize(L);
    const auto al = cns_csr::sort_lists(ev->ar_offsets, ev->ar_nodes, ar_sorted.data(), 0, A, N);
    if (al.what == cns_csr::Lists::OutOfBound)
      return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: the node list of ar_resv[" + std::to_string(al.list) + "] names a node outside the snapshot");
    if (al.what == cns_csr::Lists::Repeated)
      return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: the node list of ar_resv[" + std::to_string(al.list) + "] names node " + std::to_string(al.value) + " twice");
  }
  // ---- preempted lists: offsets ascending, running references inside the running table ----
  const bool has_pre = J && jb->preempt_offsets != nullptr;
  u64 PL = 0;
  if (has_pre) {
    const auto po = cns_csr::check_offsets(jb->preempt_offsets, J);
    if (po.what == cns_csr::Offsets::FirstNot0) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: preempt_offsets[0] != 0");
    if (po.what == cns_csr::Offsets::Decreases) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: preempt_offsets decrease at job " + std::to_string(po.index));
    PL = jb->preempt_offsets[J];
    if (PL && !jb->preempted) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: preempt_offsets without preempted");
    for (u64 x = 0; x < PL; ++x) {
      const u32 r = jb->preempted[x];
      if (r & CNS_PREEMPT_REF_PENDING) continue;
      if (r >= jb->num_running) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: preempted[" + std::to_string(x) + "] is no running job");
      if (!jb->running_alive) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: running references without running_alive");
    }
  }

  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_cc;
  HIPCHK(h, B[CC_COUNTS].ensure(8 * sizeof(u64)));
  HIPCHK(h, hipMemsetAsync(B[CC_COUNTS].p, 0, 8 * sizeof(u64), h->stream));
  float ms = 0;
  if (J) {
    if (entries) {
      if (int rc = stage(h, B[CC_EVTIME], ev->ev_time_sec, (size_t)E * 8)) return rc;
      if (int rc = stage(h, B[CC_EVOFF], ev->ev_offsets, ((size_t)E + 1) * 8)) return rc;
      if (int rc = stage(h, B[CC_EVNODES], ev->ev_nodes, (size_t)entries * 4)) return rc;
      HIPCHK(h, B[CC_CHANGE].ensure((size_t)N * 8));
    }
    if (A) {
      if (int rc = stage(h, B[CC_SLOT], slot.data(), (size_t)V * 4)) return rc;
      if (int rc = stage(h, B[CC_AREX], ev->ar_exists, (size_t)A)) return rc;
      if (int rc = stage(h, B[CC_AREND], ev->ar_end_sec, (size_t)A * 8)) return rc;
      if (int rc = stage(h, B[CC_AROFF], ev->ar_offsets, ((size_t)A + 1) * 8)) return rc;
      if (int rc = stage(h, B[CC_ARNODES], ar_sorted.data(), ar_sorted.size() * 4)) return rc;
    }
    if (int rc = stage(h, B[CC_LIMIT], jb->time_limit_sec, (size_t)J * 8)) return rc;
    if (jb->reservation) { if (int rc = stage(h, B[CC_RESV], jb->reservation, (size_t)J * 4)) return rc; }
    if (jb->gone) { if (int rc = stage(h, B[CC_GONE], jb->gone, (size_t)J)) return rc; }
    if (has_pre) {
      if (int rc = stage(h, B[CC_PREOFF], jb->preempt_offsets, ((size_t)J + 1) * 8)) return rc;
      if (int rc = stage(h, B[CC_PRE], jb->preempted, (size_t)PL * 4)) return rc;
      if (int rc = stage(h, B[CC_ALIVE], jb->running_alive, jb->running_alive ? (size_t)jb->num_running : 0)) return rc;
    }
    HIPCHK(h, B[CC_CODE].ensure((size_t)J));
    const char* rb = h->q.results.as<char>();
    CcParams P{};
    P.J = J; P.N = N; P.V = V; P.A = A; P.R = jb->running_alive ? jb->num_running : 0;
    P.start = (const i64*)(rb + h->q.ro.start); P.reason = (const uint8_t*)(rb + h->q.ro.reason);
    P.place_off = h->q.raw[JR_PLACE_OFF].as<u64>(); P.place_node = (const u32*)(rb + h->q.ro.node);
    P.limit = B[CC_LIMIT].as<i64>();
    P.resv = jb->reservation ? B[CC_RESV].as<u32>() : nullptr;
    P.gone = jb->gone ? B[CC_GONE].as<uint8_t>() : nullptr;
    P.change = entries ? B[CC_CHANGE].as<i64>() : nullptr;
    P.resv_slot = A ? B[CC_SLOT].as<u32>() : nullptr;
    P.ar_exists = B[CC_AREX].as<uint8_t>(); P.ar_end = B[CC_AREND].as<i64>(); P.ar_off = B[CC_AROFF].as<u64>(); P.ar_nodes = B[CC_ARNODES].as<u32>();
    P.pre_off = has_pre ? B[CC_PREOFF].as<u64>() : nullptr; P.pre = B[CC_PRE].as<u32>(); P.alive = B[CC_ALIVE].as<uint8_t>();
    P.code = B[CC_CODE].as<uint8_t>(); P.counts = B[CC_COUNTS].as<unsigned long long>();
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    if (entries) {
      hipLaunchKernelGGL(k_fill_i64, dim3((N + kCcBlock - 1) / kCcBlock), dim3(kCcBlock), 0, h->stream, B[CC_CHANGE].as<i64>(), N, kCcNever);
      HIPCHK(h, hipGetLastError());
      hipLaunchKernelGGL(k_cc_fold, dim3((unsigned)((entries + kCcBlock - 1) / kCcBlock)), dim3(kCcBlock), 0, h->stream, (const i64*)B[CC_EVTIME].as<i64>(),
                         (const u64*)B[CC_EVOFF].as<u64>(), (const u32*)B[CC_EVNODES].as<u32>(), E, (u32)entries, N, B[CC_CHANGE].as<i64>());
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cc_check, dim3((unsigned)((J + kCcChunk - 1) / kCcChunk)), dim3(kCcBlock), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipMemcpyAsync(out->code, P.code, (size_t)J, hipMemcpyDeviceToHost, h->stream));
  }
  u64 counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(h, hipMemcpyAsync(counts, B[CC_COUNTS].p, sizeof counts, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the sorted lists and the slot table are local vectors)
  if (J) HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (out->counts) memcpy(out->counts, counts, sizeof counts);
  if (kernel_ms) *kernel_ms = ms;
  return CNS_OK;
}

int cns_commit_check(cns_handle* h, const cns_commit_events* ev, const cns_commit_jobs* jobs, const cns_commit_out* out, double* kernel_ms) {
  if (!h || !jobs || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: null argument");
  if (kernel_ms) *kernel_ms = 0.0;
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_commit_check before a successful cycle");
  if (jobs->num_jobs != h->q.J)
    return fail(h, CNS_ERR_INVALID_ARG, "cns_commit_check: num_jobs " + std::to_string(jobs->num_jobs) + " is not the last cycle's " + std::to_string(h->q.J));
  const int rc = commit_impl(h, ev, jobs, out, kernel_ms);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_commit_shape(uint32_t* job_chunk, uint32_t* lane_max_nodes) {
  if (job_chunk) *job_chunk = kCcChunk;
  if (lane_max_nodes) *lane_max_nodes = kCcLaneMax;
  return CNS_OK;
}
