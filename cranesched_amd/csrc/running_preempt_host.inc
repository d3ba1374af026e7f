// Host side of include/crane_gpu_running/running_preempt.h.  Included by engine.hip inside extern "C", behind running_host.inc.
// Host work: the input rules (running_preempt_check_host.inc), the sort of the few preempting ids, the buffers, the launches, and the
// cycle itself (engine.hip: pre_cycle, shared with cns_select_preempt; its host side: preempt_host.inc).  Which running job owns an entry, the entries of every job, the
// marks, the ends: all on the device (running_preempt_kernels.inc), from the ledger (cns_engine::d_rl) and the sorted pairs of the
// rebuild the per-slot tables came from (d_rp[RP_KEYS] / [RP_VALS]: run_commit keeps them).  No pass over the running jobs or the
// entries runs on a host thread.  Synchronisations in front of the cycle: one, for the flag word of the id check and the found bytes
// (the pair count is known from the rebuild); cns_upload_jobs behind it has its own, as in every cycle.  The resident d_rn_end is
// never written: the cycle is bound to the patched copy.  No CPU fallback.

// RP_ENTJOB, RP_ENTSLOT, RP_RJOFF, RP_RJENT for the current per-slot tables; launches only
static int rp_build_index(cns_handle* h) {
  DevBuf* P = h->d_rp;
  const u32 M = h->rl_M, R = h->rl_R;
  HIPCHK(h, P[RP_ENTJOB].ensure((size_t)std::max<u32>(M, 1) * 4)); HIPCHK(h, P[RP_ENTSLOT].ensure((size_t)std::max<u32>(M, 1) * 4));
  HIPCHK(h, P[RP_RJOFF].ensure(((size_t)R + 1) * 4)); HIPCHK(h, P[RP_RJENT].ensure((size_t)std::max<u32>(M, 1) * 4));
  HIPCHK(h, P[RP_K0].ensure((size_t)M * 8)); HIPCHK(h, P[RP_K1].ensure((size_t)M * 8));
  HIPCHK(h, P[RP_V0].ensure((size_t)M * 4)); HIPCHK(h, P[RP_V1].ensure((size_t)M * 4));
  HIPCHK(h, P[RP_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(M, kSortTile))));
  u64* kin = P[RP_K0].as<u64>(); u64* kout = P[RP_K1].as<u64>();
  u32* vin = P[RP_V0].as<u32>(); u32* vout = P[RP_V1].as<u32>();
  if (M) {
    RpIndex X;
    memset(&X, 0, sizeof X);
    X.M = M; X.R = R; X.A = h->rl_A;
    X.keys = P[RP_KEYS].as<u64>(); X.vals = P[RP_VALS].as<u32>(); X.off = h->d_rl[RL_OFF].as<u32>();
    X.ent_job = P[RP_ENTJOB].as<u32>(); X.ent_slot = P[RP_ENTSLOT].as<u32>(); X.skeys = kin; X.svals = vin;
    hipLaunchKernelGGL(k_rp_entries, dim3((M + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, X);
    // (row, entry) pairs sorted by row, stable: the entries of a row stay in ascending d
    sort_pairs(h->stream, M, cns_sort::key_passes(R ? R - 1 : 0), kin, vin, kout, vout, P[RP_HIST].as<u32>());
  }
  hipLaunchKernelGGL(k_rp_rows, dim3((std::max<u32>(M, R + 1) + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, (const u64*)kin, (const u32*)vin, M, R,
                     P[RP_RJOFF].as<u32>(), P[RP_RJENT].as<u32>());
  HIPCHK(h, hipGetLastError());
  return 0;
}

// from_attrs: cns_running_select_preempt_attrs (running_attrs_host.inc) — the running jobs' fields come from the ledger's columns, the
// rows are the ledger's by construction (no rn_job_id to upload or to check), the ids of the preempted rows are picked on the device
static int running_select_preempt_impl(cns_handle* h, int64_t now, const cns_job_soa* jobs, const cns_preempt_soa* pre, cns_placement_soa* out,
                                       cns_preempt_out* pout, bool from_attrs = false) {
  DevBuf* P = h->d_rp;
  const u32 R = h->rl_R, M = h->rl_M;
  HIPCHK(h, hipSetDevice(h->device));
  h->pre_t0 = std::chrono::steady_clock::now();
  h->rp_timing = cns_running_preempt_timing{};
  const bool build = !h->rp_index;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  const std::vector<u32> set = cns_running::preempting_sorted(pre->preempting_job_ids, pre->num_preempting);
  const u32 ns = (u32)set.size();
  h->rp_call = false;
  if (build) { if (int rc = rp_build_index(h)) return rc; }
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  if (!from_attrs) { if (int rc = stage(h, P[RP_GIVEN], R ? pre->rn_job_id : nullptr, (size_t)R * 4)) return rc; }
  if (int rc = stage(h, P[RP_SET], set.data(), (size_t)ns * 4)) return rc;
  HIPCHK(h, P[RP_FOUND].ensure(ns));
  if (ns) HIPCHK(h, hipMemsetAsync(P[RP_FOUND].p, 0, ns, h->stream));
  HIPCHK(h, P[RP_FLAG].ensure(4));
  HIPCHK(h, hipMemsetAsync(P[RP_FLAG].p, 0xFF, 4, h->stream));
  HIPCHK(h, P[RP_RJPRE].ensure(std::max<u32>(R, 1))); HIPCHK(h, P[RP_RJEND].ensure((size_t)std::max<u32>(R, 1) * 8));
  HIPCHK(h, P[RP_ENTEND].ensure((size_t)std::max<u32>(M, 1) * 8));
  if (R) {
    RpMark K;
    memset(&K, 0, sizeof K);
    K.R = R; K.nset = ns; K.now = now;
    K.ledger_id = h->d_rl[RL_ID].as<u32>(); K.ledger_end = h->d_rl[RL_END].as<i64>(); K.given_id = from_attrs ? K.ledger_id : P[RP_GIVEN].as<u32>();
    K.set = P[RP_SET].as<u32>(); K.rj_off = P[RP_RJOFF].as<u32>(); K.found = P[RP_FOUND].as<uint8_t>();
    K.rj_preempting = P[RP_RJPRE].as<uint8_t>(); K.rj_end = P[RP_RJEND].as<i64>(); K.flag = P[RP_FLAG].as<u32>();
    hipLaunchKernelGGL(k_rp_mark, dim3((R + kRunChunk - 1) / kRunChunk), dim3(kRunBlock), 0, h->stream, K);
  }
  if (M)
    hipLaunchKernelGGL(k_rp_patch, dim3((M + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, (const u32*)P[RP_ENTJOB].as<u32>(),
                       (const uint8_t*)P[RP_RJPRE].as<uint8_t>(), (const i64*)h->d_rn_end.as<i64>(), M, R, (i64)now, P[RP_ENTEND].as<i64>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  u32 flag = 0xFFFFFFFFu;
  std::vector<uint8_t> found(ns);
  HIPCHK(h, hipMemcpyAsync(&flag, P[RP_FLAG].p, 4, hipMemcpyDeviceToHost, h->stream));
  if (ns) HIPCHK(h, hipMemcpyAsync(found.data(), P[RP_FOUND].p, ns, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the one wait in front of the cycle: the id check and which ids of the set still run
  h->rp_index = true;
  {
    float a = 0, b = 0;
    HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    HIPCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    h->rp_timing.index_ms = build ? a : 0.0; h->rp_timing.mark_ms = b;
    h->rp_timing.entries = M; h->rp_timing.rows = R; h->rp_timing.index_built = build ? 1 : 0;
  }
  if (flag != 0xFFFFFFFFu) {
    u32 ledger_id = 0;
    if (flag < R) HIPCHK(h, hipMemcpy(&ledger_id, h->d_rl[RL_ID].as<u32>() + flag, 4, hipMemcpyDeviceToHost));
    const auto v = cns_running::refuse_row_id(flag, flag < R ? pre->rn_job_id[flag] : 0u, ledger_id);
    return fail(h, v.code, v.msg);
  }
  std::vector<u32> set_in;   // m_preempting_set_ without the ids that no longer run (JobScheduler.cpp:6545-6559)
  for (u32 i = 0; i < ns; ++i)
    if (found[i]) set_in.push_back(set[i]);
  struct PreCall { cns_engine* h; ~PreCall() { h->pre_call = false; h->rn_end_bound = nullptr; } } pre_call{h};   // (run_resident_once notes it: cns_probe refuses such a state)
  h->pre_call = true;
  if (int rc = cns_upload_jobs(h, jobs)) return rc;
  h->rp_call = true;
  h->rn_end_bound = P[RP_ENTEND].as<i64>();   // this call's cycle runs on the patched copy; the resident end times are not written
  // the job ids behind the few ledger rows the cycle preempted, without the caller's rn_job_id
  const PreRowIds pick_ids = [&](const std::vector<u32>& rows, std::vector<u32>& ids) -> int {
    const u32 n = (u32)rows.size();
    ids.assign(n, 0u);
    if (!n) return 0;
    DevBuf* C = h->d_ra;
    if (int rc2 = stage(h, C[RA_PICK], rows.data(), (size_t)n * 4)) return rc2;
    HIPCHK(h, C[RA_PICKED].ensure((size_t)n * 4));
    hipLaunchKernelGGL(k_ra_pick, dim3((n + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, (const u32*)C[RA_PICK].as<u32>(), n, (const u32*)h->d_rl[RL_ID].as<u32>(), R,
                       C[RA_PICKED].as<u32>());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(ids.data(), C[RA_PICKED].p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = pre_cycle(h, now, jobs, pre, out, pout, R, M, set_in, from_attrs ? "cns_running_select_preempt_attrs" : "cns_running_select_preempt", [&](PreParams& Q) -> int {
    DevBuf* B = h->d_pre;
    if (from_attrs) {   // three device-to-device copies into the buffers the cycle reads
      DevBuf* C = h->d_ra;
      HIPCHK(h, B[B_RJQOS].ensure((size_t)R * 4)); HIPCHK(h, B[B_RJQP].ensure((size_t)R * 4)); HIPCHK(h, B[B_RJSTART].ensure((size_t)R * 8));
      if (R) {
        HIPCHK(h, hipMemcpyAsync(B[B_RJQOS].p, C[RA_QOS].p, (size_t)R * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(B[B_RJQP].p, C[RA_QPRIO].p, (size_t)R * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(B[B_RJSTART].p, C[RA_START].p, (size_t)R * 8, hipMemcpyDeviceToDevice, h->stream));
      }
    } else {
      if (int rc2 = stage(h, B[B_RJQOS], pre->rn_qos, (size_t)R * 4)) return rc2;          // (as they are: ledger order is the caller's contract)
      if (int rc2 = stage(h, B[B_RJQP], pre->rn_qos_priority, (size_t)R * 4)) return rc2;
      if (int rc2 = stage(h, B[B_RJSTART], pre->rn_start_sec, (size_t)R * 8)) return rc2;
    }
    Q.rn_job = P[RP_ENTJOB].as<u32>(); Q.ent_slot = P[RP_ENTSLOT].as<u32>();
    Q.rj_qos = B[B_RJQOS].as<u32>(); Q.rj_qprio = B[B_RJQP].as<u32>(); Q.rj_start = B[B_RJSTART].as<i64>(); Q.rj_end = P[RP_RJEND].as<i64>();
    Q.rj_preempting = P[RP_RJPRE].as<uint8_t>(); Q.rj_off = P[RP_RJOFF].as<u32>(); Q.rj_ent = P[RP_RJENT].as<u32>();
    return 0;
  }, from_attrs ? &pick_ids : nullptr);
  if (rc == CNS_OK) h->run_preempt_rl = true;
  return rc;
}

int cns_running_select_preempt(cns_handle* h, int64_t now, const cns_job_soa* jobs, const cns_preempt_soa* pre, cns_placement_soa* out,
                               cns_preempt_out* pout) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_select_preempt: null handle");
  if (!pre || !pre->enabled) return cns_select_preempt(h, now, jobs, pre, out, pout);   // exactly cns_select, the set passes through
  run_drop_if_stale(h);
  cns_running::PreemptFacts F;
  F.have_nodes = h->have_nodes; F.have_ledger = h->rl_have && h->have_nodes; F.tables_are_ledgers = h->rl_dev; F.ledger_jobs = h->rl_R;
  if (const auto v = cns_running::check_select_preempt(F, jobs, pre, out, pout)) return fail(h, v.code, v.msg);
  const int rc = running_select_preempt_impl(h, now, jobs, pre, out, pout);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_debug_get_preempt_index(cns_handle* h, const cns_preempt_index_out* o) {
  if (!h || !o) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_preempt_index: null argument");
  if (!h->rl_have || !h->rl_dev || !h->rp_index || !h->rp_call)
    return fail(h, CNS_ERR_STATE, "cns_debug_get_preempt_index before a cns_running_select_preempt with preemption enabled on the current running tables");
  const u32 M = h->rl_M, R = h->rl_R;
  if (o->num_entries) *o->num_entries = M;
  if (o->num_rows) *o->num_rows = R;
  const bool ents = o->ent_job || o->ent_slot || o->ent_end || o->rj_ent, rows = o->rj_off || o->rj_end || o->rj_preempting;
  if ((ents && o->capacity_entries < M) || (rows && o->capacity_rows < R)) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_preempt_index: the arrays are smaller than the index");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* P = h->d_rp;
  const std::tuple<void*, int, size_t> copies[] = {
      {o->ent_job, RP_ENTJOB, (size_t)M * 4}, {o->ent_slot, RP_ENTSLOT, (size_t)M * 4}, {o->ent_end, RP_ENTEND, (size_t)M * 8}, {o->rj_off, RP_RJOFF, ((size_t)R + 1) * 4},
      {o->rj_ent, RP_RJENT, (size_t)M * 4}, {o->rj_end, RP_RJEND, (size_t)R * 8}, {o->rj_preempting, RP_RJPRE, (size_t)R}};
  for (const auto& [dst, slot, bytes] : copies)
    if (dst && bytes) HIPCHK(h, hipMemcpyAsync(dst, P[slot].p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return CNS_OK;
}

int cns_running_preempt_get_timing(const cns_handle* h, cns_running_preempt_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->rp_timing;
  return CNS_OK;
}
