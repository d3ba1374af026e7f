// Host side of include/crane_gpu_running/running_attrs.h.  Included by engine.hip inside extern "C", behind running_preempt_host.inc.
// Host work: the input rules (running_attrs_check_host.inc), the buffers, the launches.  The columns travel through a seed and a cycle
// boundary inside seed_impl / advance_impl (running_host.inc); the per-row sums, the account check, the presence flags and the
// per-account CSR of cns_priority_order_resident are device work (running_attrs_kernels.inc) in front of the kernels of
// priority_kernels.hip, whose running pointers are bound to cns_engine::d_ra and whose launches are prio_launch's (priority_host.inc).
// No pass over the running jobs runs on a host thread.  No CPU fallback.

int cns_running_seed_attrs(cns_handle* h, const cns_running_soa* rn, const uint32_t* job_ids, const cns_running_attrs* attrs) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_seed_attrs: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_running_seed_attrs before cns_set_nodes");
  uint64_t R = 0, A = 0;
  if (const auto v = cns_running::check_seed(rn, job_ids, h->lay.N, &R, &A)) return fail(h, v.code, v.msg);
  if (const auto v = cns_running::check_seed_attrs(R, attrs)) return fail(h, v.code, v.msg);
  const int rc = seed_impl(h, rn, job_ids, (u32)R, (u32)A, attrs, true);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_running_advance_attrs(cns_handle* h, const cns_running_step* in, const cns_running_attrs* queue_attrs, const cns_running_step_out* out) {
  if (!h || !in) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_advance_attrs: null argument");
  run_drop_if_stale(h);
  cns_running::Facts F;
  F.have_ledger = h->rl_have && h->have_nodes;
  F.have_cycle = h->have_run; F.preempt_cycle = h->run_preempt && !h->run_preempt_rl;
  F.cycle_jobs = h->q.J; F.cycle_now = h->last_now; F.cycle_places = h->q.places;
  F.ledger_jobs = h->rl_R; F.ledger_allocs = h->rl_A;
  std::vector<u32> sorted_ids, order;
  if (const auto v = cns_running::check_step(F, in, out, &sorted_ids, &order)) return fail(h, v.code, v.msg);
  if (const auto v = cns_running::check_step_after_preempt(h->have_run && h->run_preempt_rl, in)) return fail(h, v.code, v.msg);
  if (const auto v = cns_running::check_step_attrs(h->ra_have, in, queue_attrs)) return fail(h, v.code, v.msg);
  const int rc = advance_impl(h, in, out, sorted_ids, order, queue_attrs, true);
  if (rc != 0) drain(h);
  return rc;
}

// RA_NODENUM, RA_CPU, RA_MEM and the two words of RA_SUMFLAG for the current ledger; launches only, once per ledger state
static int ra_sums(cns_handle* h) {
  if (h->ra_sums) return 0;
  DevBuf* C = h->d_ra;
  const u32 R = h->rl_R;
  HIPCHK(h, C[RA_NODENUM].ensure((size_t)std::max<u32>(R, 1) * 4));
  HIPCHK(h, C[RA_CPU].ensure((size_t)std::max<u32>(R, 1) * 8)); HIPCHK(h, C[RA_MEM].ensure((size_t)std::max<u32>(R, 1) * 8));
  HIPCHK(h, C[RA_SUMFLAG].ensure(8));
  HIPCHK(h, hipMemsetAsync(C[RA_SUMFLAG].p, 0xFF, 8, h->stream));
  if (R) {
    RaSums S;
    memset(&S, 0, sizeof S);
    S.R = R; S.A = h->rl_A; S.off = h->d_rl[RL_OFF].as<u32>(); S.res = h->d_rl[RL_RES].as<Res>();
    S.node_num = C[RA_NODENUM].as<u32>(); S.cpu = C[RA_CPU].as<i64>(); S.mem = C[RA_MEM].as<u64>(); S.flag = C[RA_SUMFLAG].as<u32>();
    hipLaunchKernelGGL(k_ra_sums, dim3((R + kRunChunk - 1) / kRunChunk), dim3(kRunBlock), 0, h->stream, S);
    HIPCHK(h, hipGetLastError());
  }
  h->ra_sums = true;
  return 0;
}

int cns_running_get_attrs(cns_handle* h, const cns_running_attrs_out* o) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_get_attrs: null handle");
  run_drop_if_stale(h);
  if (const auto v = cns_running::check_get_attrs(h->rl_have, h->ra_have, o, h->rl_R)) return fail(h, v.code, v.msg);
  const u32 R = h->rl_R;
  if (o->num_jobs) *o->num_jobs = R;
  HIPCHK(h, hipSetDevice(h->device));
  if (o->node_num || o->alloc_cpu_raw || o->alloc_mem) {
    if (int rc = ra_sums(h)) { drain(h); return rc; }
  }
  DevBuf* C = h->d_ra;
  const std::tuple<void*, int, size_t> copies[] = {
      {o->start_sec, RA_START, (size_t)R * 8}, {o->qos, RA_QOS, (size_t)R * 4}, {o->qos_priority, RA_QPRIO, (size_t)R * 4}, {o->partition_priority, RA_PART, (size_t)R * 4},
      {o->account, RA_ACCT, (size_t)R * 4}, {o->node_num, RA_NODENUM, (size_t)R * 4}, {o->alloc_cpu_raw, RA_CPU, (size_t)R * 8}, {o->alloc_mem, RA_MEM, (size_t)R * 8}};
  for (const auto& [dst, slot, bytes] : copies)
    if (dst && bytes) HIPCHK(h, hipMemcpyAsync(dst, C[slot].p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return CNS_OK;
}

static int priority_order_resident_impl(cns_handle* h, int64_t now_sec, const cns_priority_config* cfg, u32 A, const cns_prio_pending_soa* pd, uint32_t* order_out,
                                        double* priority_out) {
  const u32 J = pd->num_jobs, R = h->rl_R;
  DevBuf* C = h->d_ra;
  DevBuf* pb = h->d_prio;
  // ---- the running side, from the ledger: sums (once per ledger state), the account check, presence, the keys of the CSR ----
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (int rc = ra_sums(h)) return rc;
  if (int rc = prio_stage_pending(h, pd, J)) return rc;
  HIPCHK(h, pb[PR_PRESENT].ensure(std::max<u32>(A, 1)));
  HIPCHK(h, hipMemsetAsync(pb[PR_PRESENT].p, 0, std::max<u32>(A, 1), h->stream));
  HIPCHK(h, C[RA_FLAG].ensure(4));
  HIPCHK(h, hipMemsetAsync(C[RA_FLAG].p, 0xFF, 4, h->stream));
  HIPCHK(h, C[RA_K0].ensure((size_t)R * 8)); HIPCHK(h, C[RA_K1].ensure((size_t)R * 8));
  HIPCHK(h, C[RA_V0].ensure((size_t)R * 4)); HIPCHK(h, C[RA_V1].ensure((size_t)R * 4));
  HIPCHK(h, C[RA_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(R, kSortTile))));
  HIPCHK(h, pb[PR_ACCOFF].ensure(((size_t)A + 1) * 4));
  u64* kin = C[RA_K0].as<u64>(); u64* kout = C[RA_K1].as<u64>();
  u32* vin = C[RA_V0].as<u32>(); u32* vout = C[RA_V1].as<u32>();
  {
    RaAccounts K;
    memset(&K, 0, sizeof K);
    K.R = R; K.J = J; K.A = A;
    K.r_account = C[RA_ACCT].as<u32>(); K.p_account = pb[PR_ACCT].as<u32>(); K.present = pb[PR_PRESENT].as<uint8_t>(); K.keys = kin; K.flag = C[RA_FLAG].as<u32>();
    hipLaunchKernelGGL(k_ra_accounts, dim3((std::max(J, R) + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, K);
    HIPCHK(h, hipGetLastError());
  }
  u32 flags[3] = {cns_running::kNoRow, cns_running::kNoRow, cns_running::kNoRow};   // account; negative cpu sum; a sum outside its type
  HIPCHK(h, hipMemcpyAsync(&flags[0], C[RA_FLAG].p, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&flags[1], C[RA_SUMFLAG].p, 8, hipMemcpyDeviceToHost, h->stream));
  if (int rc = prio_scratch(h, J, R, A)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the one wait in front of the sorter's kernels: the flag words
  u32 row = 0;
  if (const int kind = cns_running::worst_row(flags[0], flags[1], flags[2], &row)) {
    if (kind == cns_running::kRowAccount) {
      u32 account = 0;
      if (row < R) HIPCHK(h, hipMemcpy(&account, C[RA_ACCT].as<u32>() + row, 4, hipMemcpyDeviceToHost));
      const auto v = cns_running::refuse_account_row(row, account, A);
      return fail(h, v.code, v.msg);
    }
    const auto v = cns_running::refuse_sum_row(row, kind);
    return fail(h, v.code, v.msg);
  }
  // ---- the per-account CSR: a stable argsort of the rows by account, the offsets as lower bounds ----
  sort_index_pairs(h->stream, R, cns_sort::key_passes(A ? A - 1 : 0), kin, vin, kout, vout, C[RA_HIST].as<u32>());
  hipLaunchKernelGGL(k_ra_accoff, dim3((u32)(((u64)A + 1 + kRunBlock - 1) / kRunBlock)), dim3(kRunBlock), 0, h->stream, (const u64*)kin, R, A, pb[PR_ACCOFF].as<u32>());
  HIPCHK(h, hipGetLastError());
  PrioParams P = prio_params(h, now_sec, cfg, J, R, A, pd->cached_priority != nullptr);
  P.r_start = C[RA_START].as<i64>(); P.r_qos = C[RA_QPRIO].as<u32>(); P.r_part = C[RA_PART].as<u32>(); P.r_node_num = C[RA_NODENUM].as<u32>();
  P.r_cpu_raw = C[RA_CPU].as<i64>(); P.r_mem = C[RA_MEM].as<u64>(); P.r_account = C[RA_ACCT].as<u32>();
  P.acc_jobs = vin;
  if (int rc = prio_launch(h, P, false, order_out, priority_out)) return rc;
  // bytes by construction: the pending side as in cns_priority_order; of a running job the sorter's kernels read 36 B twice, the terms
  // 4 + 16 B; in front of them the account pass reads 4 B and writes a key (8 B), every pass of the account sort moves 32 B, its iota 4 B
  // (the sums, once per ledger state, are not counted here)
  h->prio_bytes = (u64)J * (48 + 48 + 16 + 4 + 8ull * 32 + 4) + (u64)R * (36 + 36 + 4 + 16 + 12 + 4 + 32ull * cns_sort::key_passes(A ? A - 1 : 0)) +
                  (pd->cached_priority ? (u64)J * 8 : 0);
  return CNS_OK;
}

int cns_priority_order_resident(cns_handle* h, int64_t now_sec, const cns_priority_config* cfg, uint32_t num_accounts, const cns_prio_pending_soa* pd, uint64_t limit,
                                uint32_t* order_out, double* priority_out, uint64_t* num_ordered) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_priority_order_resident: null handle");
  run_drop_if_stale(h);
  if (const auto v = cns_running::check_order_resident(h->rl_have && h->have_nodes, h->ra_have, cfg, pd, order_out, priority_out, num_ordered)) return fail(h, v.code, v.msg);
  if (const auto v = cns_running::check_order_pending(pd, num_accounts)) return fail(h, v.code, v.msg);
  HIPCHK(h, hipSetDevice(h->device));
  h->prio_ms = 0.0; h->prio_bytes = 0;
  if (pd->num_jobs == 0) { *num_ordered = 0; return CNS_OK; }
  const int rc = priority_order_resident_impl(h, now_sec, cfg, num_accounts, pd, order_out, priority_out);
  if (rc != 0) { drain(h); return rc; }
  *num_ordered = std::min<uint64_t>(pd->num_jobs, limit);
  return CNS_OK;
}

int cns_running_select_preempt_attrs(cns_handle* h, int64_t now, const cns_job_soa* jobs, const cns_preempt_soa* pre, cns_placement_soa* out, cns_preempt_out* pout) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_select_preempt_attrs: null handle");
  if (!pre || !pre->enabled) return cns_running_select_preempt(h, now, jobs, pre, out, pout);
  run_drop_if_stale(h);
  cns_running::PreemptFacts F;
  F.have_nodes = h->have_nodes; F.have_ledger = h->rl_have && h->have_nodes; F.tables_are_ledgers = h->rl_dev; F.ledger_jobs = h->rl_R;
  if (const auto v = cns_running::check_select_preempt_attrs(F, h->ra_have, jobs, pre, out, pout)) return fail(h, v.code, v.msg);
  const int rc = running_select_preempt_impl(h, now, jobs, pre, out, pout, true);
  if (rc != 0) drain(h);
  return rc;
}
