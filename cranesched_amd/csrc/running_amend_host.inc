// Host side of include/crane_gpu_amend/running_amend.h.  Included by engine.hip inside extern "C", behind running_host.inc and
// resvq_host.inc.  Host work: the input rules and the sort of the K amend ids (running_amend_check_host.inc), the buffers, the launches.
// Every row is visited and every table entry refilled on the device (running_amend_kernels.inc).  The call writes the copy of the end
// column at d_rl[RL_WEND] and the copy of the per-slot end times at d_rl[RL_RNEND] and swaps them in behind its one synchronize, so a
// call that fails leaves the ledger and the tables as they were.  One wait: the found bytes and the count go back to the caller.
// No CPU fallback.

static int amend_impl(cns_handle* h, const cns_running_amend_out* out, const std::vector<u32>& sorted_ids, const std::vector<i64>& sorted_ends,
                      const std::vector<u32>& order) {
  const u32 K = (u32)sorted_ids.size(), R = h->rl_R, A = h->rl_A;
  const bool tables = h->rl_dev;          // the per-slot tables are the ledger's: refill them
  const u32 M = tables ? h->rl_M : 0;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_rl;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (int rc = stage(h, B[RL_AMID], sorted_ids.data(), (size_t)K * 4)) return rc;
  if (int rc = stage(h, B[RL_AMEND], sorted_ends.data(), (size_t)K * 8)) return rc;
  HIPCHK(h, B[RL_FOUND].ensure(K));
  HIPCHK(h, hipMemsetAsync(B[RL_FOUND].p, 0, K, h->stream));
  HIPCHK(h, B[RL_TOT].ensure(8 * sizeof(u32)));
  HIPCHK(h, hipMemsetAsync(B[RL_TOT].p, 0, 8 * sizeof(u32), h->stream));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  u32* tot = B[RL_TOT].as<u32>();
  if (R) {
    const u32 grid = (R + kRunChunk - 1) / kRunChunk, waves = grid * (kRunBlock / 64);
    HIPCHK(h, B[RL_WEND].ensure((size_t)R * 8));
    HIPCHK(h, B[RL_WROWS0].ensure((size_t)waves * 4));
    RunAmend P;
    memset(&P, 0, sizeof P);
    P.R = R; P.K = K;
    P.id = B[RL_ID].as<u32>(); P.end = B[RL_END].as<i64>();
    P.am_id = B[RL_AMID].as<u32>(); P.am_end = B[RL_AMEND].as<i64>(); P.found = B[RL_FOUND].as<uint8_t>();
    P.end_copy = B[RL_WEND].as<i64>(); P.wave_hits = B[RL_WROWS0].as<u32>();
    hipLaunchKernelGGL(k_run_amend, dim3(grid), dim3(kRunBlock), 0, h->stream, P);
    scan_counts(h->stream, P.wave_hits, waves, tot + 0);
    HIPCHK(h, hipGetLastError());
    if (M) {
      HIPCHK(h, B[RL_RNEND].ensure((size_t)M * sizeof(i64)));
      RunRefill F;
      memset(&F, 0, sizeof F);
      F.M = M; F.R = R; F.A = A;
      F.vals = h->d_rp[RP_VALS].as<u32>(); F.off = B[RL_OFF].as<u32>(); F.end = P.end_copy;
      F.rn_end_old = h->d_rn_end.as<i64>(); F.rn_end = B[RL_RNEND].as<i64>();
      hipLaunchKernelGGL(k_run_refill, dim3((M + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, F);
      HIPCHK(h, hipGetLastError());
    }
  }
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  u32 hits = 0;
  std::vector<uint8_t> found(K);
  HIPCHK(h, hipMemcpyAsync(&hits, tot, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(found.data(), B[RL_FOUND].p, K, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the staging vectors are free again; the copies are complete)
  if (hits > R) return fail(h, CNS_ERR_HIP, "cns_running_amend_ends: more rows were written than the ledger holds");
  float a = 0, b = 0, c = 0;
  HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIPCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  HIPCHK(h, hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
  // ---- success: the copies become the ledger's end column and the tables' end times ----
  if (R) run_swap(B[RL_END], B[RL_WEND]);
  if (R && M) run_swap(h->d_rn_end, B[RL_RNEND]);
  h->rp_index = h->rp_call = false;   // the index of a cycle with preemption carries entry ends: the next such cycle builds it again
  h->am_timing.h2d_ms = a; h->am_timing.kernels_ms = b; h->am_timing.d2h_ms = c;
  h->am_timing.rows = R; h->am_timing.pairs = M;
  for (u32 i = 0; i < K; ++i) out->found[order[i]] = found[i];
  if (out->num_amended) *out->num_amended = hits;
  return CNS_OK;
}

int cns_running_amend_ends(cns_handle* h, const cns_running_amend* in, const cns_running_amend_out* out) {
  if (!h || !in) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_amend_ends: null argument");
  run_drop_if_stale(h);
  std::vector<u32> sorted_ids, order;
  std::vector<i64> sorted_ends;
  if (const auto v = cns_running::check_amend(h->rl_have && h->have_nodes, in, out, &sorted_ids, &sorted_ends, &order)) return fail(h, v.code, v.msg);
  if (!in->num_amend) return CNS_OK;   // nothing to change, nothing written
  const int rc = amend_impl(h, out, sorted_ids, sorted_ends, order);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_running_amend_get_timing(const cns_handle* h, cns_running_amend_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->am_timing;
  return CNS_OK;
}

int cns_resvq_set_state_resident(cns_handle* h, const cns_resv_soa* resv) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_set_state_resident: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_resvq_set_state_resident before cns_set_nodes");
  run_drop_if_stale(h);
  if (!h->rl_have) return fail(h, CNS_ERR_STATE, "cns_resvq_set_state_resident before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)");
  h->rq_have = false;
  RqRunning side;   // the ledger where it is: rows validated by cns_running_seed, admitted rows name nodes of the cycle's snapshot
  side.end = h->d_rl[RL_END].as<i64>(); side.off = h->d_rl[RL_OFF].as<u32>(); side.node = h->d_rl[RL_NODE].as<u32>();
  side.jobs = h->rl_R; side.allocs = h->rl_A;
  const int rc = resvq_set_state_tables(h, side, resv, "cns_resvq_set_state_resident");
  if (rc != 0) drain(h);
  return rc;
}
