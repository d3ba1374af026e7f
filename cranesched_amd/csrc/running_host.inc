// Host side of include/crane_gpu_running/running.h.  Included by engine.hip inside extern "C".
// Host work: the input rules (running_check_host.inc), the sort of the retire ids, the node -> slots CSR of the layout (uploaded when
// the layout changed), the buffers, the launches.  Every row and every allocation is moved, expanded, sorted and grouped on the device
// (running_kernels.inc).  The admit step reads the cycle's results where they are: the queue's JobTable, cns_engine::q (results: start,
// reason, the placement planes; raw[JR_LIMIT], raw[JR_PLACE_OFF]), read only.  Everything the calls write lives in cns_engine::d_rl;
// a call that succeeded swaps its copy of the ledger with the ledger and its per-slot tables with d_rn_off / d_rn_end / d_rn_res, so a
// refused call leaves all of them as they were.  No CPU fallback.

static void run_swap(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

// a changed num_nodes drops the ledger: its node indices name another cluster
static void run_drop_if_stale(cns_handle* h) {
  if (h->rl_have && h->rl_N != h->lay.N) h->rl_have = h->ra_have = h->ra_sums = false;
}

static RunLedger run_ledger(cns_handle* h, int first) {
  DevBuf* B = h->d_rl + first;
  return RunLedger{B[0].as<u32>(), B[1].as<i64>(), B[2].as<u32>(), B[3].as<u32>(), B[4].as<u32>(), B[5].as<Res>()};
}

// The attribute columns beside the ledger (include/crane_gpu_running/running_attrs.h; the calls: running_attrs_host.inc).  A seed or an
// advance that carries them writes the copy at d_ra[RA_WSTART..] and swaps it in behind run_commit, which by itself leaves a ledger
// without columns: that is what a plain call does.
static RaCols ra_cols(cns_handle* h, int first) {
  DevBuf* B = h->d_ra + first;
  return RaCols{B[0].as<i64>(), B[1].as<u32>(), B[2].as<u32>(), B[3].as<u32>(), B[4].as<u32>()};
}
static int ra_ensure_copy(cns_handle* h, u32 rows) {
  DevBuf* B = h->d_ra;
  HIPCHK(h, B[RA_WSTART].ensure((size_t)rows * 8));
  for (int k = RA_WQOS; k <= RA_WACCT; ++k) HIPCHK(h, B[k].ensure((size_t)rows * 4));
  return 0;
}
static void ra_commit(cns_handle* h) {
  for (int k = 0; k < 5; ++k) run_swap(h->d_ra[RA_START + k], h->d_ra[RA_WSTART + k]);
  h->ra_have = true;
}

// Layout::node_slots as a CSR on the device: derived again only when a snapshot was uploaded since
static int run_layout_csr(cns_handle* h) {
  if (h->rl_lay_gen == h->lay_gen) return 0;
  const auto& ns = h->lay.node_slots;
  std::vector<u32> off(ns.size() + 1, 0), flat;
  u32 fan = 1;
  for (size_t n = 0; n < ns.size(); ++n) {
    flat.insert(flat.end(), ns[n].begin(), ns[n].end());
    off[n + 1] = (u32)flat.size();
    fan = std::max<u32>(fan, (u32)ns[n].size());
  }
  if (int rc = upload(h, h->d_rl[RL_NSOFF], off)) return rc;
  if (int rc = upload_some(h, h->d_rl[RL_NS], flat)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (local vectors)
  h->rl_fan = fan;
  h->rl_lay_gen = h->lay_gen;
  return 0;
}

// The per-slot tables of the ledger copy at d_rl[first..] (R rows, A allocations) against the handle's current layout, into RL_RNOFF /
// RL_RNEND / RL_RNRES.  Synchronous.  *over_cap: a slot is above the time map's capacity.
static int run_rebuild(cns_handle* h, int first, u32 R, u32 A, u32* pairs, bool* over_cap) {
  DevBuf* B = h->d_rl;
  const u32 S = h->rlay.S;
  *pairs = 0; *over_cap = false;
  if (int rc = run_layout_csr(h)) return rc;
  if (const auto v = cns_running::check_pairs(A, h->rl_fan)) return fail(h, v.code, v.msg);
  const RunLedger L = run_ledger(h, first);
  HIPCHK(h, B[RL_TOT].ensure(8 * sizeof(u32)));
  RunExp E;
  memset(&E, 0, sizeof E);
  E.R = R; E.A = A; E.N = h->lay.N; E.V = h->rlay.V; E.P_real = h->lay.P_real;
  E.off = L.off; E.node = L.node; E.resv = L.resv;
  E.ns_off = B[RL_NSOFF].as<u32>(); E.ns = B[RL_NS].as<u32>();
  E.part_off = h->d_part_off.as<u32>(); E.slot_node = h->d_slot_node.as<u32>();
  const u32 grid = (A + kRunBlock - 1) / kRunBlock, waves = grid * (kRunBlock / 64);
  u32 M = 0;
  if (A) {
    HIPCHK(h, B[RL_WEXP].ensure((size_t)waves * 4));
    E.wave_cnt = B[RL_WEXP].as<u32>();
    hipLaunchKernelGGL(k_run_expand<false>, dim3(grid), dim3(kRunBlock), 0, h->stream, E);
    scan_counts(h->stream, E.wave_cnt, waves, B[RL_TOT].as<u32>() + 4);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&M, B[RL_TOT].as<u32>() + 4, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the number of pairs sizes the sort
    if ((u64)M > (u64)A * h->rl_fan) return fail(h, CNS_ERR_HIP, "the expansion counted more (slot, allocation) pairs than the layout allows");
  }
  HIPCHK(h, B[RL_K0].ensure((size_t)M * 8)); HIPCHK(h, B[RL_K1].ensure((size_t)M * 8));
  HIPCHK(h, B[RL_V0].ensure((size_t)M * 4)); HIPCHK(h, B[RL_V1].ensure((size_t)M * 4));
  HIPCHK(h, B[RL_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(M, kSortTile))));
  HIPCHK(h, B[RL_RNOFF].ensure(((size_t)S + 1) * 4));
  HIPCHK(h, B[RL_RNEND].ensure((size_t)std::max<u32>(M, 1) * sizeof(i64)));
  HIPCHK(h, B[RL_RNRES].ensure((size_t)std::max<u32>(M, 1) * sizeof(Res)));
  HIPCHK(h, B[RL_FLAG].ensure(4));
  HIPCHK(h, hipMemsetAsync(B[RL_FLAG].p, 0, 4, h->stream));
  u64* kin = B[RL_K0].as<u64>(); u64* kout = B[RL_K1].as<u64>();
  u32* vin = B[RL_V0].as<u32>(); u32* vout = B[RL_V1].as<u32>();
  if (M) {
    E.M = M; E.keys = kin; E.vals = vin;
    hipLaunchKernelGGL(k_run_expand<true>, dim3(grid), dim3(kRunBlock), 0, h->stream, E);
    HIPCHK(h, hipGetLastError());
    // (slot, entry) pairs sorted by slot, stable: inside a slot the entries stay in ledger order
    sort_pairs(h->stream, M, cns_sort::key_passes(S), kin, vin, kout, vout, B[RL_HIST].as<u32>());
    HIPCHK(h, hipGetLastError());
  }
  RunFill F;
  memset(&F, 0, sizeof F);
  F.M = M; F.S = S; F.R = R; F.A = A; F.tl_cap = kTlCap;
  F.keys = kin; F.vals = vin; F.off = L.off; F.end = L.end; F.res = L.res;
  F.rv_off = h->d_rv_off.as<u32>();
  F.rn_off = B[RL_RNOFF].as<u32>(); F.rn_end = B[RL_RNEND].as<i64>(); F.rn_res = B[RL_RNRES].as<Res>(); F.flag = B[RL_FLAG].as<u32>();
  hipLaunchKernelGGL(k_run_fill, dim3((std::max<u32>(M, S + 1) + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, F);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  u32 flag = 0;
  HIPCHK(h, hipMemcpyAsync(&flag, F.flag, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *pairs = M; *over_cap = flag != 0;
  h->rl_sorted_side = kin == B[RL_K0].as<u64>() ? 0 : 1;   // (run_commit keeps that side for cns_running_select_preempt)
  return 0;
}

static const char* const kRunOverCap = "too many running allocations / reservations on one node (1006, or 502 events with reservations); the ledger and the running tables stay as they were";

// the call's copy becomes the ledger, its per-slot tables the cycle's
static int run_commit(cns_handle* h, u32 R, u32 A, u32 M) {
  DevBuf* B = h->d_rl;
  for (int k = 0; k < 6; ++k) run_swap(B[RL_ID + k], B[RL_WID + k]);
  run_swap(h->d_rn_off, B[RL_RNOFF]); run_swap(h->d_rn_end, B[RL_RNEND]); run_swap(h->d_rn_res, B[RL_RNRES]);
  // the sorted (slot, allocation) pairs these tables came from stay alive beside them: position d of the pairs is entry d of the tables
  // (running_preempt_host.inc builds the index of a cycle with preemption from them; a later call that fails writes other buffers)
  run_swap(h->d_rp[RP_KEYS], B[RL_K0 + h->rl_sorted_side]); run_swap(h->d_rp[RP_VALS], B[RL_V0 + h->rl_sorted_side]);
  h->rl_M = M; h->rp_index = h->rp_call = false;
  h->ra_have = h->ra_sums = false;   // (the caller that carried the columns swaps them in behind this)
  (void)cns_snapshot::build_running(h->lay, h->rlay, nullptr, h->run);   // (no host copy of the entries: cns_select_preempt is refused)
  h->rl_have = h->rl_dev = true;
  h->rl_R = R; h->rl_A = A; h->rl_N = h->lay.N;
  float a = 0, b = 0, c = 0;
  HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIPCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  HIPCHK(h, hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
  h->rl_timing.h2d_ms = a; h->rl_timing.kernels_ms = b; h->rl_timing.d2h_ms = c;
  h->rl_timing.jobs = R; h->rl_timing.allocs = A; h->rl_timing.pairs = M;
  return CNS_OK;
}

static int seed_impl(cns_handle* h, const cns_running_soa* rn, const uint32_t* job_ids, u32 R, u32 A, const cns_running_attrs* attrs = nullptr, bool with_attrs = false) {
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_rl;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  std::vector<Res> res(A);
  for (u32 a = 0; a < A; ++a) res[a] = cns_snapshot::alloc_row(*rn, a);
  std::vector<u32> resv;
  if (R && !rn->reservation) resv.assign(R, CNS_RESV_NONE);
  static const u32 zero = 0;
  if (int rc = stage(h, B[RL_WID], job_ids, (size_t)R * 4)) return rc;
  if (int rc = stage(h, B[RL_WEND], R ? rn->end_sec : nullptr, (size_t)R * 8)) return rc;
  if (int rc = stage(h, B[RL_WRESV], R ? (rn->reservation ? rn->reservation : resv.data()) : nullptr, (size_t)R * 4)) return rc;
  if (int rc = stage(h, B[RL_WOFF], R ? rn->alloc_offsets : &zero, ((size_t)R + 1) * 4)) return rc;
  if (int rc = stage(h, B[RL_WNODE], R ? rn->alloc_node : nullptr, (size_t)A * 4)) return rc;
  if (int rc = stage(h, B[RL_WRES], res.data(), (size_t)A * sizeof(Res))) return rc;
  if (with_attrs) {
    DevBuf* C = h->d_ra;
    if (int rc = stage(h, C[RA_WSTART], R ? attrs->start_sec : nullptr, (size_t)R * 8)) return rc;
    if (int rc = stage(h, C[RA_WQOS], R ? attrs->qos : nullptr, (size_t)R * 4)) return rc;
    if (int rc = stage(h, C[RA_WQPRIO], R ? attrs->qos_priority : nullptr, (size_t)R * 4)) return rc;
    if (int rc = stage(h, C[RA_WPART], R ? attrs->partition_priority : nullptr, (size_t)R * 4)) return rc;
    if (int rc = stage(h, C[RA_WACCT], R ? attrs->account : nullptr, (size_t)R * 4)) return rc;
  }
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  u32 M = 0;
  bool over = false;
  if (int rc = run_rebuild(h, RL_WID, R, A, &M, &over)) return rc;   // (its synchronize: the local vectors, the caller's arrays)
  if (over) return fail(h, CNS_ERR_UNSUPPORTED, kRunOverCap);
  if (int rc = run_commit(h, R, A, M)) return rc;
  if (with_attrs) ra_commit(h);
  return CNS_OK;
}

int cns_running_seed(cns_handle* h, const cns_running_soa* rn, const uint32_t* job_ids) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_seed: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_running_seed before cns_set_nodes");
  uint64_t R = 0, A = 0;
  if (const auto v = cns_running::check_seed(rn, job_ids, h->lay.N, &R, &A)) return fail(h, v.code, v.msg);
  const int rc = seed_impl(h, rn, job_ids, (u32)R, (u32)A);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

// queue_attrs / with_attrs: cns_running_advance_attrs (the columns follow the rows); a plain call launches what it always did
static int advance_impl(cns_handle* h, const cns_running_step* in, const cns_running_step_out* out, const std::vector<u32>& sorted_ids,
                        const std::vector<u32>& order, const cns_running_attrs* queue_attrs = nullptr, bool with_attrs = false) {
  const u32 K = (u32)in->num_retire, R = h->rl_R, A = h->rl_A;
  const u64 J = in->num_jobs, places = J ? h->q.places : 0;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_rl;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (int rc = stage(h, B[RL_RET], sorted_ids.data(), (size_t)K * 4)) return rc;
  HIPCHK(h, B[RL_FOUND].ensure(K));
  if (K) HIPCHK(h, hipMemsetAsync(B[RL_FOUND].p, 0, K, h->stream));
  if (J) {
    if (int rc = stage(h, B[RL_JID], in->job_id, (size_t)J * 4)) return rc;
    if (in->admit) { if (int rc = stage(h, B[RL_ADMIT], in->admit, (size_t)J)) return rc; }
    if (in->reservation) { if (int rc = stage(h, B[RL_JRESV], in->reservation, (size_t)J * 4)) return rc; }
  }
  const u32 cap_rows = (u32)(R + J), cap_ents = (u32)(A + places);   // (running_check_host.inc: both fit 32 bits)
  HIPCHK(h, B[RL_WID].ensure((size_t)cap_rows * 4)); HIPCHK(h, B[RL_WEND].ensure((size_t)cap_rows * 8)); HIPCHK(h, B[RL_WRESV].ensure((size_t)cap_rows * 4));
  HIPCHK(h, B[RL_WOFF].ensure(((size_t)cap_rows + 1) * 4)); HIPCHK(h, B[RL_WNODE].ensure((size_t)cap_ents * 4)); HIPCHK(h, B[RL_WRES].ensure((size_t)cap_ents * sizeof(Res)));
  HIPCHK(h, B[RL_TOT].ensure(8 * sizeof(u32)));
  HIPCHK(h, hipMemsetAsync(B[RL_TOT].p, 0, 8 * sizeof(u32), h->stream));
  DevBuf* C = h->d_ra;
  if (with_attrs) {
    if (int rc = ra_ensure_copy(h, cap_rows)) return rc;
    HIPCHK(h, C[RA_ORIGIN].ensure((size_t)cap_rows * 4));
    if (J) {
      if (int rc = stage(h, C[RA_QQOS], queue_attrs->qos, (size_t)J * 4)) return rc;
      if (int rc = stage(h, C[RA_QQPRIO], queue_attrs->qos_priority, (size_t)J * 4)) return rc;
      if (int rc = stage(h, C[RA_QPART], queue_attrs->partition_priority, (size_t)J * 4)) return rc;
      if (int rc = stage(h, C[RA_QACCT], queue_attrs->account, (size_t)J * 4)) return rc;
    }
  }
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  u32* tot = B[RL_TOT].as<u32>();   // kept rows, kept entries, admitted rows, admitted entries
  RunSrc S;
  memset(&S, 0, sizeof S);
  S.D = run_ledger(h, RL_WID); S.cap_rows = cap_rows; S.cap_ents = cap_ents;
  if (R) {   // ---- retire: the ledger without the rows that carry a listed id ----
    const u32 grid = (R + kRunChunk - 1) / kRunChunk, waves = grid * (kRunBlock / 64);
    HIPCHK(h, B[RL_WROWS0].ensure((size_t)waves * 4)); HIPCHK(h, B[RL_WENTS0].ensure((size_t)waves * 4));
    S.n = R; S.L = run_ledger(h, RL_ID); S.src_ents = A;
    S.nret = K; S.ret = B[RL_RET].as<u32>(); S.found = B[RL_FOUND].as<uint8_t>();
    S.wave_rows = B[RL_WROWS0].as<u32>(); S.wave_ents = B[RL_WENTS0].as<u32>();
    S.base = nullptr;
    hipLaunchKernelGGL(k_run_keep<false>, dim3(grid), dim3(kRunBlock), 0, h->stream, S);
    scan_counts(h->stream, S.wave_rows, waves, tot + 0);
    scan_counts(h->stream, S.wave_ents, waves, tot + 1);
    hipLaunchKernelGGL(k_run_compact<false>, dim3(grid), dim3(kRunBlock), 0, h->stream, S);
    if (with_attrs) hipLaunchKernelGGL(k_ra_origin<false>, dim3(grid), dim3(kRunBlock), 0, h->stream, S, C[RA_ORIGIN].as<u32>());
    HIPCHK(h, hipGetLastError());
  }
  if (J) {   // ---- admit: the jobs of the last cycle that the commit loop started, behind the kept rows ----
    const u32 grid = (u32)((J + kRunChunk - 1) / kRunChunk), waves = grid * (kRunBlock / 64);
    HIPCHK(h, B[RL_WROWS1].ensure((size_t)waves * 4)); HIPCHK(h, B[RL_WENTS1].ensure((size_t)waves * 4));
    const char* rb = h->q.results.as<char>();
    const auto& ro = h->q.ro;
    S.n = J; S.nret = 0; S.ret = nullptr; S.found = nullptr;
    S.job_id = B[RL_JID].as<u32>();
    S.admit = in->admit ? B[RL_ADMIT].as<uint8_t>() : nullptr;
    S.jresv = in->reservation ? B[RL_JRESV].as<u32>() : nullptr;
    S.reason = (const uint8_t*)(rb + ro.reason); S.start = (const i64*)(rb + ro.start);
    S.limit = h->q.raw[JR_LIMIT].as<i64>(); S.place_off = h->q.raw[JR_PLACE_OFF].as<u64>(); S.places = places;
    S.pnode = (const u32*)(rb + ro.node); S.pcpu = (const i64*)(rb + ro.cpu); S.pmem = (const u64*)(rb + ro.mem);
    S.pclo = (const u64*)(rb + ro.clo); S.pchi = (const u64*)(rb + ro.chi); S.pgres = (const u64*)(rb + ro.gres);
    S.pc2 = h->lay.wide_cores ? (const u64*)(rb + ro.c2) : nullptr; S.pc3 = h->lay.wide_cores ? (const u64*)(rb + ro.c3) : nullptr;
    S.now = in->now_sec;
    S.wave_rows = B[RL_WROWS1].as<u32>(); S.wave_ents = B[RL_WENTS1].as<u32>();
    S.base = tot;
    hipLaunchKernelGGL(k_run_keep<true>, dim3(grid), dim3(kRunBlock), 0, h->stream, S);
    scan_counts(h->stream, S.wave_rows, waves, tot + 2);
    scan_counts(h->stream, S.wave_ents, waves, tot + 3);
    hipLaunchKernelGGL(k_run_compact<true>, dim3(grid), dim3(kRunBlock), 0, h->stream, S);
    if (with_attrs) hipLaunchKernelGGL(k_ra_origin<true>, dim3(grid), dim3(kRunBlock), 0, h->stream, S, C[RA_ORIGIN].as<u32>());
    HIPCHK(h, hipGetLastError());
  }
  hipLaunchKernelGGL(k_run_seal, dim3(1), dim3(64), 0, h->stream, S.D.off, (const u32*)tot, cap_rows);
  if (with_attrs && cap_rows) {
    RaGather G;
    memset(&G, 0, sizeof G);
    G.cap_rows = cap_rows; G.old_rows = R; G.queue_jobs = J; G.now = in->now_sec;
    G.tot = tot; G.origin = C[RA_ORIGIN].as<u32>(); G.L = ra_cols(h, RA_START); G.D = ra_cols(h, RA_WSTART);
    G.q_qos = C[RA_QQOS].as<u32>(); G.q_qprio = C[RA_QQPRIO].as<u32>(); G.q_part = C[RA_QPART].as<u32>(); G.q_account = C[RA_QACCT].as<u32>();
    hipLaunchKernelGGL(k_ra_gather, dim3((cap_rows + kRunBlock - 1) / kRunBlock), dim3(kRunBlock), 0, h->stream, G);
  }
  HIPCHK(h, hipGetLastError());
  u32 ht[4] = {0, 0, 0, 0};
  std::vector<uint8_t> found(K);
  HIPCHK(h, hipMemcpyAsync(ht, tot, sizeof ht, hipMemcpyDeviceToHost, h->stream));
  if (K) HIPCHK(h, hipMemcpyAsync(found.data(), B[RL_FOUND].p, K, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the new ledger's sizes size the rebuild
  const u64 R2 = (u64)ht[0] + ht[2], A2 = (u64)ht[1] + ht[3];
  if (ht[0] > R || ht[1] > A || R2 > cap_rows || A2 > cap_ents) return fail(h, CNS_ERR_HIP, "cns_running_advance: the compaction counted more rows than its sources have");
  u32 M = 0;
  bool over = false;
  if (int rc = run_rebuild(h, RL_WID, (u32)R2, (u32)A2, &M, &over)) return rc;
  if (over) return fail(h, CNS_ERR_UNSUPPORTED, kRunOverCap);
  if (int rc = run_commit(h, (u32)R2, (u32)A2, M)) return rc;
  if (with_attrs) ra_commit(h);
  for (u32 i = 0; i < K; ++i) out->found[order[i]] = found[i];
  if (out && out->num_retired) *out->num_retired = R - ht[0];
  if (out && out->num_admitted) *out->num_admitted = ht[2];
  return CNS_OK;
}

int cns_running_advance(cns_handle* h, const cns_running_step* in, const cns_running_step_out* out) {
  if (!h || !in) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_advance: null argument");
  run_drop_if_stale(h);
  cns_running::Facts F;
  F.have_ledger = h->rl_have && h->have_nodes;
  F.have_cycle = h->have_run; F.preempt_cycle = h->run_preempt && !h->run_preempt_rl;   // (served behind cns_running_select_preempt: the caller's mask decides)
  F.cycle_jobs = h->q.J; F.cycle_now = h->last_now; F.cycle_places = h->q.places;
  F.ledger_jobs = h->rl_R; F.ledger_allocs = h->rl_A;
  std::vector<u32> sorted_ids, order;
  if (const auto v = cns_running::check_step(F, in, out, &sorted_ids, &order)) return fail(h, v.code, v.msg);
  if (const auto v = cns_running::check_step_after_preempt(h->have_run && h->run_preempt_rl, in)) return fail(h, v.code, v.msg);
  const int rc = advance_impl(h, in, out, sorted_ids, order);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_running_get(cns_handle* h, const cns_running_ledger* o) {
  if (!h || !o) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_get: null argument");
  run_drop_if_stale(h);
  if (!h->rl_have) return fail(h, CNS_ERR_STATE, "cns_running_get before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)");
  const u32 R = h->rl_R, A = h->rl_A;
  if (o->num_jobs) *o->num_jobs = R;
  if (o->num_allocs) *o->num_allocs = A;
  const bool rows = o->job_id || o->end_sec || o->reservation || o->alloc_offsets;
  const bool ents = o->alloc_node || o->alloc_cpu_raw || o->alloc_mem || o->alloc_core_lo || o->alloc_core_hi || o->alloc_core_w2 || o->alloc_core_w3 || o->alloc_gres;
  if ((rows && o->capacity_jobs < R) || (ents && o->capacity_allocs < A)) return fail(h, CNS_ERR_INVALID_ARG, "cns_running_get: the arrays are smaller than the ledger");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_rl;
  std::vector<Res> res(ents ? A : 0);
  if (o->job_id && R) HIPCHK(h, hipMemcpyAsync(o->job_id, B[RL_ID].p, (size_t)R * 4, hipMemcpyDeviceToHost, h->stream));
  if (o->end_sec && R) HIPCHK(h, hipMemcpyAsync(o->end_sec, B[RL_END].p, (size_t)R * 8, hipMemcpyDeviceToHost, h->stream));
  if (o->reservation && R) HIPCHK(h, hipMemcpyAsync(o->reservation, B[RL_RESV].p, (size_t)R * 4, hipMemcpyDeviceToHost, h->stream));
  if (o->alloc_offsets) HIPCHK(h, hipMemcpyAsync(o->alloc_offsets, B[RL_OFF].p, ((size_t)R + 1) * 4, hipMemcpyDeviceToHost, h->stream));
  if (o->alloc_node && A) HIPCHK(h, hipMemcpyAsync(o->alloc_node, B[RL_NODE].p, (size_t)A * 4, hipMemcpyDeviceToHost, h->stream));
  if (ents && A) HIPCHK(h, hipMemcpyAsync(res.data(), B[RL_RES].p, (size_t)A * sizeof(Res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (u32 a = 0; a < (ents ? A : 0); ++a) {
    const Res& r = res[a];
    if (o->alloc_cpu_raw) o->alloc_cpu_raw[a] = r.cpu;
    if (o->alloc_mem) o->alloc_mem[a] = r.mem;
    if (o->alloc_core_lo) o->alloc_core_lo[a] = r.clo;
    if (o->alloc_core_hi) o->alloc_core_hi[a] = r.chi;
    if (o->alloc_core_w2) o->alloc_core_w2[a] = r.c2;
    if (o->alloc_core_w3) o->alloc_core_w3[a] = r.c3;
    if (o->alloc_gres) o->alloc_gres[a] = r.gres;
  }
  return CNS_OK;
}

int cns_running_get_timing(const cns_handle* h, cns_running_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->rl_timing;
  return CNS_OK;
}

int cns_running_shape(uint32_t* job_chunk, uint32_t* lane_max_allocs, uint32_t* sort_tile, uint32_t* scan_span) {
  if (job_chunk) *job_chunk = kRunChunk;
  if (lane_max_allocs) *lane_max_allocs = kRunLaneMax;
  if (sort_tile) *sort_tile = kSortTile;
  if (scan_span) *scan_span = kRunScanSpan;
  return CNS_OK;
}
