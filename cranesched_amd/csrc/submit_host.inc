// Host side of include/crane_gpu_submit/submit_limits.h.  Included by engine.hip inside extern "C".
// Host work: validation of the tables (once, cns_set_submit_limits) and of the call's key indices (the pass that uploads), the input rule
// on the 32-bit counts, the buffers, the launches.  Every check of a job against a limit or a counter runs on the device
// (submit_kernels.inc).  Everything lives in cns_engine::d_sub: no buffer of a cycle, of the validity check or of the run limits is read or
// written.  No CPU fallback.

int cns_set_submit_limits(cns_handle* h, const cns_submit_tables* t) {
  if (!h || !t) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_submit_limits: null argument");
  h->sub_have = false;
  cns_acct::Space S;
  if (const auto v = cns_submit_host::check_tables(t, &S)) return fail(h, v.code, v.msg);
  // the table: five count tables back to back, then one exists value per user, account, QoS
  std::vector<u32> st((size_t)(S.NR + S.NE), 0u);
  u32 mx = 0;
  const u32* cnt[5] = {t->user_qos_submit, t->user_part_submit, t->acct_qos_submit, t->acct_part_submit, t->qos_submit};
  for (int w = 0; w < 5; ++w)
    if (cnt[w])
      for (u64 i = 0; i < S.len[w]; ++i) { st[(size_t)(S.base[w] + i)] = cnt[w][i]; mx = std::max(mx, cnt[w][i]); }
  const uint8_t* ex[3] = {t->user_exists, t->acct_exists, t->qos_exists};
  for (int w = 0; w < 3; ++w)
    if (ex[w])
      for (u64 i = 0; i < S.ent_len[w]; ++i) st[(size_t)(S.ent[w] + i)] = ex[w][i] ? 1u : 0u;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_sub;
  int rc = 0;
  if ((rc = stage(h, B[SB_QOS], t->qos, (size_t)S.Q * sizeof(cns_submit_qos))) || (rc = stage(h, B[SB_PL], t->part_limits, (size_t)t->num_part_limits * sizeof(cns_submit_part_limit))) ||
      (rc = stage(h, B[SB_PARENT], t->acct_parent, (size_t)S.A * 4)) || (rc = stage(h, B[SB_UPL], t->user_part_limit, (size_t)S.len[1] * 4)) ||
      (rc = stage(h, B[SB_APL], t->acct_part_limit, (size_t)S.len[3] * 4)) || (rc = stage(h, B[SB_UQ], t->user_qos, (size_t)S.len[0] * sizeof(cns_usage))) ||
      (rc = stage(h, B[SB_AQ], t->acct_qos, (size_t)S.len[2] * sizeof(cns_usage))) || (rc = stage(h, B[SB_G], t->qos_usage, (size_t)S.len[4] * sizeof(cns_usage))) ||
      (rc = stage(h, B[SB_ST_SET], st.data(), st.size() * 4)) || (rc = stage(h, B[SB_ST], st.data(), st.size() * 4))) {
    drain(h);
    return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->sub_sp = S;
  h->sub_has_upl = t->user_part_limit != nullptr; h->sub_has_apl = t->acct_part_limit != nullptr;
  h->sub_has_uq = t->user_qos != nullptr; h->sub_has_aq = t->acct_qos != nullptr; h->sub_has_g = t->qos_usage != nullptr;
  h->sub_lay = t->gres;
  h->sub_max_set = h->sub_max_cur = mx;
  h->sub_timing = cns_submit_timing{};
  h->sub_have = true;
  return CNS_OK;
}

static int submit_impl(cns_handle* h, const cns_job_soa* jb, const cns_submit_keys* ky, u32 flags, const cns_submit_out* out) {
  const u32 J = (u32)jb->num_jobs;
  const cns_acct::Space& S = h->sub_sp;
  if (const auto v = cns_submit_host::check_jobs(S, jb, ky, out, flags, h->sub_max_set, h->sub_max_cur)) return fail(h, v.code, v.msg);
  const bool carry = (flags & CNS_SUBMIT_CARRY) != 0;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_sub;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  {
    const struct { int b; const void* p; size_t sz; } ups[] = {
        {SB_JPART, jb->partition, 4}, {SB_JTL, jb->time_limit_sec, 8}, {SB_JNCPU, jb->node_cpu_raw, 8}, {SB_JNMEM, jb->node_mem, 8},
        {SB_JTCPU, jb->task_cpu_raw, 8}, {SB_JTMEM, jb->task_mem, 8}, {SB_JK, jb->node_num, 4}, {SB_JNT, jb->ntasks, 4},
        {SB_JGT, jb->gres_total, CNS_MAX_GRES_NAMES}, {SB_JGS, jb->gres_spec, CNS_MAX_GRES_CLASSES}, {SB_KUSER, ky->user, 4}, {SB_KUA, ky->user_acct, 4},
        {SB_KACCT, ky->account, 4}, {SB_KQOS, ky->qos, 4}, {SB_KCOUNT, ky->count, 4}, {SB_KSKIP, ky->skip, 1}};
    for (const auto& u : ups)
      if (int rc = stage(h, B[u.b], u.p, (size_t)J * u.sz)) return rc;
  }
  const u32 NR = (u32)S.NR, NK = (u32)(S.NR + S.NE);
  const size_t n = (size_t)J * kSubItems;
  HIPCHK(h, B[SB_PRE].ensure(J)); HIPCHK(h, B[SB_STATE].ensure(J)); HIPCHK(h, B[SB_STAT].ensure((size_t)J * 8)); HIPCHK(h, B[SB_COND].ensure((size_t)J * 8));
  HIPCHK(h, B[SB_IKEY].ensure(n * 4)); HIPCHK(h, B[SB_ITHR].ensure(n * 4)); HIPCHK(h, B[SB_CODE].ensure(J)); HIPCHK(h, B[SB_TLO].ensure((size_t)J * 8));
  HIPCHK(h, B[SB_CTR].ensure(64));
  HIPCHK(h, hipMemsetAsync(B[SB_CTR].p, 0, 64, h->stream));
  if (!carry) HIPCHK(h, hipMemcpyAsync(B[SB_ST].p, B[SB_ST_SET].p, (size_t)NK * 4, hipMemcpyDeviceToDevice, h->stream));
  const char* mode_env = getenv("CNS_SUBMIT_MODE");   // "seq": force the ordered single-wave kernel (tests cover both)
  const bool par = !(mode_env && std::string(mode_env) == "seq");
  if (par) HIPCHK(h, B[SB_SK0].ensure(n * 8));

  SubParams P;
  memset(&P, 0, sizeof P);
  P.J = J; P.Q = (u32)S.Q; P.Pn = (u32)S.Pn; P.NK = NK;
  P.base_uq = (u32)S.base[0]; P.base_up = (u32)S.base[1]; P.base_aq = (u32)S.base[2]; P.base_ap = (u32)S.base[3]; P.base_g = (u32)S.base[4];
  P.ent_user = (u32)S.ent[0]; P.ent_acct = (u32)S.ent[1]; P.ent_qos = (u32)S.ent[2];
  P.part = B[SB_JPART].as<u32>(); P.tl = B[SB_JTL].as<i64>(); P.ncpu = jb->node_cpu_raw ? B[SB_JNCPU].as<i64>() : nullptr; P.nmem = B[SB_JNMEM].as<u64>();
  P.tcpu = B[SB_JTCPU].as<i64>(); P.tmem = B[SB_JTMEM].as<u64>(); P.k = B[SB_JK].as<u32>(); P.nt = B[SB_JNT].as<u32>();
  P.gt = jb->gres_total ? B[SB_JGT].as<u32>() : nullptr; P.gs = jb->gres_spec ? B[SB_JGS].as<u64>() : nullptr;
  P.user = B[SB_KUSER].as<u32>(); P.ua = B[SB_KUA].as<u32>(); P.account = B[SB_KACCT].as<u32>(); P.qos = B[SB_KQOS].as<u32>();
  P.count = B[SB_KCOUNT].as<u32>(); P.skip = ky->skip ? B[SB_KSKIP].as<uint8_t>() : nullptr;
  P.q = B[SB_QOS].as<cns_submit_qos>(); P.pl = B[SB_PL].as<cns_submit_part_limit>(); P.acct_parent = B[SB_PARENT].as<u32>();
  P.upl = h->sub_has_upl ? B[SB_UPL].as<u32>() : nullptr; P.apl = h->sub_has_apl ? B[SB_APL].as<u32>() : nullptr;
  P.uq_use = h->sub_has_uq ? B[SB_UQ].as<cns_usage>() : nullptr; P.aq_use = h->sub_has_aq ? B[SB_AQ].as<cns_usage>() : nullptr;
  P.g_use = h->sub_has_g ? B[SB_G].as<cns_usage>() : nullptr;
  P.lay = h->sub_lay;
  P.st = B[SB_ST].as<u32>();
  P.pre = B[SB_PRE].as<uint8_t>(); P.state = B[SB_STATE].as<uint8_t>(); P.stat = B[SB_STAT].as<u64>(); P.cond = B[SB_COND].as<u64>();
  P.item_key = B[SB_IKEY].as<u32>(); P.item_thr = B[SB_ITHR].as<u32>(); P.sort_key = par ? B[SB_SK0].as<u64>() : nullptr;
  P.code = B[SB_CODE].as<uint8_t>(); P.tlo = B[SB_TLO].as<i64>(); P.ctr = B[SB_CTR].as<u64>();

  const dim3 jg((J + kSubChunk - 1) / kSubChunk);
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  hipLaunchKernelGGL(k_sub_prep, jg, dim3(256), 0, h->stream, P);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));

  u32 rounds = 0;
  bool decided = false;
  if (par) {
    const u32 n32 = (u32)n;
    HIPCHK(h, B[SB_SK1].ensure(n * 8)); HIPCHK(h, B[SB_SV0].ensure(n * 4)); HIPCHK(h, B[SB_SV1].ensure(n * 4));
    HIPCHK(h, B[SB_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(n32, kSortTile))));
    HIPCHK(h, B[SB_SKEY].ensure(n * 4)); HIPCHK(h, B[SB_SITEM].ensure(n * 4)); HIPCHK(h, B[SB_SADD].ensure(n * 4)); HIPCHK(h, B[SB_VAL].ensure(n * 8));
    // (job, position) items sorted by table index, stable: inside a record the jobs stay in arrival order
    u64* kin = B[SB_SK0].as<u64>(); u64* kout = B[SB_SK1].as<u64>();
    u32* vin = B[SB_SV0].as<u32>(); u32* vout = B[SB_SV1].as<u32>();
    sort_index_pairs(h->stream, n32, cns_sort::key_passes(NK), kin, vin, kout, vout, B[SB_HIST].as<u32>());
    hipLaunchKernelGGL(k_sub_gather, dim3((n32 + 255) / 256), dim3(256), 0, h->stream, (const u64*)kin, (const u32*)vin, n32, NK, P.count, B[SB_SKEY].as<u32>(),
                       B[SB_SITEM].as<u32>(), B[SB_SADD].as<u32>(), P.ctr);
    HIPCHK(h, hipGetLastError());
    u64 ctr[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(ctr, P.ctr, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the number of items that carry a key sizes the rounds' grids
    SubPar R;
    memset(&R, 0, sizeof R);
    R.n = (u32)ctr[2]; R.nchunks = (R.n + kSubItemChunk - 1) / kSubItemChunk; R.J = J; R.NK = NK;
    R.s_key = B[SB_SKEY].as<u32>(); R.s_item = B[SB_SITEM].as<u32>(); R.s_add = B[SB_SADD].as<u32>(); R.state = P.state; R.st = P.st;
    HIPCHK(h, B[SB_TAILS].ensure((size_t)R.nchunks * 8)); HIPCHK(h, B[SB_HEADS].ensure(R.nchunks)); HIPCHK(h, B[SB_CARRY].ensure((size_t)R.nchunks * 8));
    R.tails = B[SB_TAILS].as<uint2>(); R.heads = B[SB_HEADS].as<uint8_t>(); R.carry = B[SB_CARRY].as<uint2>(); R.val = B[SB_VAL].as<uint2>();
    u64 und = R.n ? 1 : 0;   // without items nothing depends on the batch: the final pass decides from the static codes
    while (und && rounds < kSubMaxRounds) {
      ++rounds;
      HIPCHK(h, hipMemsetAsync(P.ctr + 3, 0, 8, h->stream));
      hipLaunchKernelGGL(k_sub_tails, dim3(R.nchunks), dim3(256), 0, h->stream, R);
      hipLaunchKernelGGL(k_sub_carry, dim3(1), dim3(1024), 0, h->stream, R);
      hipLaunchKernelGGL(k_sub_eval<false>, dim3(R.nchunks), dim3(256), 0, h->stream, R);
      hipLaunchKernelGGL(k_sub_decide, jg, dim3(256), 0, h->stream, P, (const uint2*)R.val);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(&und, P.ctr + 3, 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (und == 0) {   // every job decided: exact values -> codes, and the table after the batch
      if (R.n) {
        hipLaunchKernelGGL(k_sub_tails, dim3(R.nchunks), dim3(256), 0, h->stream, R);
        hipLaunchKernelGGL(k_sub_carry, dim3(1), dim3(1024), 0, h->stream, R);
        hipLaunchKernelGGL(k_sub_eval<true>, dim3(R.nchunks), dim3(256), 0, h->stream, R);
      }
      hipLaunchKernelGGL(k_sub_final, jg, dim3(256), 0, h->stream, P, (const uint2*)R.val);
      decided = true;
    }
  }
  if (!decided) hipLaunchKernelGGL(k_sub_admit, dim3(1), dim3(64), 0, h->stream, P);   // CNS_SUBMIT_MODE=seq, or a chain the rounds did not finish
  if (NR) hipLaunchKernelGGL(k_sub_max, dim3((NR + 255) / 256), dim3(256), 0, h->stream, (const u32*)P.st, NR, P.ctr);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float a = 0, b = 0, c = 0, d = 0;
  HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIPCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  HIPCHK(h, hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
  u64 ctr[5] = {0, 0, 0, 0, 0};
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  HIPCHK(h, hipMemcpyAsync(out->code, P.code, J, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out->time_limit_out, P.tlo, (size_t)J * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ctr, P.ctr, 40, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipEventElapsedTime(&d, h->ev[0], h->ev[1]));
  if (out->num_admitted) *out->num_admitted = ctr[1];
  h->sub_max_cur = (u32)ctr[4];
  h->sub_timing.h2d_ms = a; h->sub_timing.prep_ms = b; h->sub_timing.admit_ms = c; h->sub_timing.d2h_ms = d;
  h->sub_timing.candidates = ctr[0]; h->sub_timing.admitted = ctr[1];
  h->sub_timing.rounds = rounds; h->sub_timing.ordered_fallback = decided ? 0 : 1;
  return CNS_OK;
}

int cns_check_submissions(cns_handle* h, const cns_job_soa* jobs, const cns_submit_keys* keys, uint32_t flags, const cns_submit_out* out) {
  if (!h || !jobs || !keys) return fail(h, CNS_ERR_INVALID_ARG, "cns_check_submissions: null argument");
  if (!h->sub_have) return fail(h, CNS_ERR_STATE, "cns_check_submissions before cns_set_submit_limits");
  if (jobs->num_jobs == 0) return CNS_OK;   // nothing asked, nothing written
  if (jobs->num_jobs > CNS_SUBMIT_MAX_JOBS) return fail(h, CNS_ERR_UNSUPPORTED, "cns_check_submissions: more than 2^24 jobs in one call");
  if (!out) return fail(h, CNS_ERR_INVALID_ARG, "cns_check_submissions: null result");
  const int rc = submit_impl(h, jobs, keys, flags, out);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_get_submit_usage(cns_handle* h, uint32_t* user_qos_submit, uint32_t* user_part_submit, uint32_t* acct_qos_submit, uint32_t* acct_part_submit,
                         uint32_t* qos_submit, uint8_t* user_exists, uint8_t* acct_exists, uint8_t* qos_exists) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_get_submit_usage: null handle");
  if (!h->sub_have) return fail(h, CNS_ERR_STATE, "cns_get_submit_usage before cns_set_submit_limits");
  HIPCHK(h, hipSetDevice(h->device));
  const cns_acct::Space& S = h->sub_sp;
  std::vector<u32> st((size_t)(S.NR + S.NE));
  if (!st.empty()) HIPCHK(h, hipMemcpyAsync(st.data(), h->d_sub[SB_ST].p, st.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  uint32_t* cnt[5] = {user_qos_submit, user_part_submit, acct_qos_submit, acct_part_submit, qos_submit};
  for (int w = 0; w < 5; ++w)
    if (cnt[w] && S.len[w]) memcpy(cnt[w], st.data() + S.base[w], S.len[w] * 4);
  uint8_t* ex[3] = {user_exists, acct_exists, qos_exists};
  for (int w = 0; w < 3; ++w)
    if (ex[w])
      for (u64 i = 0; i < S.ent_len[w]; ++i) ex[w][i] = st[S.ent[w] + i] ? 1 : 0;
  return CNS_OK;
}

int cns_get_submit_timing(const cns_handle* h, cns_submit_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->sub_timing;
  return CNS_OK;
}

int cns_submit_shape(uint32_t* job_chunk, uint32_t* item_chunk, uint32_t* max_rounds) {
  if (job_chunk) *job_chunk = kSubChunk;
  if (item_chunk) *item_chunk = kSubItemChunk;
  if (max_rounds) *max_rounds = kSubMaxRounds;
  return CNS_OK;
}
