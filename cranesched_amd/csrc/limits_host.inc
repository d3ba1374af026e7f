// Host side of the run-limit admission (include/crane_gpu/run_limits.h).  Included by engine.hip inside extern "C".
// Done on the host: validation and pure re-layout — cns_usage / cns_tres records into the 16-component check order
// of limits_kernels.hip, the account tree levels, the per-QoS "which partition checks apply" flags
// (CheckPartitionRunLimitsForEntity_, AccountMetaContainer.cpp:577,589,598).  Every comparison, every usage update
// and the allocation views are computed on the GPU; there is no CPU fallback.

namespace {

struct LimCompMap { u32 name_comp[CNS_MAX_GRES_NAMES]; u32 class_comp[CNS_MAX_GRES_CLASSES]; u32 class_name[CNS_MAX_GRES_CLASSES]; u32 ncls; };

LimCompMap lim_comp_map(const cns_engine* h) {
  LimCompMap m{};
  m.ncls = h->gres.num_classes;
  for (u32 g = 0; g < m.ncls; ++g) m.class_name[g] = (h->gres.class_name_packed >> (4 * g)) & 0xF;
  u32 comp = 4;
  for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n) {  // CheckGres_ order: ascending name, its total, then its classes
    m.name_comp[n] = comp++;
    for (u32 g = 0; g < m.ncls; ++g)
      if (m.class_name[g] == n) m.class_comp[g] = comp++;
  }
  return m;
}

void lim_pack_tres(const LimCompMap& m, const cns_tres& t, LimRec& r) {
  r.lim[0] = t.cpu_raw;
  r.lim[3] = (i64)t.mem;
  for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n)
    if (t.name_mask >> n & 1) { r.has |= 1u << m.name_comp[n]; r.lim[m.name_comp[n]] = (i64)t.name_total[n]; }
  for (u32 g = 0; g < m.ncls; ++g)
    if ((t.class_mask >> g & 1) && (t.name_mask >> m.class_name[g] & 1)) {
      r.has |= 1u << m.class_comp[g];
      r.lim[m.class_comp[g]] = (i64)t.class_count[g];
    }
}

bool lim_tres_unlimited(const cns_tres& t) {  // IsUnlimitedTres_, AccountMetaContainer.cpp:362-365
  return t.cpu_raw == CNS_LIM_UNLIMITED_CPU_RAW && t.mem == CNS_LIM_MAX_JOB_MEMORY && t.name_mask == 0;
}

void lim_pack_usage(const LimCompMap& m, const cns_usage* u, i64* out) {
  for (u32 c = 0; c < 16; ++c) out[c] = 0;
  if (!u) return;
  out[0] = u->cpu_raw; out[1] = u->jobs_count; out[2] = u->wall_sec; out[3] = (i64)u->mem;
  for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n) out[m.name_comp[n]] = (i64)u->name_total[n];
  for (u32 g = 0; g < m.ncls; ++g) out[m.class_comp[g]] = (i64)u->class_count[g];
}

void lim_unpack_usage(const LimCompMap& m, const i64* in, cns_usage* u) {
  memset(u, 0, sizeof *u);
  u->cpu_raw = in[0]; u->jobs_count = (u32)in[1]; u->wall_sec = in[2]; u->mem = (u64)in[3];
  for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n) u->name_total[n] = (u64)in[m.name_comp[n]];
  for (u32 g = 0; g < m.ncls; ++g) u->class_count[g] = (u64)in[m.class_comp[g]];
}

}  // namespace

int cns_set_run_limits(cns_handle* h, const cns_limit_tables* t) {
  if (!h || !t) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_run_limits: null argument");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_set_run_limits before cns_set_nodes (the GRES layout comes with the nodes)");
  h->lim_have_tables = h->lim_have_jobs = h->lim_have_run = false;
  cns_acct::Space S;
  std::vector<u32> level;   // account tree levels (root = 0); the chain of a job is its account and the ancestors
  if (const auto v = cns_limits_host::check_tables(t, &S, &level)) return fail(h, v.code, v.msg);
  HIPCHK(h, hipSetDevice(h->device));
  const LimCompMap m = lim_comp_map(h);
  const u64 Q = S.Q;
  // limit records: [Qos per-user | Qos per-account | Qos global | partition limits]
  std::vector<LimRec> lim(3 * Q + t->num_part_limits);
  std::vector<u32> qflags(Q, 0);
  for (auto& r : lim) { for (i64& x : r.lim) x = kInf; r.cpu_x = kInf; r.has = 0; r.pad = 0; }
  auto zero_gres = [](LimRec& r) { for (u32 c = 4; c < 16; ++c) r.lim[c] = 0; };
  for (u64 q = 0; q < Q; ++q) {
    const cns_qos_limits& s = t->qos[q];
    const i64 wall = s.max_wall_sec > 0 ? s.max_wall_sec : kInf;
    LimRec& ru = lim[q]; LimRec& ra = lim[Q + q]; LimRec& rg = lim[2 * Q + q];
    zero_gres(ru); zero_gres(ra); zero_gres(rg);
    ru.lim[1] = s.max_jobs_per_user; ru.lim[2] = wall; ru.cpu_x = s.max_cpus_per_user_raw; lim_pack_tres(m, s.max_tres_per_user, ru);
    ra.lim[1] = s.max_jobs_per_account; ra.lim[2] = wall; lim_pack_tres(m, s.max_tres_per_account, ra);
    rg.lim[1] = s.max_jobs; rg.lim[2] = wall; lim_pack_tres(m, s.max_tres, rg);
    qflags[q] = (s.max_jobs_per_user == CNS_LIM_UNLIMITED_JOBS ? kLqUserJobsUnl : 0) |
                (s.max_jobs_per_account == CNS_LIM_UNLIMITED_JOBS ? kLqAcctJobsUnl : 0) |
                (s.max_wall_sec == 0 ? kLqWallZero : 0) | (lim_tres_unlimited(s.max_tres_per_user) ? kLqUserTresUnl : 0) |
                (lim_tres_unlimited(s.max_tres_per_account) ? kLqAcctTresUnl : 0);
  }
  for (u32 i = 0; i < t->num_part_limits; ++i) {
    const cns_part_limit& s = t->part_limits[i];
    LimRec& r = lim[3 * Q + i];
    zero_gres(r);
    r.lim[1] = s.max_jobs; r.lim[2] = s.max_wall_sec > 0 ? s.max_wall_sec : kInf;
    lim_pack_tres(m, s.max_tres, r);
  }
  // usage records, one array: [user_qos | user_part | acct_qos | acct_part | qos]; entries that do not exist are zero
  std::vector<i64> usage(std::max<u64>(S.NR, 1) * 16, 0);
  std::vector<uint8_t> exists(std::max<u64>(S.NR, 1), 1);
  const cns_usage* use[5] = {t->user_qos, t->user_part, t->acct_qos, t->acct_part, t->qos_usage};
  const uint8_t* nex[5] = {t->user_qos_exists, t->user_part_exists, t->acct_qos_exists, t->acct_part_exists, nullptr};
  for (int w = 0; w < 5; ++w)
    for (u64 i = 0, r = S.base[w]; i < S.len[w]; ++i, ++r) {
      exists[r] = !nex[w] || nex[w][i];
      lim_pack_usage(m, (use[w] && exists[r]) ? use[w] + i : nullptr, usage.data() + r * 16);
    }
  std::vector<u32> parent(t->acct_parent, t->acct_parent + S.A);
  if (parent.empty()) { parent.push_back(kNone); level.push_back(0); }
  DevBuf* b = h->d_lim;  // (buf_slots.h)
  if (int rc = upload(h, b[LM_LIM], lim)) return rc;
  if (int rc = upload(h, b[LM_QFLAGS], qflags)) return rc;
  if (int rc = upload(h, b[LM_PARENT], parent)) return rc;
  if (int rc = upload(h, b[LM_LEVEL], level)) return rc;
  h->lim_has_upl = t->user_part_limit != nullptr && S.len[1] > 0;
  h->lim_has_apl = t->acct_part_limit != nullptr && S.len[3] > 0;
  std::vector<u32> upl, apl;  // kept alive until the stream is drained below
  if (h->lim_has_upl) { upl.assign(t->user_part_limit, t->user_part_limit + S.len[1]); if (int rc = upload(h, b[LM_UPL], upl)) return rc; }
  if (h->lim_has_apl) { apl.assign(t->acct_part_limit, t->acct_part_limit + S.len[3]); if (int rc = upload(h, b[LM_APL], apl)) return rc; }
  if (int rc = upload(h, b[LM_USAGE0], usage)) return rc;
  if (int rc = upload(h, b[LM_EXISTS0], exists)) return rc;
  HIPCHK(h, b[LM_USAGE].ensure(usage.size() * 8));
  HIPCHK(h, b[LM_EXISTS].ensure(exists.size()));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->lim_sp = S;
  h->lim_level = level;
  h->lim_have_tables = true;
  return CNS_OK;
}

int cns_upload_limit_jobs(cns_handle* h, const cns_limit_job_soa* jb) {
  if (!h || !jb) return fail(h, CNS_ERR_INVALID_ARG, "cns_upload_limit_jobs: null argument");
  if (!h->lim_have_tables) return fail(h, CNS_ERR_STATE, "cns_upload_limit_jobs before cns_set_run_limits");
  if (!h->have_jobs) return fail(h, CNS_ERR_STATE, "cns_upload_limit_jobs before cns_upload_jobs / cns_select");
  h->lim_have_jobs = h->lim_have_run = false;
  const u64 J = jb->num_jobs;
  if (const auto v = cns_limits_host::check_jobs(h->lim_sp, jb, h->q.J)) return fail(h, v.code, v.msg);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  DevBuf* b = h->d_lim;
  // job keys of skipped jobs may be anything: they are never dereferenced on the device
  if (jb->select_index) { if (int rc = stage(h, b[LM_SEL], jb->select_index, J * 8)) return rc; }
  if (int rc = stage(h, b[LM_USER], jb->user, J * 4)) return rc;
  if (int rc = stage(h, b[LM_UA], jb->user_acct, J * 4)) return rc;
  if (int rc = stage(h, b[LM_ACCT], jb->account, J * 4)) return rc;
  if (int rc = stage(h, b[LM_QOS], jb->qos, J * 4)) return rc;
  if (int rc = stage(h, b[LM_PART], jb->partition, J * 4)) return rc;
  if (int rc = stage(h, b[LM_TL], jb->time_limit_sec, J * 8)) return rc;
  if (jb->skip) { if (int rc = stage(h, b[LM_SKIP], jb->skip, J)) return rc; }
  if (int rc = stage(h, b[LM_PLACEOFF], h->q.h_place.p, h->q.h_place.p ? (size_t)(h->q.J + 1) * 8 : 0)) return rc;
  h->lim_has_sel = jb->select_index != nullptr;
  h->lim_has_skip = jb->skip != nullptr;
  const u64 nb = (J + 255) / 256, Jc = std::max<u64>(J, 1);
  HIPCHK(h, b[LM_BLKCNT].ensure(std::max<u64>(nb, 1) * 4));
  HIPCHK(h, b[LM_BLKOFF].ensure(std::max<u64>(nb, 1) * 8));
  HIPCHK(h, b[LM_CTR].ensure(32));   // total, admitted, n_items, undecided
  HIPCHK(h, b[LM_RECADD].ensure(Jc * 16 * 8));
  HIPCHK(h, b[LM_RECC].ensure(Jc * 16 * 4));
  HIPCHK(h, b[LM_RECL].ensure(Jc * 16 * 4));
  HIPCHK(h, b[LM_RECEN].ensure(Jc * 16 * 4));
  HIPCHK(h, b[LM_RECJOB].ensure(Jc * 4));
  HIPCHK(h, b[LM_RECMETA].ensure(Jc * 4));
  HIPCHK(h, b[LM_OUT].ensure(Jc));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->lim_timing = cns_limit_timing{};
  h->lim_timing.h2d_ms = ms;
  h->lim_J = J;
  h->lim_sel_J = h->q.J;
  h->lim_have_jobs = true;
  return CNS_OK;
}

int cns_run_limits_resident(cns_handle* h) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_run_limits_resident: null handle");
  if (!h->lim_have_jobs) return fail(h, CNS_ERR_STATE, "cns_run_limits_resident before cns_upload_limit_jobs");
  if (!h->have_run || h->lim_sel_J != h->q.J) return fail(h, CNS_ERR_STATE, "cns_run_limits_resident without the matching cns_select results");
  HIPCHK(h, hipSetDevice(h->device));
  h->lim_have_run = false;
  DevBuf* b = h->d_lim;
  LimParams P;
  memset(&P, 0, sizeof P);
  const cns_acct::Space& S = h->lim_sp;
  P.J = h->lim_J; P.Q = (u32)S.Q; P.Pn = (u32)S.Pn;
  P.base_uq = (u32)S.base[0]; P.base_up = (u32)S.base[1]; P.base_aq = (u32)S.base[2]; P.base_ap = (u32)S.base[3]; P.base_g = (u32)S.base[4];
  P.sel = h->lim_has_sel ? b[LM_SEL].as<u64>() : nullptr;
  P.user = b[LM_USER].as<u32>(); P.ua = b[LM_UA].as<u32>(); P.account = b[LM_ACCT].as<u32>(); P.qos = b[LM_QOS].as<u32>(); P.part = b[LM_PART].as<u32>();
  P.tl = b[LM_TL].as<i64>(); P.skip = h->lim_has_skip ? b[LM_SKIP].as<uint8_t>() : nullptr;
  P.acct_parent = b[LM_PARENT].as<u32>(); P.acct_level = b[LM_LEVEL].as<u32>(); P.qos_flags = b[LM_QFLAGS].as<u32>();
  P.user_part_limit = h->lim_has_upl ? b[LM_UPL].as<u32>() : nullptr;
  P.acct_part_limit = h->lim_has_apl ? b[LM_APL].as<u32>() : nullptr;
  P.lim = b[LM_LIM].as<LimRec>();
  P.usage = b[LM_USAGE].as<i64>(); P.exists = b[LM_EXISTS].as<uint8_t>();
  const char* rb = h->q.results.as<char>();
  P.o_reason = (const uint8_t*)(rb + h->q.ro.reason); P.place_off = b[LM_PLACEOFF].as<u64>(); P.o_node = (const u32*)(rb + h->q.ro.node);
  P.o_cpu = (const i64*)(rb + h->q.ro.cpu); P.o_mem = (const u64*)(rb + h->q.ro.mem); P.o_gres = (const u64*)(rb + h->q.ro.gres);
  P.blk_cnt = b[LM_BLKCNT].as<u32>(); P.blk_off = b[LM_BLKOFF].as<u64>(); P.total = b[LM_CTR].as<u64>(); P.admitted = b[LM_CTR].as<u64>() + 1;
  P.rec_add = b[LM_RECADD].as<i64>(); P.rec_c = b[LM_RECC].as<u32>(); P.rec_l = b[LM_RECL].as<u32>(); P.rec_en = b[LM_RECEN].as<u32>();
  P.rec_job = b[LM_RECJOB].as<u32>(); P.rec_meta = b[LM_RECMETA].as<u32>(); P.out = b[LM_OUT].as<uint8_t>();
  const LimCompMap m = lim_comp_map(h);
  for (u32 g = 0; g < 8; ++g) {
    P.lay.class_mask[g] = g < m.ncls ? h->gres.class_mask[g] : 0;
    P.lay.class_comp[g] = (uint8_t)(g < m.ncls ? m.class_comp[g] : 15);
    P.lay.class_name_comp[g] = (uint8_t)(g < m.ncls ? m.name_comp[m.class_name[g]] : 15);
  }
  P.lay.num_classes = m.ncls;
  const u32 nb = (u32)((h->lim_J + 255) / 256);
  const char* mode_env = getenv("CNS_LIMITS_MODE");   // "seq": force the ordered single-wave kernel (tests cover both)
  const bool force_seq = mode_env && std::string(mode_env) == "seq";
  P.NR = (u32)S.NR;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  HIPCHK(h, hipMemcpyAsync(b[LM_USAGE].p, b[LM_USAGE0].p, std::max<u64>(S.NR, 1) * 128, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(b[LM_EXISTS].p, b[LM_EXISTS0].p, std::max<u64>(S.NR, 1), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(b[LM_CTR].p, 0, 32, h->stream));   // total, admitted, n_items, undecided
  u64 res[2] = {0, 0};
  u32 rounds = 0;
  bool used_seq = false;
  if (nb) {
    hipLaunchKernelGGL(k_lim_flags, dim3(nb), dim3(256), 0, h->stream, P);
    hipLaunchKernelGGL(k_lim_scan, dim3(1), dim3(kLimScanThreads), 0, h->stream, P, nb);
    HIPCHK(h, hipMemcpyAsync(res, b[LM_CTR].p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // M sizes the item stream of the parallel pass
  }
  const u64 M = res[0];
  const u64 n = M * 16;
  DevBuf* pb = h->d_limpar;
  const bool par = M > 0 && !force_seq && n < cns_acct::kMaxRecords;
  if (par) {
    HIPCHK(h, pb[LP_K0].ensure(n * 8));
    P.item_key = pb[LP_K0].as<u64>();
  }
  if (M) hipLaunchKernelGGL(k_lim_build, dim3(nb), dim3(256), 0, h->stream, P);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  if (par) {
    const u32 n32 = (u32)n;
    HIPCHK(h, pb[LP_K1].ensure(n * 8)); HIPCHK(h, pb[LP_V0].ensure(n * 4)); HIPCHK(h, pb[LP_V1].ensure(n * 4));
    HIPCHK(h, pb[LP_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(n32, kSortTile))));
    for (int x : {LP_SKEY, LP_SK, LP_SL, LP_SEN, LP_SSLOT}) HIPCHK(h, pb[x].ensure(n * 4));
    HIPCHK(h, pb[LP_SADD].ensure(n * 128));
    HIPCHK(h, pb[LP_STATE].ensure(M)); HIPCHK(h, pb[LP_FLAGS].ensure(M * 4)); HIPCHK(h, pb[LP_JOBKEY].ensure(M * 4));
    HIPCHK(h, pb[LP_TAILS].ensure((size_t)kParChunks * 256)); HIPCHK(h, pb[LP_HEADS].ensure(kParChunks)); HIPCHK(h, pb[LP_CARRY].ensure((size_t)kParChunks * 256));
    // (candidate, slot) items sorted by usage record, stable: inside a record the candidates stay in commit-loop order
    u64* kin = pb[LP_K0].as<u64>(); u64* kout = pb[LP_K1].as<u64>();
    u32* vin = pb[LP_V0].as<u32>(); u32* vout = pb[LP_V1].as<u32>();
    sort_index_pairs(h->stream, n32, cns_sort::key_passes(h->lim_sp.NR), kin, vin, kout, vout, pb[LP_HIST].as<u32>());
    ParParams R;
    memset(&R, 0, sizeof R);
    u64* ctr = b[LM_CTR].as<u64>();
    R.n_items = ctr + 2; R.total = ctr; R.undecided = ctr + 3; R.admitted = ctr + 1;
    R.s_key = pb[LP_SKEY].as<u32>(); R.s_k = pb[LP_SK].as<u32>(); R.s_l = pb[LP_SL].as<u32>(); R.s_en = pb[LP_SEN].as<u32>(); R.s_slot = pb[LP_SSLOT].as<u32>();
    R.s_add = pb[LP_SADD].as<i64>(); R.state = pb[LP_STATE].as<uint8_t>(); R.flags = pb[LP_FLAGS].as<u32>(); R.jobkey = pb[LP_JOBKEY].as<u32>();
    R.tails = pb[LP_TAILS].as<i64>(); R.heads = pb[LP_HEADS].as<uint8_t>(); R.carry = pb[LP_CARRY].as<i64>();
    R.lim = P.lim; R.usage0 = b[LM_USAGE0].as<i64>(); R.exists0 = b[LM_EXISTS0].as<uint8_t>(); R.usage = P.usage; R.exists = P.exists;
    R.rec_meta = P.rec_meta; R.rec_job = P.rec_job; R.out = P.out;
    hipLaunchKernelGGL(k_par_gather, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, h->stream, (const u64*)kin, (const u32*)vin, n,
                       P.NR, P, pb[LP_SKEY].as<u32>(), pb[LP_SK].as<u32>(), pb[LP_SL].as<u32>(), pb[LP_SEN].as<u32>(), pb[LP_SSLOT].as<u32>(), pb[LP_SADD].as<i64>(), ctr + 2);
    HIPCHK(h, hipMemsetAsync(pb[LP_STATE].p, 0, M, h->stream));
    HIPCHK(h, hipMemsetAsync(pb[LP_FLAGS].p, 0, M * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(pb[LP_JOBKEY].p, 0xFF, M * 4, h->stream));
    const dim3 cg(kParChunks * 16 / 256), jg((unsigned)((M + 255) / 256));
    u64 und = M;
    while (und && rounds < kLimMaxRounds) {
      ++rounds;
      HIPCHK(h, hipMemsetAsync(ctr + 3, 0, 8, h->stream));
      hipLaunchKernelGGL(k_par_tails, cg, dim3(256), 0, h->stream, R);
      hipLaunchKernelGGL(k_par_carry, dim3(1), dim3(kParRowGroups * 16), 0, h->stream, R);
      hipLaunchKernelGGL(k_par_eval<false>, cg, dim3(256), 0, h->stream, R);
      hipLaunchKernelGGL(k_par_update, jg, dim3(256), 0, h->stream, R);
      HIPCHK(h, hipMemcpyAsync(&und, ctr + 3, 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (und == 0) {  // every job decided: exact sums -> reasons and the usage tables after the pass
      hipLaunchKernelGGL(k_par_tails, cg, dim3(256), 0, h->stream, R);
      hipLaunchKernelGGL(k_par_carry, dim3(1), dim3(kParRowGroups * 16), 0, h->stream, R);
      hipLaunchKernelGGL(k_par_eval<true>, cg, dim3(256), 0, h->stream, R);
      hipLaunchKernelGGL(k_par_finish, jg, dim3(256), 0, h->stream, R);
    } else {
      used_seq = true;   // pathological chains: the ordered kernel decides everything from the pristine usage copy
    }
  }
  if (M && (!par || used_seq)) {
    used_seq = true;
    hipLaunchKernelGGL(k_lim_admit, dim3(1), dim3(64), 0, h->stream, P);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  HIPCHK(h, hipMemcpyAsync(res, b[LM_CTR].p, 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float a = 0, c = 0;
  HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIPCHK(h, hipEventElapsedTime(&c, h->ev[1], h->ev[2]));
  h->lim_timing.prep_ms = a;
  h->lim_timing.admit_ms = c;
  h->lim_timing.candidates = res[0];
  h->lim_timing.admitted = res[1];
  h->lim_timing.rounds = rounds;
  h->lim_timing.ordered_fallback = used_seq ? 1 : 0;
  h->lim_have_run = true;
  return CNS_OK;
}

int cns_download_limits(cns_handle* h, uint8_t* out, uint64_t* num_admitted) {
  if (!h || (!out && h->lim_J)) return fail(h, CNS_ERR_INVALID_ARG, "cns_download_limits: null argument");
  if (!h->lim_have_run) return fail(h, CNS_ERR_STATE, "cns_download_limits before a successful run");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (h->lim_J) HIPCHK(h, hipMemcpyAsync(out, h->d_lim[LM_OUT].p, h->lim_J, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->lim_timing.d2h_ms = ms;
  if (num_admitted) *num_admitted = h->lim_timing.admitted;
  return CNS_OK;
}

int cns_apply_run_limits(cns_handle* h, const cns_limit_job_soa* jobs, uint8_t* out, uint64_t* num_admitted) {
  if (int rc = cns_upload_limit_jobs(h, jobs)) return rc;
  if (int rc = cns_run_limits_resident(h)) return rc;
  return cns_download_limits(h, out, num_admitted);
}

int cns_get_limit_timing(const cns_handle* h, cns_limit_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->lim_timing;
  return CNS_OK;
}

int cns_limits_shape(uint32_t* min_item_chunk, uint32_t* num_chunks, uint32_t* batch, uint32_t* carry_row_chunks, uint32_t* max_rounds,
                     uint32_t* scan_jobs) {
  if (min_item_chunk) *min_item_chunk = kParMinChunk;
  if (num_chunks) *num_chunks = kParChunks;
  if (batch) *batch = kParBatch;
  if (carry_row_chunks) *carry_row_chunks = kParRowChunks;
  if (max_rounds) *max_rounds = kLimMaxRounds;
  if (scan_jobs) *scan_jobs = kLimScanJobs;
  return CNS_OK;
}

int cns_get_usage(cns_handle* h, cns_usage* uq, uint8_t* uqe, cns_usage* up, uint8_t* upe, cns_usage* aq, uint8_t* aqe,
                  cns_usage* ap, uint8_t* ape, cns_usage* qu) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_get_usage: null handle");
  if (!h->lim_have_run) return fail(h, CNS_ERR_STATE, "cns_get_usage before a successful admission run");
  HIPCHK(h, hipSetDevice(h->device));
  const cns_acct::Space& S = h->lim_sp;
  const u64 NR = std::max<u64>(S.NR, 1);
  std::vector<i64> usage(NR * 16);
  std::vector<uint8_t> exists(NR);
  HIPCHK(h, hipMemcpy(usage.data(), h->d_lim[LM_USAGE].p, NR * 128, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(exists.data(), h->d_lim[LM_EXISTS].p, NR, hipMemcpyDeviceToHost));
  const LimCompMap m = lim_comp_map(h);
  cns_usage* outs[5] = {uq, up, aq, ap, qu};
  uint8_t* exs[5] = {uqe, upe, aqe, ape, nullptr};
  for (u32 tb = 0; tb < 5; ++tb)
    for (u64 i = 0; i < S.len[tb]; ++i) {
      const u64 r = S.base[tb] + i;
      if (outs[tb]) lim_unpack_usage(m, usage.data() + r * 16, outs[tb] + i);
      if (exs[tb]) exs[tb][i] = exists[r];
    }
  return CNS_OK;
}
