// Host side of include/crane_gpu_usage/usage.h.  Included by engine.hip inside extern "C".
// Host work: the input rules (usage_check_host.inc), packing the caller's tables into the device layout and back, the buffers, the
// launches.  Every record's arithmetic and every mask bit is computed on the device (usage_kernels.inc).  Everything lives in
// cns_engine::d_use: no buffer of a cycle, of the run limits or of the submit limits is read or written.  No CPU fallback.
//
// Three copies of the table: US_TAB_SET (as set), US_TAB_CUR (after the last call that succeeded), US_TAB_WORK (the call's output:
// a copy of its source that the kernels write into; swapped with CUR when the call succeeded, so a refused charge leaves CUR alone).

static size_t use_tab_bytes(const cns_engine* h) { return (size_t)h->use_sp.NR * kUseComp * 8 + (size_t)(h->use_sp.NR + h->use_sp.NE); }

int cns_usage_set_tables(cns_handle* h, const cns_usage_tables* t) {
  if (!h || !t) return fail(h, CNS_ERR_INVALID_ARG, "cns_usage_set_tables: null argument");
  h->use_have = h->use_have_cur = false;
  cns_acct::Space D;
  if (const auto v = cns_usage_host::check_tables(t, &D)) return fail(h, v.code, v.msg);
  // records [NR][17], then the exists bytes [NR] (1 for the qos records), then the entity bytes [NE]
  std::vector<u64> tab(((size_t)D.NR * kUseComp * 8 + (size_t)(D.NR + D.NE) + 7) / 8, 0ull);
  uint8_t* ex = reinterpret_cast<uint8_t*>(tab.data() + (size_t)D.NR * kUseComp);
  {
    const cns_usage* use[5] = {t->user_qos, t->user_part, t->acct_qos, t->acct_part, t->qos_usage};
    const u32* sub[5] = {t->user_qos_submit, t->user_part_submit, t->acct_qos_submit, t->acct_part_submit, t->qos_submit};
    const uint8_t* nex[5] = {t->user_qos_exists, t->user_part_exists, t->acct_qos_exists, t->acct_part_exists, nullptr};
    for (int w = 0; w < 5; ++w) {
      const u64 off = D.base[w];
      for (u64 i = 0; i < D.len[w]; ++i) {
        const bool exists = w == 4 || (nex[w] ? nex[w][i] != 0 : (use[w] || sub[w]));
        ex[off + i] = exists ? 1 : 0;
        if (!exists) continue;   // read as zero, whatever its value
        u64* r = tab.data() + (size_t)(off + i) * kUseComp;
        if (use[w]) {
          const cns_usage& s = use[w][i];
          r[0] = (u64)s.cpu_raw; r[1] = s.mem; r[2] = (u64)s.wall_sec; r[3] = s.jobs_count;
          for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n) r[5 + n] = s.name_total[n];
          for (u32 g = 0; g < CNS_MAX_GRES_CLASSES; ++g) r[9 + g] = s.class_count[g];
        }
        if (sub[w]) r[4] = sub[w][i];
      }
    }
    const uint8_t* ent[3] = {t->user_exists, t->acct_exists, t->qos_exists};
    for (int w = 0; w < 3; ++w)
      if (ent[w])
        for (u64 i = 0; i < D.ent_len[w]; ++i) ex[D.ent[w] + i] = ent[w][i] ? 1 : 0;
  }
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_use;
  const size_t bytes = (size_t)D.NR * kUseComp * 8 + (size_t)(D.NR + D.NE);
  int rc = 0;
  if ((rc = stage(h, B[US_PARENT], t->acct_parent, (size_t)D.A * 4)) || (rc = stage(h, B[US_TAB_SET], tab.data(), bytes)) ||
      (rc = stage(h, B[US_TAB_CUR], tab.data(), bytes)) || (rc = stage(h, B[US_TAB_WORK], nullptr, bytes))) {
    drain(h);
    return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->use_sp = D;
  h->use_timing = cns_usage_timing{};
  h->use_have = true;
  return CNS_OK;
}

static int usage_impl(cns_handle* h, u32 op, const cns_usage_jobs* jb, u32 flags, const cns_usage_out* out) {
  const cns_acct::Space& D = h->use_sp;
  const u32 J = (u32)jb->num_jobs;
  const bool carry = (flags & CNS_USAGE_CARRY) != 0;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_use;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  {
    const struct { int b; const void* p; size_t sz; } ups[] = {
        {US_JUSER, jb->user, 4}, {US_JUA, jb->user_acct, 4}, {US_JACCT, jb->account, 4}, {US_JQOS, jb->qos, 4}, {US_JPART, jb->partition, 4},
        {US_JCPU, jb->cpu_raw, 8}, {US_JMEM, jb->mem, 8}, {US_JWALL, jb->wall_sec, 8}, {US_JJOBS, jb->jobs_count, 4}, {US_JSUB, jb->submit_count, 4},
        {US_JNT, jb->name_total, 8 * CNS_MAX_GRES_NAMES}, {US_JCC, jb->class_count, 8 * CNS_MAX_GRES_CLASSES}, {US_JSKIP, jb->skip, 1}};
    for (const auto& u : ups)
      if (int rc = stage(h, B[u.b], u.p, (size_t)J * u.sz)) return rc;
  }
  const u32 NR = (u32)D.NR, NK = (u32)(D.NR + D.NE);
  const size_t n = (size_t)J * kUseSlots, tab_bytes = use_tab_bytes(h), rec_bytes = (size_t)NR * kUseComp * 8;
  const u32 n32 = (u32)n;
  HIPCHK(h, B[US_DELTA].ensure((size_t)J * kUseComp * 8)); HIPCHK(h, B[US_MASK].ensure((size_t)J * 4)); HIPCHK(h, B[US_CTR].ensure(64));
  HIPCHK(h, B[US_SK0].ensure(n * 8)); HIPCHK(h, B[US_SK1].ensure(n * 8)); HIPCHK(h, B[US_SV0].ensure(n * 4)); HIPCHK(h, B[US_SV1].ensure(n * 4));
  HIPCHK(h, B[US_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(n32, kSortTile)))); HIPCHK(h, B[US_SKEY].ensure(n * 4)); HIPCHK(h, B[US_SITEM].ensure(n * 4));
  HIPCHK(h, hipMemsetAsync(B[US_CTR].p, 0, 64, h->stream));
  const DevBuf& src = carry ? B[US_TAB_CUR] : B[US_TAB_SET];
  if (tab_bytes) HIPCHK(h, hipMemcpyAsync(B[US_TAB_WORK].p, src.p, tab_bytes, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));

  UseParams P;
  memset(&P, 0, sizeof P);
  P.J = J; P.op = op; P.Q = (u32)D.Q; P.Pn = (u32)D.Pn; P.NK = NK;
  P.base_uq = (u32)D.base[0]; P.base_up = (u32)D.base[1]; P.base_aq = (u32)D.base[2]; P.base_ap = (u32)D.base[3]; P.base_g = (u32)D.base[4];
  P.ent_user = (u32)D.ent[0]; P.ent_acct = (u32)D.ent[1]; P.ent_qos = (u32)D.ent[2];
  P.user = B[US_JUSER].as<u32>(); P.ua = B[US_JUA].as<u32>(); P.account = B[US_JACCT].as<u32>(); P.qos = B[US_JQOS].as<u32>(); P.part = B[US_JPART].as<u32>();
  P.cpu = jb->cpu_raw ? B[US_JCPU].as<i64>() : nullptr; P.mem = jb->mem ? B[US_JMEM].as<u64>() : nullptr; P.wall = jb->wall_sec ? B[US_JWALL].as<i64>() : nullptr;
  P.jobs = jb->jobs_count ? B[US_JJOBS].as<u32>() : nullptr; P.submit = jb->submit_count ? B[US_JSUB].as<u32>() : nullptr;
  P.nt = jb->name_total ? B[US_JNT].as<u64>() : nullptr; P.cc = jb->class_count ? B[US_JCC].as<u64>() : nullptr;
  P.skip = jb->skip ? B[US_JSKIP].as<uint8_t>() : nullptr;
  P.acct_parent = B[US_PARENT].as<u32>();
  P.src_ex = src.as<uint8_t>() + rec_bytes; P.dst_ex = B[US_TAB_WORK].as<uint8_t>() + rec_bytes;
  P.delta = B[US_DELTA].as<u64>(); P.sort_key = B[US_SK0].as<u64>(); P.mask = B[US_MASK].as<u32>();
  hipLaunchKernelGGL(k_use_items, dim3((J + kUseChunk - 1) / kUseChunk), dim3(256), 0, h->stream, P);

  // (row, slot) items sorted by record id, stable: inside a record the rows stay in call order
  u64* kin = B[US_SK0].as<u64>(); u64* kout = B[US_SK1].as<u64>();
  u32* vin = B[US_SV0].as<u32>(); u32* vout = B[US_SV1].as<u32>();
  sort_index_pairs(h->stream, n32, cns_sort::key_passes(NK), kin, vin, kout, vout, B[US_HIST].as<u32>());
  u64* ctr = B[US_CTR].as<u64>();
  hipLaunchKernelGGL(k_use_gather, dim3((n32 + 255) / 256), dim3(256), 0, h->stream, (const u64*)kin, (const u32*)vin, n32, NK, B[US_SKEY].as<u32>(),
                     B[US_SITEM].as<u32>(), ctr);
  HIPCHK(h, hipGetLastError());
  u64 hc[3] = {0, 0, 0};
  HIPCHK(h, hipMemcpyAsync(hc, ctr, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the number of items that carry a record sizes the scan's grids
  UsePar R;
  memset(&R, 0, sizeof R);
  R.n = (u32)hc[0]; R.nchunks = (R.n + kUseItemChunk - 1) / kUseItemChunk; R.op = op; R.base_g = (u32)D.base[4];
  if (R.n) {
    HIPCHK(h, B[US_TAILS].ensure((size_t)R.nchunks * kUseComp * 8)); HIPCHK(h, B[US_TFLAGS].ensure((size_t)R.nchunks * 4));
    HIPCHK(h, B[US_CARRY].ensure((size_t)R.nchunks * kUseComp * 8)); HIPCHK(h, B[US_CFLAGS].ensure((size_t)R.nchunks * 4));
    R.s_key = B[US_SKEY].as<u32>(); R.s_item = B[US_SITEM].as<u32>(); R.delta = P.delta;
    R.src_rec = src.as<u64>(); R.src_ex = P.src_ex; R.dst_rec = B[US_TAB_WORK].as<u64>(); R.dst_ex = P.dst_ex;
    R.tails = B[US_TAILS].as<u64>(); R.tflags = B[US_TFLAGS].as<u32>(); R.carry = B[US_CARRY].as<u64>(); R.cflags = B[US_CFLAGS].as<u32>();
    R.mask = P.mask; R.ctr = ctr;
    hipLaunchKernelGGL(k_use_tails, dim3(R.nchunks), dim3(256), 0, h->stream, R);
    hipLaunchKernelGGL(k_use_carry, dim3(1), dim3(kUseCarryLanes), 0, h->stream, R);
    hipLaunchKernelGGL(k_use_eval, dim3(R.nchunks), dim3(256), 0, h->stream, R);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  std::vector<u32> mask(J);
  HIPCHK(h, hipMemcpyAsync(mask.data(), P.mask, (size_t)J * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(hc, ctr, 24, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (hc[2]) return fail(h, CNS_ERR_UNSUPPORTED, "cns_usage_apply: a charge takes a count beyond UINT32_MAX or a sum beyond 64 bits; the tables stay as they were");
  float a = 0, b = 0, c = 0;
  HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIPCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  HIPCHK(h, hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
  std::swap(B[US_TAB_CUR].p, B[US_TAB_WORK].p);
  std::swap(B[US_TAB_CUR].cap, B[US_TAB_WORK].cap);
  h->use_have_cur = true;
  u64 clean = 0;
  for (u32 j = 0; j < J; ++j) {
    out->not_found[j] = (uint16_t)(mask[j] & 0xFFFFu);
    out->over_free[j] = (uint16_t)(mask[j] >> 16);
    clean += mask[j] == 0;
  }
  if (out->num_clean) *out->num_clean = clean;
  h->use_timing.h2d_ms = a; h->use_timing.kernels_ms = b; h->use_timing.d2h_ms = c;
  h->use_timing.items = hc[0]; h->use_timing.records = hc[1];
  return CNS_OK;
}

int cns_usage_apply(cns_handle* h, uint32_t op, const cns_usage_jobs* jobs, uint32_t flags, const cns_usage_out* out) {
  if (!h || !jobs) return fail(h, CNS_ERR_INVALID_ARG, "cns_usage_apply: null argument");
  if (!h->use_have) return fail(h, CNS_ERR_STATE, "cns_usage_apply before cns_usage_set_tables");
  if ((flags & CNS_USAGE_CARRY) && !h->use_have_cur) return fail(h, CNS_ERR_STATE, "cns_usage_apply: CNS_USAGE_CARRY before a first cns_usage_apply");
  if (jobs->num_jobs == 0) return CNS_OK;   // nothing asked, nothing written
  if (const auto v = cns_usage_host::check_jobs(h->use_sp, jobs, out, op, nullptr)) return fail(h, v.code, v.msg);
  const int rc = usage_impl(h, op, jobs, flags, out);
  if (rc != 0) drain(h);   // nothing of the call is left in flight, the message survives
  return rc;
}

int cns_usage_get_tables(cns_handle* h, const cns_usage_tables_out* o) {
  if (!h || !o) return fail(h, CNS_ERR_INVALID_ARG, "cns_usage_get_tables: null argument");
  if (!h->use_have) return fail(h, CNS_ERR_STATE, "cns_usage_get_tables before cns_usage_set_tables");
  const cns_acct::Space& D = h->use_sp;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = use_tab_bytes(h);
  std::vector<u64> tab((bytes + 7) / 8, 0ull);
  if (bytes) HIPCHK(h, hipMemcpyAsync(tab.data(), h->d_use[US_TAB_CUR].p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint8_t* ex = reinterpret_cast<const uint8_t*>(tab.data() + (size_t)D.NR * kUseComp);
  cns_usage* use[5] = {o->user_qos, o->user_part, o->acct_qos, o->acct_part, o->qos_usage};
  u32* sub[5] = {o->user_qos_submit, o->user_part_submit, o->acct_qos_submit, o->acct_part_submit, o->qos_submit};
  uint8_t* nex[5] = {o->user_qos_exists, o->user_part_exists, o->acct_qos_exists, o->acct_part_exists, nullptr};
  for (int w = 0; w < 5; ++w) {
    const u64 off = D.base[w];
    for (u64 i = 0; i < D.len[w]; ++i) {
      const u64* r = tab.data() + (size_t)(off + i) * kUseComp;
      if (use[w]) {
        cns_usage& s = use[w][i];
        s.cpu_raw = (int64_t)r[0]; s.mem = r[1]; s.wall_sec = (int64_t)r[2]; s.jobs_count = (u32)r[3]; s.reserved0 = 0;
        for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n) s.name_total[n] = r[5 + n];
        for (u32 g = 0; g < CNS_MAX_GRES_CLASSES; ++g) s.class_count[g] = r[9 + g];
      }
      if (sub[w]) sub[w][i] = (u32)r[4];
      if (nex[w]) nex[w][i] = ex[off + i];
    }
  }
  uint8_t* ent[3] = {o->user_exists, o->acct_exists, o->qos_exists};
  for (int w = 0; w < 3; ++w)
    if (ent[w])
      for (u64 i = 0; i < D.ent_len[w]; ++i) ent[w][i] = ex[D.ent[w] + i];
  return CNS_OK;
}

int cns_usage_get_timing(const cns_handle* h, cns_usage_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->use_timing;
  return CNS_OK;
}

int cns_usage_shape(uint32_t* job_chunk, uint32_t* item_chunk, uint32_t* carry_lanes) {
  if (job_chunk) *job_chunk = kUseChunk;
  if (item_chunk) *item_chunk = kUseItemChunk;
  if (carry_lanes) *carry_lanes = kUseCarryLanes;
  return CNS_OK;
}
