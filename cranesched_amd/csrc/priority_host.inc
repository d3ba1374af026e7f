// Host side of cns_priority_order (include/crane_gpu/priority.h).  Included by engine.hip inside extern "C".
// Packing done here on the host: the CSR of running jobs per account (stable, O(R)) and the "account is
// present" flags — both are pure data layout; every min/max, every fp64 operation and the sort run on the GPU.

// The pieces cns_priority_order and cns_priority_order_resident (running_attrs_host.inc) share: the upload of the pending side, the
// scratch and the initial bounds, the parameter block over cns_engine::d_prio, the launches and the download.

static int prio_stage_pending(cns_handle* h, const cns_prio_pending_soa* pd, u32 J) {
  DevBuf* pb = h->d_prio;  // (buf_slots.h)
  if (int rc = stage(h, pb[PR_SUBMIT], pd->submit_sec, (size_t)J * 8)) return rc;
  if (int rc = stage(h, pb[PR_QOS], pd->qos_priority, (size_t)J * 4)) return rc;
  if (int rc = stage(h, pb[PR_PART], pd->partition_priority, (size_t)J * 4)) return rc;
  if (int rc = stage(h, pb[PR_NODENUM], pd->node_num, (size_t)J * 4)) return rc;
  if (int rc = stage(h, pb[PR_CPU], pd->total_cpu_raw, (size_t)J * 8)) return rc;
  if (int rc = stage(h, pb[PR_MEM], pd->total_mem, (size_t)J * 8)) return rc;
  if (int rc = stage(h, pb[PR_ACCT], pd->account, (size_t)J * 4)) return rc;
  if (pd->cached_priority) { if (int rc = stage(h, pb[PR_CACHED], pd->cached_priority, (size_t)J * 8)) return rc; }
  return 0;
}

static PrioBounds prio_bounds_start() {
  PrioBounds B0{};
  B0.age_max = 0; B0.age_min = ~0ull; B0.mem_max = 0; B0.mem_min = ~0ull;
  B0.cpus_max_bits = 0;  // bits of 0.0
  {
    const double dmax = std::numeric_limits<double>::max();
    memcpy(&B0.cpus_min_bits, &dmax, 8);
  }
  B0.sv_max = 0.0; B0.sv_min = 4294967295.0;
  B0.qos_max = 0; B0.qos_min = ~0u; B0.part_max = 0; B0.part_min = ~0u; B0.nn_max = 0; B0.nn_min = ~0u;
  return B0;
}

static int prio_scratch(cns_handle* h, u32 J, u32 R, u32 A) {
  DevBuf* pb = h->d_prio;
  static const PrioBounds B0 = prio_bounds_start();   // (outlives the copy)
  if (int rc = stage(h, pb[PR_BOUNDS], &B0, sizeof B0)) return rc;
  HIPCHK(h, pb[PR_ACCVAL].ensure((size_t)std::max<u32>(A, 1) * 8));
  HIPCHK(h, pb[PR_PRIO].ensure((size_t)J * 8));
  HIPCHK(h, pb[PR_K0].ensure((size_t)J * 8));
  HIPCHK(h, pb[PR_K1].ensure((size_t)J * 8));
  HIPCHK(h, pb[PR_V0].ensure((size_t)J * 4));
  HIPCHK(h, pb[PR_V1].ensure((size_t)J * 4));
  HIPCHK(h, pb[PR_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(J, kSortTile))));  // [digit][tile] table + 256 row totals
  HIPCHK(h, pb[PR_TERMS].ensure((size_t)std::max<u32>(R, 1) * 8));
  return 0;
}

// every pointer names its slot of d_prio; cns_priority_order_resident rebinds the running side to the ledger's buffers
static PrioParams prio_params(cns_handle* h, int64_t now_sec, const cns_priority_config* cfg, u32 J, u32 R, u32 A, bool cached) {
  DevBuf* pb = h->d_prio;
  PrioParams P{};
  P.now = now_sec; P.max_age = cfg->max_age_sec;
  P.w_age = cfg->weight_age; P.w_fair = cfg->weight_fair_share; P.w_size = cfg->weight_job_size;
  P.w_part = cfg->weight_partition; P.w_qos = cfg->weight_qos; P.favor_small = cfg->favor_small ? 1u : 0u;
  P.J = J; P.R = R; P.A = A;
  P.submit = pb[PR_SUBMIT].as<i64>(); P.qos = pb[PR_QOS].as<u32>(); P.part = pb[PR_PART].as<u32>(); P.node_num = pb[PR_NODENUM].as<u32>();
  P.cpu_raw = pb[PR_CPU].as<i64>(); P.mem = pb[PR_MEM].as<u64>(); P.account = pb[PR_ACCT].as<u32>();
  P.cached = cached ? pb[PR_CACHED].as<double>() : nullptr;
  P.r_start = pb[PR_RSTART].as<i64>(); P.r_qos = pb[PR_RQOS].as<u32>(); P.r_part = pb[PR_RPART].as<u32>(); P.r_node_num = pb[PR_RNODENUM].as<u32>();
  P.r_cpu_raw = pb[PR_RCPU].as<i64>(); P.r_mem = pb[PR_RMEM].as<u64>(); P.r_account = pb[PR_RACCT].as<u32>();
  P.acc_off = pb[PR_ACCOFF].as<u32>(); P.acc_jobs = pb[PR_ACCJOBS].as<u32>(); P.acc_present = pb[PR_PRESENT].as<uint8_t>();
  P.bounds = pb[PR_BOUNDS].as<PrioBounds>(); P.acc_val = pb[PR_ACCVAL].as<double>(); P.prio = pb[PR_PRIO].as<double>();
  P.keys = pb[PR_K0].as<u64>();
  P.terms = pb[PR_TERMS].as<double>();
  return P;
}

// bounds, service values, priorities, the sort, the download; record_start: ev[0] is recorded here (else the caller did, in front of
// device work of its own)
static int prio_launch(cns_handle* h, const PrioParams& P, bool record_start, uint32_t* order_out, double* priority_out) {
  DevBuf* pb = h->d_prio;
  const u32 J = P.J, R = P.R, A = P.A;
  if (record_start) HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  const u32 rb = std::min<u32>(512u, (std::max(J, R) + 255u) / 256u);
  hipLaunchKernelGGL(k_prio_bounds, dim3(rb), dim3(256), 0, h->stream, P);
  if (A) {
    if (R) hipLaunchKernelGGL(k_prio_terms, dim3((R + 255) / 256), dim3(256), 0, h->stream, P);
    hipLaunchKernelGGL(k_prio_service, dim3((A + 255) / 256), dim3(256), 0, h->stream, P);
    hipLaunchKernelGGL(k_prio_service_bounds, dim3(1), dim3(256), 0, h->stream, P);
  }
  hipLaunchKernelGGL(k_prio_calc, dim3((J + 255) / 256), dim3(256), 0, h->stream, P);
  u64* kin = pb[PR_K0].as<u64>(); u64* kout = pb[PR_K1].as<u64>();
  u32* vin = pb[PR_V0].as<u32>(); u32* vout = pb[PR_V1].as<u32>();
  sort_index_pairs(h->stream, J, 8, kin, vin, kout, vout, pb[PR_HIST].as<u32>());   // the keys use all 64 bits: 8 passes, whatever J
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipMemcpyAsync(order_out, vin, (size_t)J * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(priority_out, P.prio, (size_t)J * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->prio_ms = ms;
  return 0;
}

int cns_priority_order(cns_handle* h, int64_t now_sec, const cns_priority_config* cfg, uint32_t num_accounts,
                       const cns_prio_pending_soa* pd, const cns_prio_running_soa* rn, uint64_t limit,
                       uint32_t* order_out, double* priority_out, uint64_t* num_ordered) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_priority_order: null handle");
  if (!cfg || !pd || !num_ordered) return fail(h, CNS_ERR_INVALID_ARG, "cns_priority_order: null argument");
  const u32 J = pd->num_jobs, R = rn ? rn->num_jobs : 0, A = num_accounts;
  if (J && (!pd->submit_sec || !pd->qos_priority || !pd->partition_priority || !pd->node_num || !pd->total_cpu_raw ||
            !pd->total_mem || !pd->account || !order_out || !priority_out))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_priority_order: missing pending array");
  if (R && (!rn->start_sec || !rn->qos_priority || !rn->partition_priority || !rn->node_num || !rn->alloc_cpu_raw ||
            !rn->alloc_mem || !rn->account))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_priority_order: missing running array");
  HIPCHK(h, hipSetDevice(h->device));
  *num_ordered = std::min<uint64_t>(J, limit);
  h->prio_ms = 0.0; h->prio_bytes = 0;
  if (J == 0) return CNS_OK;

  // ---- host packing: account CSR over the running jobs (vector order kept), presence flags ----
  std::vector<u32> acc_off(A + 1, 0), acc_jobs(R);
  std::vector<uint8_t> present(std::max<u32>(A, 1), 0);
  for (u32 i = 0; i < J; ++i) {
    if (pd->account[i] >= A) return fail(h, CNS_ERR_INVALID_ARG, "pending job account >= num_accounts");
    if (pd->total_cpu_raw[i] < 0) return fail(h, CNS_ERR_INVALID_ARG, "negative cpu request");
    present[pd->account[i]] = 1;
  }
  for (u32 i = 0; i < R; ++i) {
    if (rn->account[i] >= A) return fail(h, CNS_ERR_INVALID_ARG, "running job account >= num_accounts");
    if (rn->alloc_cpu_raw[i] < 0) return fail(h, CNS_ERR_INVALID_ARG, "negative cpu allocation");
    present[rn->account[i]] = 1;
    acc_off[rn->account[i] + 1]++;
  }
  for (u32 a = 0; a < A; ++a) acc_off[a + 1] += acc_off[a];
  {
    std::vector<u32> cur(acc_off.begin(), acc_off.end() - 1);
    for (u32 i = 0; i < R; ++i) acc_jobs[cur[rn->account[i]]++] = i;
  }

  // ---- upload ----
  DevBuf* pb = h->d_prio;  // (buf_slots.h)
  if (int rc = prio_stage_pending(h, pd, J)) return rc;
  if (R) {
    if (int rc = stage(h, pb[PR_RSTART], rn->start_sec, (size_t)R * 8)) return rc;
    if (int rc = stage(h, pb[PR_RQOS], rn->qos_priority, (size_t)R * 4)) return rc;
    if (int rc = stage(h, pb[PR_RPART], rn->partition_priority, (size_t)R * 4)) return rc;
    if (int rc = stage(h, pb[PR_RNODENUM], rn->node_num, (size_t)R * 4)) return rc;
    if (int rc = stage(h, pb[PR_RCPU], rn->alloc_cpu_raw, (size_t)R * 8)) return rc;
    if (int rc = stage(h, pb[PR_RMEM], rn->alloc_mem, (size_t)R * 8)) return rc;
    if (int rc = stage(h, pb[PR_RACCT], rn->account, (size_t)R * 4)) return rc;
  }
  if (int rc = stage(h, pb[PR_ACCOFF], acc_off.data(), acc_off.size() * 4)) return rc;
  if (int rc = stage(h, pb[PR_ACCJOBS], acc_jobs.data(), (size_t)R * 4)) return rc;
  if (int rc = stage(h, pb[PR_PRESENT], present.data(), present.size())) return rc;
  if (int rc = prio_scratch(h, J, R, A)) return rc;

  // ---- device work ----
  if (int rc = prio_launch(h, prio_params(h, now_sec, cfg, J, R, A, pd->cached_priority != nullptr), true, order_out, priority_out)) return rc;
  // bytes by construction: bounds + calc each stream the pending SoA (48 B / job, + 8 B cached), the running
  // SoA is read twice (36 B / job), calc writes prio + key (16 B), each sort pass reads keys twice + values once
  // and writes both (8 + 8 + 4 + 12 = 32 B / element), iota 4 B
  h->prio_bytes = (u64)J * (48 + 48 + 16 + 4 + 8ull * 32) + (u64)R * (36 + 36 + 4 + 16) + (pd->cached_priority ? (u64)J * 8 : 0);
  return CNS_OK;
}

int cns_priority_timing(const cns_handle* h, double* kernels_ms, uint64_t* algorithmic_bytes) {
  if (!h) return CNS_ERR_INVALID_ARG;
  if (kernels_ms) *kernels_ms = h->prio_ms;
  if (algorithmic_bytes) *algorithmic_bytes = h->prio_bytes;
  return CNS_OK;
}
