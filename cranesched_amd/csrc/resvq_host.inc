// Host side of include/crane_gpu_resv/resv_probe.h.  Included by engine.hip inside extern "C".
// Host work: validation, the per-node CSR of the reservations (a few entries per node), the buffers.  latest_end, the codes, the pick
// and the earliest-start search run on the device (resvq_kernels.inc; the sort is the radix passes of sort_kernels.inc).  Everything
// lives in cns_engine::d_rq: no flag and no buffer of the cycle or of the probes is read or written, only the node count of cns_set_nodes
// (cns_engine::N together with have_nodes).  No CPU fallback.

constexpr u64 kRqMaxCandidates = 0x7FFFFFFFull;   // of one call
constexpr u64 kRqMaxIntervals = 1ull << 26;       // of one call (DESIGN.md 8): two event times each, 40 bytes per time while they are sorted: 5 GiB at the cap

// CNS_RESVQ_MAX_INTERVALS lowers the cap (tests: the refusal without a huge input); it never raises it
static u64 rq_interval_cap() {
  const char* e = getenv("CNS_RESVQ_MAX_INTERVALS");
  if (!e || !*e) return kRqMaxIntervals;
  return std::min<u64>(kRqMaxIntervals, strtoull(e, nullptr, 10));
}

// the running side of the per-node tables: the arrays k_rq_latest reads, on the host (uploaded into RQ_RAW_*) or on the device where they are
struct RqRunning {
  const i64* end = nullptr;    // [jobs]
  const u32* off = nullptr;    // [jobs + 1]
  const u32* node = nullptr;   // [allocs]
  u32 jobs = 0, allocs = 0;
  bool host = false;
};

// everything behind the running side: the reservations' per-node CSR, latest_end[N].  who: the call's name in front of its messages
static int resvq_set_state_tables(cns_handle* h, const RqRunning& side, const cns_resv_soa* rv, const std::string& who) {
  const u32 N = h->lay.N;
  const u32 RJ = side.jobs, RA = side.allocs;
  const u32 V = rv ? rv->num_resv : 0, VA = V ? rv->alloc_offsets ? rv->alloc_offsets[V] : 0 : 0;
  if (V && (!rv->start_sec || !rv->end_sec || !rv->alloc_offsets || (VA && !rv->alloc_node))) return fail(h, CNS_ERR_INVALID_ARG, who + ": missing array (reservations)");
  // per node: the (start, end) of every reservation that lists it, sorted (the earliest-start walk merges them in this order)
  std::vector<u32> off((size_t)N + 1, 0);
  if (V) {
    if (rv->alloc_offsets[0] != 0) return fail(h, CNS_ERR_INVALID_ARG, who + ": reservation alloc_offsets do not start at 0");
    for (u32 v = 0; v < V; ++v)
      if (rv->alloc_offsets[v] > rv->alloc_offsets[v + 1]) return fail(h, CNS_ERR_INVALID_ARG, who + ": reservation alloc_offsets decrease");
    for (u32 a = 0; a < VA; ++a) {
      if (rv->alloc_node[a] >= N) return fail(h, CNS_ERR_INVALID_ARG, who + ": reservation on a node >= num_nodes");
      ++off[(size_t)rv->alloc_node[a] + 1];
    }
  }
  for (u32 n = 0; n < N; ++n) off[(size_t)n + 1] += off[n];
  std::vector<std::pair<i64, i64>> ent(VA);
  {
    std::vector<u32> fill(off.begin(), off.end() - 1);
    for (u32 v = 0; v < V; ++v)
      for (u32 a = rv->alloc_offsets[v]; a < rv->alloc_offsets[v + 1]; ++a) ent[fill[rv->alloc_node[a]]++] = {rv->start_sec[v], rv->end_sec[v]};
  }
  std::vector<i64> st(std::max<u32>(VA, 1)), ed(std::max<u32>(VA, 1));
  std::vector<u32> cnt(N);
  for (u32 n = 0; n < N; ++n) {
    std::sort(ent.begin() + off[n], ent.begin() + off[(size_t)n + 1]);
    cnt[n] = off[(size_t)n + 1] - off[n];
  }
  for (u32 a = 0; a < VA; ++a) { st[a] = ent[a].first; ed[a] = ent[a].second; }
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_rq;
  if (int rc = upload(h, B[RQ_RVOFF], off)) return rc;
  if (int rc = upload(h, B[RQ_RVST], st)) return rc;
  if (int rc = upload(h, B[RQ_RVED], ed)) return rc;
  HIPCHK(h, B[RQ_LATEST].ensure((size_t)N * 8));
  hipLaunchKernelGGL(k_fill_i64, dim3((N + 255) / 256), dim3(256), 0, h->stream, B[RQ_LATEST].as<i64>(), N, (i64)INT64_MIN);
  HIPCHK(h, hipGetLastError());
  if (RA) {
    const i64* d_end = side.end; const u32* d_off = side.off; const u32* d_node = side.node;
    if (side.host) {
      HIPCHK(h, B[RQ_RAW_END].ensure((size_t)RJ * 8));
      HIPCHK(h, B[RQ_RAW_OFF].ensure(((size_t)RJ + 1) * 4));
      HIPCHK(h, B[RQ_RAW_NODE].ensure((size_t)RA * 4));
      HIPCHK(h, hipMemcpyAsync(B[RQ_RAW_END].p, side.end, (size_t)RJ * 8, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(B[RQ_RAW_OFF].p, side.off, ((size_t)RJ + 1) * 4, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(B[RQ_RAW_NODE].p, side.node, (size_t)RA * 4, hipMemcpyHostToDevice, h->stream));
      d_end = B[RQ_RAW_END].as<i64>(); d_off = B[RQ_RAW_OFF].as<u32>(); d_node = B[RQ_RAW_NODE].as<u32>();
    }
    hipLaunchKernelGGL(k_rq_latest, dim3((RA + 255) / 256), dim3(256), 0, h->stream, d_end, d_off, d_node, RJ, RA, N, B[RQ_LATEST].as<i64>());
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the staging vectors and the caller's arrays are free again)
  h->rq_N = N;
  h->rq_rv_cnt = std::move(cnt);
  h->rq_have = true;
  return CNS_OK;
}

// the running side handed in: its rules, then the shared tables
static int resvq_set_state_impl(cns_handle* h, const cns_running_soa* rn, const cns_resv_soa* rv) {
  const u32 N = h->lay.N;
  const u32 RJ = rn ? rn->num_jobs : 0, RA = rn ? rn->num_allocs : 0;
  if (RJ && (!rn->end_sec || !rn->alloc_offsets || (RA && !rn->alloc_node))) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_set_state: missing array (running)");
  if (RJ) {
    if (rn->alloc_offsets[0] != 0 || rn->alloc_offsets[RJ] != RA) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_set_state: running alloc_offsets do not span num_allocs");
    for (u32 j = 0; j < RJ; ++j)
      if (rn->alloc_offsets[j] > rn->alloc_offsets[j + 1]) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_set_state: running alloc_offsets decrease");
    for (u32 a = 0; a < RA; ++a)
      if (rn->alloc_node[a] >= N) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_set_state: running allocation on a node >= num_nodes");
  }
  RqRunning side;
  if (rn) { side.end = rn->end_sec; side.off = rn->alloc_offsets; side.node = rn->alloc_node; }
  side.jobs = RJ; side.allocs = RA; side.host = true;
  return resvq_set_state_tables(h, side, rv, "cns_resvq_set_state");
}

int cns_resvq_set_state(cns_handle* h, const cns_running_soa* running, const cns_resv_soa* resv) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_set_state: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_resvq_set_state before cns_set_nodes");
  h->rq_have = false;
  const int rc = resvq_set_state_impl(h, running, resv);
  if (rc != 0) drain(h);
  return rc;
}

static int resvq_run_impl(cns_handle* h, i64 now, const cns_resvq_soa* q, cns_resvq_out* out, double* kernel_ms) {
  const u64 Q64 = q->num_queries;
  if (!q->start_sec || !q->duration_sec || !q->node_num || !q->cand_offsets) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: missing array");
  if (Q64 > 0x7FFFFFFFull) return fail(h, CNS_ERR_UNSUPPORTED, "cns_resvq_run: more than 2^31-1 queries");
  const u32 Q = (u32)Q64, N = h->rq_N;
  const auto co = cns_csr::check_offsets(q->cand_offsets, Q);
  if (co.what == cns_csr::Offsets::FirstNot0) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: cand_offsets does not start at 0");
  if (co.what == cns_csr::Offsets::Decreases) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: cand_offsets decrease");
  const u64 L64 = q->cand_offsets[Q];
  if (L64 > kRqMaxCandidates) return fail(h, CNS_ERR_UNSUPPORTED, "cns_resvq_run: more than 2^31-1 candidates in one call");
  const u32 L = (u32)L64;
  if (L && !q->cand_nodes) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: cand_offsets without cand_nodes");
  if (!out->status || !out->start_sec || !out->num_free || !out->chosen_offsets || (L && (!out->code || !out->chosen_nodes)))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: missing result array");
  // per query: k, mode, "in the past"; per list: no node twice; the intervals of the earliest-start search
  std::vector<u32> kq(Q), flags(Q), coff((size_t)Q + 1), choff((size_t)Q + 1, 0), seg_off((size_t)Q + 1, 0);
  bool any_earliest = false;
  for (u32 i = 0; i < Q && q->find_earliest && !any_earliest; ++i) any_earliest = q->find_earliest[i] != 0;
  std::vector<u32> ev_off(any_earliest ? (size_t)L + 1 : 0, 0);   // first event slot per candidate: only a call that searches an earliest start pays for it
  std::vector<u32> stamp(N, 0);
  std::set<u32> beyond;
  u64 chosen_slots = 0, intervals = 0;
  for (u32 i = 0; i < Q; ++i) {
    const i64 s = q->start_sec[i], d = q->duration_sec[i];
    if (d <= 0) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: query " + std::to_string(i) + ": duration_sec <= 0");
    if (s > INT64_MAX - d) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: query " + std::to_string(i) + ": start_sec + duration_sec overflows");
    const u64 b = q->cand_offsets[i], e = q->cand_offsets[i + 1], len = e - b;
    const bool past = s + d <= now, earliest = q->find_earliest && q->find_earliest[i];   // JobScheduler.cpp:4323
    kq[i] = q->node_num[i] ? q->node_num[i] : (u32)len;                                   // :4357-4358
    flags[i] = (earliest ? 1u : 0u) | (past ? 2u : 0u);
    coff[i] = (u32)b;
    seg_off[i] = (u32)std::min<u64>(intervals, 0xFFFFFFFFull);
    chosen_slots += std::min<u64>(kq[i], len);
    choff[(size_t)i + 1] = (u32)chosen_slots;
    beyond.clear();
    for (u64 c = b; c < e; ++c) {
      const u32 n = q->cand_nodes[c];
      bool twice;
      if (any_earliest) ev_off[c] = (u32)std::min<u64>(intervals, 0xFFFFFFFFull);   // (a sum beyond the cap is refused below, before anything reads this)
      if (n < N) { twice = stamp[n] == i + 1; stamp[n] = i + 1; if (earliest && !past) intervals += 1u + h->rq_rv_cnt[n]; }
      else twice = !beyond.insert(n).second;
      if (twice) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: query " + std::to_string(i) + " lists node " + std::to_string(n) + " twice");
    }
  }
  coff[Q] = L;
  if (out->code_capacity < L) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: code_capacity too small");
  if (out->chosen_capacity < chosen_slots) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: chosen_capacity too small");
  const u64 cap = rq_interval_cap();
  if (intervals > cap)
    return fail(h, CNS_ERR_UNSUPPORTED, "cns_resvq_run: " + std::to_string(intervals) + " intervals in the earliest-start queries of one call, the limit is " + std::to_string(cap));
  const u32 EV = (u32)intervals, EV2 = 2 * EV;
  seg_off[Q] = EV;
  if (any_earliest) ev_off[L] = EV;

  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* B = h->d_rq;
  if (int rc = stage(h, B[RQ_START], q->start_sec, (size_t)Q * 8)) return rc;
  if (int rc = stage(h, B[RQ_DUR], q->duration_sec, (size_t)Q * 8)) return rc;
  if (int rc = stage(h, B[RQ_K], kq.data(), (size_t)Q * 4)) return rc;
  if (int rc = stage(h, B[RQ_FLAGS], flags.data(), (size_t)Q * 4)) return rc;
  if (int rc = stage(h, B[RQ_CANDOFF], coff.data(), ((size_t)Q + 1) * 4)) return rc;
  if (int rc = stage(h, B[RQ_CAND], q->cand_nodes, (size_t)L * 4)) return rc;
  if (int rc = stage(h, B[RQ_CHOFF], choff.data(), ((size_t)Q + 1) * 4)) return rc;
  HIPCHK(h, B[RQ_BEST].ensure((size_t)Q * 8));
  HIPCHK(h, B[RQ_CODE].ensure(L));
  HIPCHK(h, B[RQ_CHOSEN].ensure((size_t)chosen_slots * 4));
  HIPCHK(h, B[RQ_STATUS].ensure(Q));
  HIPCHK(h, B[RQ_OSTART].ensure((size_t)Q * 8));
  HIPCHK(h, B[RQ_NFREE].ensure((size_t)Q * 4));
  if (EV) {
    if (int rc = stage(h, B[RQ_EVOFF], ev_off.data(), ((size_t)L + 1) * 4)) return rc;
    if (int rc = stage(h, B[RQ_SEGOFF], seg_off.data(), ((size_t)Q + 1) * 4)) return rc;
    for (int b : {RQ_KA, RQ_KB, RQ_KC, RQ_SORTED}) HIPCHK(h, B[b].ensure((size_t)EV2 * 8));
    for (int b : {RQ_VA, RQ_VB}) HIPCHK(h, B[b].ensure((size_t)EV2 * 4));
    HIPCHK(h, B[RQ_HIST].ensure(cns_sort::hist_bytes(cns_sort::tiles(EV2, kSortTile))));
  }
  RqParams P{};
  P.N = N; P.latest = B[RQ_LATEST].as<i64>(); P.rv_off = B[RQ_RVOFF].as<u32>(); P.rv_st = B[RQ_RVST].as<i64>(); P.rv_ed = B[RQ_RVED].as<i64>();
  P.Q = Q; P.L = L; P.q_start = B[RQ_START].as<i64>(); P.q_dur = B[RQ_DUR].as<i64>(); P.q_k = B[RQ_K].as<u32>(); P.q_flags = B[RQ_FLAGS].as<u32>();
  P.cand_off = B[RQ_CANDOFF].as<u32>(); P.cand = B[RQ_CAND].as<u32>(); P.chosen_off = B[RQ_CHOFF].as<u32>();
  P.EV = EV; P.ev_off = B[RQ_EVOFF].as<u32>(); P.seg_off = B[RQ_SEGOFF].as<u32>(); P.ev_key = B[RQ_KA].as<u64>(); P.ev_seg = B[RQ_VA].as<u32>();
  P.plus_s = B[RQ_SORTED].as<i64>(); P.minus_s = B[RQ_SORTED].as<i64>() + EV; P.best = B[RQ_BEST].as<i64>();
  P.code = B[RQ_CODE].as<uint8_t>(); P.chosen = B[RQ_CHOSEN].as<u32>(); P.status = B[RQ_STATUS].as<uint8_t>();
  P.o_start = B[RQ_OSTART].as<i64>(); P.num_free = B[RQ_NFREE].as<u32>();

  const dim3 blk(kRqBlock);
  auto grid = [](u64 n) { return dim3((unsigned)((n + kRqBlock - 1) / kRqBlock)); };
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  hipLaunchKernelGGL(k_fill_i64, grid(Q), blk, 0, h->stream, P.best, Q, kRqNever);
  HIPCHK(h, hipGetLastError());
  if (EV) {
    hipLaunchKernelGGL(k_rq_emit, grid(L), blk, 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    // all 2 EV event times by (segment, time), stable LSD passes: the 8 digits of the time, then the digits of the segment number
    u32* hist = B[RQ_HIST].as<u32>();
    u64 *ka = B[RQ_KA].as<u64>(), *kb = B[RQ_KB].as<u64>(), *kc = B[RQ_KC].as<u64>();
    u32 *va = B[RQ_VA].as<u32>(), *vb = B[RQ_VB].as<u32>();
    sort_pairs(h->stream, EV2, 8, ka, va, kb, vb, hist);                         // an even number of passes: the times in order are in RQ_KA again, their segments in RQ_VA
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_rq_by_segment, grid(EV2), blk, 0, h->stream, (const u32*)va, kb, vb, EV2);
    HIPCHK(h, hipGetLastError());
    sort_pairs(h->stream, EV2, cns_resvq::seg_passes(Q), kb, vb, kc, va, hist);  // (key, value) = (segment, position in time order); afterwards in (kb, vb)
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_rq_gather, grid(EV2), blk, 0, h->stream, (const u64*)ka, (const u32*)vb, B[RQ_SORTED].as<i64>(), EV2);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_rq_first, grid(EV), blk, 0, h->stream, P, EV);
    HIPCHK(h, hipGetLastError());
  }
  if (L) {
    hipLaunchKernelGGL(k_rq_classify, grid(L), blk, 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
  }
  hipLaunchKernelGGL(k_rq_pick, dim3(std::min<u32>(Q, kRqPickGrid)), blk, 0, h->stream, P);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  // results: the per-query arrays and the codes as they are, the chosen nodes through their slots
  std::vector<u32> slots((size_t)chosen_slots);
  HIPCHK(h, hipMemcpyAsync(out->status, P.status, Q, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out->start_sec, P.o_start, (size_t)Q * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out->num_free, P.num_free, (size_t)Q * 4, hipMemcpyDeviceToHost, h->stream));
  if (L) HIPCHK(h, hipMemcpyAsync(out->code, P.code, L, hipMemcpyDeviceToHost, h->stream));
  if (chosen_slots) HIPCHK(h, hipMemcpyAsync(slots.data(), P.chosen, (size_t)chosen_slots * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (kernel_ms) *kernel_ms = ms;
  u64 w = 0;
  for (u32 i = 0; i < Q; ++i) {
    out->chosen_offsets[i] = w;
    if (out->status[i] != CNS_RESVQ_OK) continue;
    if (kq[i]) memcpy(out->chosen_nodes + w, slots.data() + choff[i], (size_t)kq[i] * 4);   // OK: k <= num_free <= list length, the slots hold k
    w += kq[i];
  }
  out->chosen_offsets[Q] = w;
  return CNS_OK;
}

int cns_resvq_run(cns_handle* h, int64_t now_sec, const cns_resvq_soa* q, cns_resvq_out* out, double* kernel_ms) {
  if (!h || !q) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: null argument");
  if (kernel_ms) *kernel_ms = 0.0;
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_resvq_run before cns_set_nodes, or after a new one without cns_resvq_set_state");
  if (!h->rq_have) return fail(h, CNS_ERR_STATE, "cns_resvq_run before cns_resvq_set_state");
  if (q->num_queries == 0) return CNS_OK;   // nothing asked, nothing written
  if (!out) return fail(h, CNS_ERR_INVALID_ARG, "cns_resvq_run: null result");
  const int rc = resvq_run_impl(h, now_sec, q, out, kernel_ms);
  if (rc != 0) drain(h);
  return rc;
}

int cns_resvq_shape(uint32_t* pick_block, uint32_t* pick_grid, uint32_t* sort_tile, uint32_t* scan_span) {
  if (pick_block) *pick_block = kRqBlock;
  if (pick_grid) *pick_grid = kRqPickGrid;
  if (sort_tile) *sort_tile = kSortTile;
  if (scan_span) *scan_span = kSortScanSpan;
  return CNS_OK;
}
