// The steps of a JobTable (engine.hip): one uploaded cns_job_soa, its 64-dword records and its packed results.  Included by engine.hip
// inside its unnamed namespace.  cns_upload_jobs / cns_run_resident / cns_download sequence them on the cycle's queue (cns_engine::q),
// the cns_probe_* calls (probe_host.inc) on the probes (cns_engine::pt); what only one of the two does stays with that caller.

// What a caller's table is called in the messages of the shared steps: each caller keeps its own wording, whole.
struct TableMsgs { const char *missing, *too_many, *no_lists, *capacity, *missing_out, *need_wide; };
const TableMsgs kQueueMsgs{"cns_upload_jobs: missing array", "more than 2^32-16 jobs", "cns_upload_jobs: include / exclude offsets without node lists",
                           "cns_download: place_capacity too small", "cns_download: missing result array",
                           "cns_download: the snapshot has nodes with core ids above 127: core_w2 / core_w3 are required"};
const TableMsgs kProbeMsgs{"cns_probe_upload: missing array", "more than 2^32-16 probes", "cns_probe_upload: include / exclude offsets without node lists",
                           "cns_probe_download: place_capacity too small", "cns_probe_download: missing result array",
                           "cns_probe_download: the snapshot has nodes with core ids above 127: core_w2 / core_w3 are required"};

// The arrays every job needs, and the widest table (the queue invalidates its cycle only behind these, so they are a step of their own)
int table_check(cns_engine* h, const cns_job_soa* jb, const TableMsgs& m) {
  if (jb->num_jobs && (!jb->partition || !jb->time_limit_sec || !jb->node_mem || !jb->task_cpu_raw || !jb->task_mem ||
                       !jb->node_num || !jb->ntasks || !jb->ntasks_per_node_min || !jb->ntasks_per_node_max))
    return fail(h, CNS_ERR_INVALID_ARG, m.missing);
  if (jb->num_jobs > 0xFFFFFFF0ull) return fail(h, CNS_ERR_UNSUPPORTED, m.too_many);
  return 0;
}

// Offsets that name nodes without the list that holds them.  The queue reports this behind pass 1's validation, the probes in front
// of their copies: each caller places the step itself.
int table_lists_check(cns_engine* h, const cns_job_soa* jb, const TableMsgs& m) {
  const u64 J = jb->num_jobs;
  if ((jb->incl_offsets && !jb->incl_nodes && jb->incl_offsets[J]) || (jb->excl_offsets && !jb->excl_nodes && jb->excl_offsets[J]))
    return fail(h, CNS_ERR_INVALID_ARG, m.no_lists);
  return 0;
}

// The caller's arrays go to the device as they are (k_pack_jobs builds the 64-dword job records there); from page-locked arrays
// (cns_host_alloc) these are DMA transfers the thread does not wait for, and both host passes run in their shadow.  An optional array
// that is absent is not staged (stage() issues no copy from a null source: a missing node list costs nothing here).
int table_stage(cns_engine* h, JobTable& T, const cns_job_soa* jb) {
  const u64 J = jb->num_jobs;
  const u64 n_incl = jb->incl_offsets ? jb->incl_offsets[J] : 0, n_excl = jb->excl_offsets ? jb->excl_offsets[J] : 0;
  const struct { DevBuf& buf; const void* src; size_t bytes; bool optional; } arrays[] = {
      {T.raw[JR_LIMIT], jb->time_limit_sec, J * 8, false},          {T.raw[JR_NCPU], jb->node_cpu_raw, J * 8, true},
      {T.raw[JR_NMEM], jb->node_mem, J * 8, false},                 {T.raw[JR_TCPU], jb->task_cpu_raw, J * 8, false},
      {T.raw[JR_TMEM], jb->task_mem, J * 8, false},                 {T.raw[JR_K], jb->node_num, J * 4, false},
      {T.raw[JR_NTASKS], jb->ntasks, J * 4, false},                 {T.raw[JR_TMIN], jb->ntasks_per_node_min, J * 4, false},
      {T.raw[JR_TMAX], jb->ntasks_per_node_max, J * 4, false},      {T.raw[JR_EXCL], jb->exclusive, J, true},
      {T.raw[JR_GTOT], jb->gres_total, J * CNS_MAX_GRES_NAMES, true}, {T.raw[JR_GSPEC], jb->gres_spec, J * CNS_MAX_GRES_CLASSES, true},
      {T.raw[JR_INCL_OFF], jb->incl_offsets, (J + 1) * 8, true},    {T.raw[JR_EXCL_OFF], jb->excl_offsets, (J + 1) * 8, true},
      {T.incl, jb->incl_nodes, n_incl * 4, false},                  {T.excl, jb->excl_nodes, n_excl * 4, false}};
  for (const auto& a : arrays)
    if (a.src || !a.optional)
      if (int rc = stage(h, a.buf, a.src, a.bytes)) return rc;
  return 0;
}

// The pre-checks and the routing of the ordered loop (jobs_host.inc: pass 1 on a few host threads, pass 2 behind it) against the
// handle's snapshot, into the table's page-locked buffers; `batch`: the jobs that reach an ordered loop at most.  O keeps the counts
// for table_layout and what only the queue reads (pj_off, algo, n_shaped).  A table that fails pass 1: its status, the message behind
// the caller's `prefix`.
int table_route(cns_engine* h, JobTable& T, const cns_job_soa* jb, u64 batch, const char* prefix, cns_jobs_host::Out& O) {
  namespace jh = cns_jobs_host;
  const u64 J = jb->num_jobs, J1 = std::max<u64>(J, 1);
  HIPCHK(h, T.h_reason.ensure(J1));
  HIPCHK(h, T.h_place.ensure((J + 1) * 8));
  if (h->lay.shared) HIPCHK(h, T.h_jtag.ensure(J1));
  T.job_part.resize((size_t)J);
  jh::Route R;
  R.P = h->rlay.P; R.Pu = h->lay.Pu; R.P_real = h->lay.P_real; R.V = h->rlay.V;
  R.upart_refused = h->lay.upart_refused.data(); R.upart_eng = h->lay.upart_eng.data(); R.upart_size = h->lay.upart_size.data();
  R.upart_tag = h->lay.upart_tag.data(); R.part_off = h->rlay.part_off.data();
  R.s_node = h->rlay.big_nodes ? 48 : 32; R.gres_classes = h->gres.num_classes; R.batch = batch;
  O.reason = T.h_reason.as<uint8_t>(); O.job_part = T.job_part.data(); O.place_off = T.h_place.as<u64>();
  O.jtag = h->lay.shared ? T.h_jtag.as<uint8_t>() : nullptr;
  std::vector<jh::Chunk> chunks;
  std::string perr;
  if (const int rc = jh::pass1(jb, R, O, chunks, jh::threads_for(J, h->host_threads), &perr)) return fail(h, rc, prefix + perr);
  HIPCHK(h, T.h_grouped.ensure(std::max<u64>(O.Jg, 1) * 4));
  O.grouped = T.h_grouped.as<u32>();
  jh::pass2(jb, O, chunks);   // the offsets of the placement records and the table grouped by partition in queue order, one u32 per job
  if (J == 0) { O.reason[0] = CNS_REASON_NONE; if (O.jtag) O.jtag[0] = 0; }   // (the one-element stand-ins of an empty table)
  if (O.Jg == 0) O.grouped[0] = 0;
  return 0;
}

// What the host pass computed goes to the device, and k_pack_jobs builds the records of the jobs that were routed.
int table_pack(cns_engine* h, JobTable& T, const cns_job_soa* jb) {
  const u64 J1 = std::max<u64>(T.J, 1), Jg1 = std::max<u64>(T.Jg, 1);
  if (int rc = stage(h, T.raw[JR_PLACE_OFF], T.h_place.p, (T.J + 1) * 8)) return rc;
  if (int rc = stage(h, T.raw[JR_GROUPED], T.h_grouped.p, Jg1 * 4)) return rc;
  if (h->lay.shared) { if (int rc = stage(h, T.jtag, T.h_jtag.p, J1)) return rc; }
  if (int rc = stage(h, T.reason_init, T.h_reason.p, J1)) return rc;
  HIPCHK(h, T.jobs.ensure((size_t)Jg1 * kJobRecDwords * 4));
  if (!T.Jg) return 0;
  const DevBuf* r = T.raw;
  PackParams K{};
  K.Jg = T.Jg; K.grouped = r[JR_GROUPED].as<u32>();
  K.L = r[JR_LIMIT].as<i64>(); K.ncpu = jb->node_cpu_raw ? r[JR_NCPU].as<i64>() : nullptr; K.nmem = r[JR_NMEM].as<u64>();
  K.tcpu = r[JR_TCPU].as<i64>(); K.tmem = r[JR_TMEM].as<u64>(); K.k = r[JR_K].as<u32>(); K.ntasks = r[JR_NTASKS].as<u32>();
  K.tmin = r[JR_TMIN].as<u32>(); K.tmax = r[JR_TMAX].as<u32>();
  K.excl = jb->exclusive ? r[JR_EXCL].as<uint8_t>() : nullptr;
  K.gtot = jb->gres_total ? r[JR_GTOT].as<uint8_t>() : nullptr; K.gspec = jb->gres_spec ? r[JR_GSPEC].as<uint8_t>() : nullptr;
  K.incl_off = jb->incl_offsets ? r[JR_INCL_OFF].as<u64>() : nullptr; K.excl_off = jb->excl_offsets ? r[JR_EXCL_OFF].as<u64>() : nullptr;
  K.place_off = r[JR_PLACE_OFF].as<u64>(); K.jobrec = T.jobs.as<u32>();
  K.tag = h->lay.shared ? T.jtag.as<uint8_t>() : nullptr;
  hipLaunchKernelGGL(k_pack_jobs, dim3((unsigned)((T.Jg + 255) / 256)), dim3(256), 0, h->stream, K);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The table's counts as the host pass found them, and its result buffer laid out for them (jobs_host.inc: result_layout): set here
// and nowhere else, so counts and layout agree whichever way an upload ends.
int table_layout(cns_engine* h, JobTable& T, const cns_job_soa* jb, const cns_jobs_host::Out& O) {
  T.J = jb->num_jobs; T.Jg = O.Jg; T.places = O.places;
  T.ro = cns_jobs_host::result_layout(T.J, T.places, h->lay.wide_cores);
  HIPCHK(h, T.results.ensure(T.ro.total));
  return 0;
}

// The result buffer in front of a pass.  result_layout's section order is what lets one memset cover start and the 8-byte records.
int table_reset(cns_engine* h, JobTable& T) {
  char* rb = T.results.as<char>();
  const cns_jobs_host::ResOff& ro = T.ro;
  const u64 pl = std::max<u64>(T.places, 1), J1 = std::max<u64>(T.J, 1);
  HIPCHK(h, hipMemsetAsync(rb + ro.start, 0, ro.node - ro.start, h->stream));
  HIPCHK(h, hipMemsetAsync(rb + ro.node, 0xFF, 4 * pl, h->stream));   // CNS_NODE_NONE
  HIPCHK(h, hipMemsetAsync(rb + ro.ntasks, 0, 4 * pl, h->stream));
  if (h->lay.wide_cores) HIPCHK(h, hipMemsetAsync(rb + ro.c2, 0, ro.total - ro.c2, h->stream));   // core ids 128..255 of the records
  HIPCHK(h, hipMemcpyAsync(rb + ro.reason, T.reason_init.p, J1, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

// The table's records, node lists and result arrays in a kernel's parameter block
void table_bind(const cns_engine* h, const JobTable& T, KParams& K) {
  char* rb = T.results.as<char>();
  const cns_jobs_host::ResOff& ro = T.ro;
  K.jobrec = T.jobs.as<u32>(); K.incl_nodes = T.incl.as<u32>(); K.excl_nodes = T.excl.as<u32>();
  K.o_start = (i64*)(rb + ro.start); K.o_cpu = (i64*)(rb + ro.cpu); K.o_mem = (u64*)(rb + ro.mem); K.o_clo = (u64*)(rb + ro.clo);
  K.o_chi = (u64*)(rb + ro.chi); K.o_gres = (u64*)(rb + ro.gres); K.o_node = (u32*)(rb + ro.node); K.o_ntasks = (u32*)(rb + ro.ntasks);
  K.o_reason = (uint8_t*)(rb + ro.reason);
  K.o_c2 = h->lay.wide_cores ? (u64*)(rb + ro.c2) : nullptr; K.o_c3 = h->lay.wide_cores ? (u64*)(rb + ro.c3) : nullptr;
}

// The results into the caller's arrays: the copies are on the stream when this returns, the caller waits for them.
int table_download(cns_engine* h, const JobTable& T, cns_placement_soa* out, const TableMsgs& m) {
  if (out->place_capacity < T.places) return fail(h, CNS_ERR_INVALID_ARG, m.capacity);
  if (!out->start_sec || !out->reason || !out->place_offsets || !out->node_idx || !out->ntasks || !out->cpu_raw ||
      !out->mem || !out->core_lo || !out->core_hi || !out->gres)
    return fail(h, CNS_ERR_INVALID_ARG, m.missing_out);
  if (h->lay.wide_cores && (!out->core_w2 || !out->core_w3)) return fail(h, CNS_ERR_INVALID_ARG, m.need_wide);
  const char* rb = T.results.as<char>();
  const cns_jobs_host::ResOff& ro = T.ro;
  const size_t J = (size_t)T.J, pl = (size_t)T.places;
  const struct { void* dst; size_t off, bytes; } parts[] = {
      {out->start_sec, ro.start, 8 * J}, {out->reason, ro.reason, J},     {out->cpu_raw, ro.cpu, 8 * pl},  {out->mem, ro.mem, 8 * pl},
      {out->core_lo, ro.clo, 8 * pl},    {out->core_hi, ro.chi, 8 * pl},  {out->gres, ro.gres, 8 * pl},    {out->node_idx, ro.node, 4 * pl},
      {out->ntasks, ro.ntasks, 4 * pl},  {out->core_w2, ro.c2, h->lay.wide_cores ? 8 * pl : 0}, {out->core_w3, ro.c3, h->lay.wide_cores ? 8 * pl : 0}};
  for (const auto& p : parts)
    if (p.bytes) HIPCHK(h, hipMemcpyAsync(p.dst, rb + p.off, p.bytes, hipMemcpyDeviceToHost, h->stream));
  if (!h->lay.wide_cores) {
    if (out->core_w2 && pl) memset(out->core_w2, 0, 8 * pl);
    if (out->core_w3 && pl) memset(out->core_w3, 0, 8 * pl);
  }
  return 0;
}
// ... and the place offsets: a host copy, made in the shadow of those transfers
void table_offsets(const JobTable& T, cns_placement_soa* out) { memcpy(out->place_offsets, T.h_place.p, 8 * ((size_t)T.J + 1)); }
