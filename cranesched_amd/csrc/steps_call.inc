// Device side of cns_schedule_steps (include/crane_gpu/steps.h).  Included by engine.hip inside extern "C".
// The argument checks and the re-layout are cns_steps::pack (steps_host.inc, no HIP in there); what it returns is uploaded as it is.
// Every feasibility test, the top-k queue and the allocations run on the GPU.  No CPU fallback.

int cns_schedule_steps(cns_handle* h, const cns_step_job_soa* jb, const cns_step_soa* st, cns_step_result_soa* out,
                       double* kernel_ms) {
  if (!h || !jb || !st || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_schedule_steps: null argument");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_schedule_steps before cns_set_nodes (the GRES layout comes with the nodes)");
  cns_steps::Packed pk;
  if (const cns_steps::Status s = cns_steps::pack(h->gres.num_classes, jb, st, out, pk)) return fail(h, s.code, s.msg);
  const u32 Jn = jb->num_jobs, S = st->num_steps, Nn = jb->num_nodes;
  const u64 places = pk.places, tasks = pk.tasks;
  const u32 n_incl = pk.n_incl, n_excl = pk.n_excl;
  std::vector<StepRec>& recs = pk.recs;
  std::vector<Res>& avail = pk.avail;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf* b = h->d_step;  // (buf_slots.h)
  if (int rc = stage(h, b[ST_NODEOFF], jb->node_offsets, ((size_t)Jn + 1) * 4)) return rc;
  if (int rc = stage(h, b[ST_NODEIDX], jb->node_idx, (size_t)Nn * 4)) return rc;
  if (int rc = upload(h, b[ST_AVAIL], avail)) return rc;
  if (int rc = stage(h, b[ST_STEPOFF], jb->step_offsets, ((size_t)Jn + 1) * 4)) return rc;
  if (int rc = upload(h, b[ST_STEPS], recs)) return rc;
  if (int rc = stage(h, b[ST_INCL], st->incl_nodes, (size_t)n_incl * 4)) return rc;
  if (int rc = stage(h, b[ST_EXCL], st->excl_nodes, (size_t)n_excl * 4)) return rc;
  const size_t pl = std::max<u64>(places, 1), tk = std::max<u64>(tasks, 1);
  HIPCHK(h, b[ST_SCHEDULED].ensure(std::max<u32>(S, 1))); HIPCHK(h, b[ST_ONODE].ensure(pl * 4)); HIPCHK(h, b[ST_ONT].ensure(pl * 4)); HIPCHK(h, b[ST_OALLOC].ensure(pl * sizeof(Res)));
  HIPCHK(h, b[ST_TNODE].ensure(tk * 4)); HIPCHK(h, b[ST_TALLOC].ensure(tk * sizeof(Res)));
  HIPCHK(h, hipMemsetAsync(b[ST_SCHEDULED].p, 0, std::max<u32>(S, 1), h->stream));
  HIPCHK(h, hipMemsetAsync(b[ST_ONODE].p, 0xFF, pl * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(b[ST_ONT].p, 0, pl * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(b[ST_OALLOC].p, 0, pl * sizeof(Res), h->stream));
  HIPCHK(h, hipMemsetAsync(b[ST_TNODE].p, 0xFF, tk * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(b[ST_TALLOC].p, 0, tk * sizeof(Res), h->stream));
  StepParams P;
  memset(&P, 0, sizeof P);
  P.num_jobs = Jn;
  P.node_off = b[ST_NODEOFF].as<u32>(); P.node_idx = b[ST_NODEIDX].as<u32>(); P.avail = b[ST_AVAIL].as<Res>(); P.step_off = b[ST_STEPOFF].as<u32>();
  P.steps = b[ST_STEPS].as<StepRec>(); P.incl = b[ST_INCL].as<u32>(); P.excl = b[ST_EXCL].as<u32>();
  P.scheduled = b[ST_SCHEDULED].as<uint8_t>(); P.o_node = b[ST_ONODE].as<u32>(); P.o_nt = b[ST_ONT].as<u32>(); P.o_alloc = b[ST_OALLOC].as<Res>();
  P.t_node = b[ST_TNODE].as<u32>(); P.t_alloc = b[ST_TALLOC].as<Res>();
  P.gres = h->gres;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (Jn) hipLaunchKernelGGL(k_sched_steps, dim3((Jn + 63) / 64), dim3(64), 0, h->stream, P);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  std::vector<Res> o_alloc(pl), t_alloc(tk);
  HIPCHK(h, hipMemcpyAsync(out->scheduled, b[ST_SCHEDULED].p, S, hipMemcpyDeviceToHost, h->stream));
  if (places) {
    HIPCHK(h, hipMemcpyAsync(out->node_idx, b[ST_ONODE].p, places * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out->node_ntasks, b[ST_ONT].p, places * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(o_alloc.data(), b[ST_OALLOC].p, places * sizeof(Res), hipMemcpyDeviceToHost, h->stream));
  }
  if (tasks) {
    HIPCHK(h, hipMemcpyAsync(out->task_node, b[ST_TNODE].p, tasks * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(t_alloc.data(), b[ST_TALLOC].p, tasks * sizeof(Res), hipMemcpyDeviceToHost, h->stream));
  }
  if (Nn) HIPCHK(h, hipMemcpyAsync(avail.data(), b[ST_AVAIL].p, (size_t)Nn * sizeof(Res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (u64 i = 0; i < places; ++i) {
    out->node_cpu_raw[i] = o_alloc[i].cpu; out->node_mem[i] = o_alloc[i].mem; out->node_core_lo[i] = o_alloc[i].clo;
    out->node_core_hi[i] = o_alloc[i].chi; out->node_gres[i] = o_alloc[i].gres;
    if (out->node_core_w2) out->node_core_w2[i] = o_alloc[i].c2;
    if (out->node_core_w3) out->node_core_w3[i] = o_alloc[i].c3;
  }
  for (u64 i = 0; i < tasks; ++i) {
    out->task_cpu_raw[i] = t_alloc[i].cpu; out->task_mem[i] = t_alloc[i].mem; out->task_core_lo[i] = t_alloc[i].clo;
    out->task_core_hi[i] = t_alloc[i].chi; out->task_gres[i] = t_alloc[i].gres;
    if (out->task_core_w2) out->task_core_w2[i] = t_alloc[i].c2;
    if (out->task_core_w3) out->task_core_w3[i] = t_alloc[i].c3;
  }
  for (u32 n = 0; n < Nn; ++n) {
    out->avail_cpu_raw[n] = avail[n].cpu; out->avail_mem[n] = avail[n].mem; out->avail_core_lo[n] = avail[n].clo;
    out->avail_core_hi[n] = avail[n].chi; out->avail_gres[n] = avail[n].gres;
    if (out->avail_core_w2) out->avail_core_w2[n] = avail[n].c2;
    if (out->avail_core_w3) out->avail_core_w3[n] = avail[n].c3;
  }
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (kernel_ms) *kernel_ms = ms;
  return CNS_OK;
}
