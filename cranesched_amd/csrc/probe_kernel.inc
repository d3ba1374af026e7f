// k_probe — what-if start-time probes against the FINAL state of a cycle (include/crane_gpu_probe/probe.h).
//
// A probe is a job record (k_pack_jobs + k_prep_jobs, as in a cycle) that is tested against the committed arrays of the last cycle —
// cost, front summaries, dips, node blocks — exactly as the ordered loop would test the job behind the last one it took
// (GetNodesAndTrySchedule_ + Backfill_, JobScheduler.cpp:6147-6376, and the reason of a later start, :6797-6831), and committed
// NOWHERE: the kernel stores to the probe's own result arrays and to its workgroup's own scratch, to nothing else.
//
// Q probes are Q independent problems, so the kernel is parallel over probes: persistent one-wave workgroups take probes from one
// counter (a vector atomic), one probe per workgroup at a time.  No workgroup ever waits for another one — no co-residency is needed,
// the kernel may share the GPU — and every loop is bounded by data the workgroup holds: a candidate walk consumes one slot of the
// partition per trip (<= n_p trips), the scans run over n_p slots, window_min / next_fit_wave over a map's length (<= kTlCap),
// earliest_start has its own iteration bound.
//
// Per probe, the walk of worker_job_slow (select_kernels.hip) with the memory scan of k_mem (wide_kernel.inc, giant_eval) in the
// place of the scanner waves:
//   Phase A  candidates that may start now — eval_node's necessary front filter, the slot's dip, node lists — in ascending
//            (cost, slot) order; exact test on the node block (window_min + feasible / max_tasks, window_all_total for an
//            exclusive job); top-k heap with the early break of :6294-6297 -> start now.
//   Phase B  the res_total walk (:6233-6242) from the cheapest slot again, distribute_and_alloc, earliest_start over the k
//            blocks, later_start_reason; "Resource" without a start when the partition cannot host the job at all.
// The front arrays are read from HBM only; a time map's length comes from the block header (KParams::f_len is kept by one
// commit path only).  Cost ties break on the slot (= ascending dense node index inside a partition); in a group of partitions that
// share nodes a probe sees the slots of its own partition, their own costs, and the node's one time map through slot_block.
#pragma once

namespace cns {

struct ProbeParams {
  u64 nq;              // probes that reach a walk (grouped by engine partition: records [0, nq) of KParams::jobrec)
  const u32* part;     // [nq] engine partition of record i
  u32* counter;        // [1] next record to take, zeroed before the launch
  u32 heap_stride;     // HeapEnt per resident workgroup: min(widest partition, widest node_num of the call) + 1
  u32 pad;
};

constexpr u32 kProbeLoffClamp = 0xFFFFFFFFu;   // KParams::dip_t is 32 bits of seconds after `now`: a longer time limit reaches every dip
constexpr int kProbeBlock = 64;   // one wave: the routines of the exact test are wave-wide, and the parallelism is over probes

// May the time-map entry behind a slot's dip (KParams::dip_*: packed upper bounds of one FUTURE entry below the front) host the
// minimum view?  Every saturated field counts as "fits": only a necessary condition may filter.
__device__ __forceinline__ bool probe_fits_dip(const Req& mv, u32 flags, u32 dcm, u32 dg, const GresDev& G) {
  const u32 dc = dcm >> 16, dm = dcm & 0xFFFFu;
  static_assert(kDipCpuSat == 0xFFFFu && kDipMemSat == 0xFFFFu && kDipGresSat == 15u, "the packing of KParams::dip_cm / dip_g");
  const i64 rcpus = mv.cpu >> 8;          // whole cpus of the request, rounded down (the dip's are rounded up)
  const u64 rgib = mv.mem >> 30;          // GiB, rounded down
  if (dc != kDipCpuSat && rcpus > (i64)dc) return false;
  if (dm != kDipMemSat && rgib > (u64)dm) return false;
  if (flags & kJfGres) {
    for (int g = 0; g < kMaxClasses; ++g) {
      const u32 need = (u32)((mv.gspec >> (8 * g)) & 0xFFull), have = (dg >> (4 * g)) & 15u;
      if (have != kDipGresSat && need > have) return false;
    }
    for (int a = 0; a < kMaxNames; ++a) {
      const u32 tot = (mv.gtot >> (8 * a)) & 0xFFu;
      if (!tot) continue;
      u32 have = 0;
      bool sat = false;
      for (int g = 0; g < kMaxClasses; ++g)
        if ((G.name_bytes[a] >> (8 * g)) & 0xFFull) { const u32 h = (dg >> (4 * g)) & 15u; have += h; sat = sat || h == kDipGresSat; }
      if (!sat && have < tot) return false;
    }
  }
  return true;
}

// The next candidate of the walk: the lexicographic (cost key, slot) minimum over the probe's slots [rb, rb + rn) of its partition
// that lies at or behind (lc, ln) and passes the filter of the phase (start_now: Phase A, else the res_total set).  Wave-uniform
// result; kNone: the walk is over.  The time map's length is NOT looked at here (the caller skips a full node when it is delivered).
__device__ __forceinline__ void probe_next(const KParams& P, const KParams& Pm, const JobCtx& J, u64 tyok, bool start_now, u32 qbeg, u32 rb, u32 rn,
                                           u64 lc, u32 ln, u32 lane, u64& oc, u32& op) {
  u64 bc = ~0ull;
  u32 bp = kNone;
  const u32 loff = J.L >= (i64)kProbeLoffClamp ? kProbeLoffClamp : (u32)J.L;   // an entry t seconds after now lies in the window iff t < L (:6279)
  for (u32 o = lane; o < rn; o += (u32)kProbeBlock) {
    const u32 p = rb + o, q = qbeg + p;
    const u64 ck = cost_key(P.cost[q]);
    if (ck < lc || (ck == lc && p < ln)) continue;   // delivered already
    if (!(ck < bc)) continue;                        // (a lane's slots ascend and `<` is strict: the smallest slot among equal keys)
    NodeSum ns;
    ns.cost = 0; ns.code = p; ns.len = 0; ns.type = P.slot_type[q];
    ns.fcpu = P.f_cpu[q]; ns.fmem = P.f_mem[q]; ns.fcnt = P.f_cnt[q];
    bool b, a;
    eval_node(P, J.min_view, J.flags, tyok, ns, b, a);
    if (J.flags & kJfExclusive) {   // exclusive: the node must be completely free now (necessary for :6251-6257)
      const Res tt = P.type_total[ns.type];
      a = b && ns.fcpu >= clamp_cpu(tt.cpu) && ns.fmem >= mem_mib_ceil(tt.mem) && ns.fcnt == class_counts(tt.gres, Pm.gres);
    }
    bool ok = start_now ? a : b;
    if (ok && start_now) {          // a window that reaches the slot's dip must fit the dip too
      const u32 dt = P.dip_t[q];
      if (dt < loff && !probe_fits_dip(J.min_view, J.flags, P.dip_cm[q], P.dip_g[q], Pm.gres)) ok = false;
    }
    if (ok && (J.flags & (kJfIncl | kJfExcl))) {   // included / excluded node lists (:6202-6220)
      const u32 n = P.slot_node[q];
      if ((J.flags & kJfIncl) && !in_list(P.incl_nodes, J.incl_b, J.incl_e, n)) ok = false;
      if ((J.flags & kJfExcl) && in_list(P.excl_nodes, J.excl_b, J.excl_e, n)) ok = false;
    }
    if (ok) { bc = ck; bp = p; }
  }
  wave_argmin(bc, bp);
  oc = uni64(bc); op = uni32(bp);
}

// The placement records of a decided probe, ascending node index (commit_selection's record part), and its start / reason.
__device__ __forceinline__ void probe_emit(const KParams& P, const JobCtx& J, const HeapEnt* H, i64 start, int reason, u32 lane) {
  for (u32 i = lane; i < J.k; i += (u32)kProbeBlock) {
    const HeapEnt me = H[i];
    u32 rank = 0;
    for (u32 m = 0; m < J.k; ++m) rank += H[m].node < me.node ? 1u : 0u;
    const u64 o = J.poff + rank;
    P.o_node[o] = me.node;
    P.o_ntasks[o] = (u32)me.ntasks;
    P.o_cpu[o] = me.res.cpu;
    P.o_mem[o] = me.res.mem;
    P.o_clo[o] = me.res.clo;
    P.o_chi[o] = me.res.chi;
    P.o_gres[o] = me.res.gres;
    if (P.o_c2) { P.o_c2[o] = me.res.c2; P.o_c3[o] = me.res.c3; }
  }
  if (lane == 0) { P.o_start[J.orig] = start; P.o_reason[J.orig] = (uint8_t)reason; }
}

// One probe: record `ji` of the probe table against engine partition `part`.  H: this workgroup's heap scratch.
__device__ __noinline__ void probe_one(const KParams* Pg, u64 ji, u32 part, HeapEnt* H) {
  const KParams& Pm = *Pg;                  // the block in HBM: for the out-of-line routines and the GRES tables
  const auto& P = kparams_scalar(Pg);
  const u32 lane = threadIdx.x & 63u;
  const u32 raw = fetch_job(P, ji);
  const JobCtx J = make_job(P, ji, raw);
  const u64 tyok = jr64(raw, kJdTyok);
  const u32 orig = J.orig;
  const u32 qbeg = uni32(P.part_off[part]);
  const u32 nn = uni32(P.part_off[part + 1]) - qbeg;
  const bool resv_part = part >= P.num_real_parts;
  if (resv_part) {   // a reservation's scheduler exists only while the reservation is active (JobScheduler.cpp:6643,6754-6759)
    const i64 rs = P.resv_se[2 * (part - P.num_real_parts)], re = P.resv_se[2 * (part - P.num_real_parts) + 1];
    if (!(rs <= P.now && P.now < re)) {
      if (lane == 0) { P.o_start[orig] = 0; P.o_reason[orig] = CNS_REASON_RESERVATION_NOT_FOUND; }
      return;
    }
  }
  // a probe into a group of partitions that share nodes sees the slots of its own partition only
  u32 rb = 0, rn = nn;
  if (P.slot_tag && P.tag_off) {
    const u32 tb = uni32(P.tag_base[part]) + ((J.flags >> 8) & 0xFFu);
    rb = uni32(P.tag_off[tb]); rn = uni32(P.tag_off[tb + 1]) - rb;
  }
  const bool excl_job = (J.flags & kJfExclusive) != 0;
  // ntasks_on_node_total per node type (JobScheduler.cpp:6222): lane t evaluates type t
  int tt_lane = 0;
  if (lane < P.num_types) {
    const Res ttot = P.type_total[lane];
    if (J.general) tt_lane = max_tasks(J.min_view, J.tcpu, J.tmem, J.tmin, J.tmax, ttot, Pm.gres);
    else { Res tmp; tt_lane = feasible(J.min_view, ttot, tmp, Pm.gres) ? (int)J.tmin : 0; }
  }

  // ---- Phase A: start now (GetNodesAndTrySchedule_, JobScheduler.cpp:6188-6333) -------------
  {
    int hsize = 0, hsum = 0;  // topk_nodes_avail.size(), topk_ntasks_sum_avail
    u64 lc = 0;
    u32 ln = 0;
    for (;;) {
      u64 wc;
      u32 wp;
      probe_next(P, Pm, J, tyok, true, qbeg, rb, rn, lc, ln, lane, wc, wp);
      if (wp == kNone) break;
      lc = wc; ln = wp + 1u;
      const u32 q = qbeg + wp;
      NodeHdr* const hd = hdr_of(P, q);
      const u32 len = uni32(hd->len);
      if (len >= P.max_jobs_per_node) continue;   // :6194, on the map as the cycle left it
      const TlMap T = tl_of(P, hd);
      const u32 n = uni32(hd->node);
      bool ok = false;
      Res m = res_zero();
      int ta = 0;
      if (!excl_job) {
        const Res a0 = uni_res(hd->avail0);
        Res f;
        if (feasible(J.min_view, a0, f, Pm.gres)) {             // :6274
          m = window_min(T, len, a0, J.E, lane);                // :6278-6283
          if (J.general) ta = max_tasks(J.min_view, J.tcpu, J.tmem, J.tmin, J.tmax, m, Pm.gres);  // :6285
          else ta = feasible(J.min_view, m, f, Pm.gres) ? (int)J.tmin : 0;
          ok = ta > 0;
        }
      } else {
        m = uni_res(hd->total);
        ok = window_all_total(T, len, m, J.E, lane);            // :6250-6260
        ta = __shfl(tt_lane, (int)uni32(hd->type));
      }
      if (!ok) continue;
      HeapEnt x;
      x.ntasks = ta; x.p = wp; x.node = n; x.pad = 0;
      x.cost = P.cost[q];
      x.res = m;
      int nsum = hsum + ta, nsize = hsize + 1;
      if (lane == 0) {
        H[hsize] = x;
        pq_push(H, nsize);                                                // :6288-6289
        if (nsize > (int)J.k) { nsum -= H[0].ntasks; pq_pop(H, nsize); }  // :6290-6293
      }
      nsum = __shfl(nsum, 0);
      if (nsize > (int)J.k) --nsize;
      hsum = nsum; hsize = nsize;
      __threadfence_block();
      if (hsize == (int)J.k && (u32)hsum >= J.ntasks) {                   // :6294-6297
        if (!distribute_and_alloc(Pm, J, H, lane)) { if (lane == 0) set_fault(P, 2, orig, n, 2); }
        probe_emit(P, J, H, P.now, CNS_REASON_NONE, lane);                // start_time = now (:6326)
        return;
      }
    }
  }

  // ---- Phase B: top-k nodes by total capacity, then the earliest start (:6233-6242, :6335-6368, Backfill_ :6371-6376) -----
  int nsel = 0, tsum = 0;
  bool complete = false;
  {
    u64 lc = 0;
    u32 ln = 0;
    for (;;) {
      u64 cc;
      u32 cp;
      probe_next(P, Pm, J, tyok, false, qbeg, rb, rn, lc, ln, lane, cc, cp);
      if (cp == kNone) break;
      lc = cc; ln = cp + 1u;
      const u32 q = qbeg + cp;
      NodeHdr* const hd = hdr_of(P, q);
      if (uni32(hd->len) >= P.max_jobs_per_node) continue;   // :6194
      HeapEnt x;
      x.p = cp; x.node = uni32(hd->node); x.pad = 0;
      x.cost = P.cost[q];
      x.res = res_zero();
      if (!J.general) {
        x.ntasks = 1;
        if (lane == 0) H[nsel] = x;
        ++nsel;
        if (nsel == (int)J.k) { complete = true; break; }
      } else {
        const int tt = __shfl(tt_lane, (int)uni32(hd->type));
        x.ntasks = tt;
        int nsum = tsum + tt, nsize = nsel + 1;  // the push condition (:6233-6234) held, else the walk had stopped
        if (lane == 0) {
          H[nsel] = x;
          pq_push(H, nsize);
          if (nsize > (int)J.k) { nsum -= H[0].ntasks; pq_pop(H, nsize); }
        }
        nsum = __shfl(nsum, 0);
        if (nsize > (int)J.k) --nsize;
        tsum = nsum; nsel = nsize;
        __threadfence_block();
        if (nsel == (int)J.k && (u32)tsum >= J.ntasks) { complete = true; break; }
      }
    }
  }
  if (complete) {
    __threadfence_block();
    for (u32 i = lane; i < J.k; i += (u32)kProbeBlock) {
      HeapEnt x = H[i];
      x.res = hdr_of(P, qbeg + x.p)->total;
      H[i] = x;
    }
    __threadfence_block();
    if (!distribute_and_alloc(Pm, J, H, lane)) { if (lane == 0) set_fault(P, 3, orig, 0, 1); }
    const i64 t = earliest_start(P, J.k, [&](u32 i, i64 t0) {
      NodeHdr* hd = hdr_of(P, qbeg + H[i].p);
      return next_fit_wave(tl_of(P, hd), hd->len, &H[i].res, J.L, t0);
    });
    if (t != kInf) {
      int reason = CNS_REASON_NONE;
      if (t != P.now) {
        bool notle = false, reserved = false;
        for (u32 i = lane; i < J.k; i += (u32)kProbeBlock) {
          const HeapEnt x = H[i];
          const u32 qx = qbeg + x.p;
          if (!res_le(x.res, hdr_of(P, qx)->avail0)) notle = true;
          if (P.first_resv[qx] < P.now + J.L) reserved = true;
        }
        reason = later_start_reason(!resv_part && __any(reserved), __any(notle));
      }
      probe_emit(P, J, H, t, reason, lane);
      return;
    }
  }
  if (lane == 0) { P.o_start[orig] = 0; P.o_reason[orig] = CNS_REASON_RESOURCE; }  // :6768
}

__global__ __launch_bounds__(kProbeBlock) void k_probe(const KParams* __restrict__ Pg, const ProbeParams Q) {
  HeapEnt* const H = Pg->heap + (u64)blockIdx.x * Q.heap_stride;
  for (;;) {
    u32 i = 0;
    if (threadIdx.x == 0) i = atomicAdd(Q.counter, 1u);
    i = uni32(i);
    if ((u64)i >= Q.nq) return;
    probe_one(Pg, (u64)i, uni32(Q.part[i]), H);
  }
}

}  // namespace cns
