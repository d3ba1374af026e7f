// k_pipe<NPL> — the selection kernel with the exact test and the commit taken OFF the sequential chain.
// Included from select_kernels.hip (inside namespace cns); shares every device routine with k_select.
//
// Why: inside a partition job j+1 must see job j's commit (SURVEY.md §7), and in k_select one worker wave carries
// the whole chain  scan -> exact test -> commit -> merge  (12.9 k cycles per job on C4, profiles/r01_cycle_breakdown).
// But job j+1's SELECTION only needs to know WHICH node job j took and what that does to the node's cost and front
// summary — and that is arithmetic on the request (JobScheduler.h:47-53: cost += secs * cpu_alloc / cpu_total;
// front -= allocation) as soon as one assumes that the first node in cost order that passes the scanners' front
// filter also passes the exact test (:6274-6285).  On C4 that assumption fails 27 times in 10^6 jobs.  So:
//
//   waves 4-11  SCANNERS  the register tile of k_select (512 lanes x NPL nodes).  They run the queue ON THEIR OWN: scan
//                         (filters + argmin, top-k lists for multi-node jobs), exchange the per-wave results through
//                         LDS, decide — every wave computes the same decision: start now on A / backfill on T / fail —
//                         and the wave that owns a selected node applies the PREDICTED effect to its registers.  The
//                         sequential chain of a partition is exactly this loop.
//   wave 0      SUPERVISOR follows a few jobs behind: re-derives the decision from the same exchange records, posts
//                         the task (with the dependency on the previous task of the node); runs the serial jobs, the
//                         flushes and the end.
//   waves 1-3   TESTERS   take the tasks in order: wait for the last task on the same node (dep), ONE coalesced
//                         block read, window-min + GetFeasibleResourceInNode (start now) or allocation against
//                         res_total + earliest start (backfill), verdict; then — once every OLDER task has a verdict
//                         and none of them failed — commit (time map, cost, front arrays, placement records).
//                         A verdict that contradicts the prediction (candidate rejected, node map full, no start in
//                         the window) FLUSHES: younger tasks abort before writing anything, the scanners reload
//                         their tile from the HBM arrays (which only ever hold committed state) and the job is
//                         redone by the sequential protocol.
//
// Everything that is not "ntasks == node_num <= 8, tpn_min == 1, shared nodes, class-determined GRES split" runs in
// SERIAL mode: the pipeline drains, the tile is reloaded, and the job goes through k_select's one-candidate-per-round
// protocol (worker_job_slow) with the selector as the worker and every other wave following the barriers.
//
// Exactness: the tile only feeds NECESSARY conditions and the cost order.  Predicted values are exact for the cost
// and the front cpu, conservative (never below the truth) for memory in GiB and saturated GRES counts, and the
// time-map length keeps its last exact value (a node whose map filled up meanwhile is caught by its tester).
// Synchronisation is LDS-only (sequence numbers + s_sleep polling between co-resident waves of ONE workgroup); every
// wait for progress is bounded and raises a device fault instead of hanging.

#ifndef CNS_PIPE_BLOCK
#define CNS_PIPE_BLOCK 768
#endif
#ifndef CNS_PIPE_TESTERS
#define CNS_PIPE_TESTERS 3
#endif
// 768 threads = 12 waves = 3 per SIMD = 168 VGPRs per lane.  (The first version ran 1024 threads / 128 VGPRs: the scan
// loop spilled ~70 values to scratch and took 22 k cycles per job instead of ~4 k; profiles/r02_pipe_1024_spills.txt.)
constexpr int kPBlock = CNS_PIPE_BLOCK;
constexpr int kPWaves = kPBlock / 64;
constexpr int kPTesters = CNS_PIPE_TESTERS;  // waves 1..kPTesters
constexpr int kPScanW0 = 1 + kPTesters;   // first scanner wave
constexpr int kPScanWaves = kPWaves - kPScanW0;
constexpr u32 kPScan = kPScanWaves * 64;  // scanner lanes = nodes per tile row
#if CNS_PIPE_BLOCK == 768 && CNS_PIPE_TESTERS == 3
#define CNS_PNPL_LIST(X) X(1) X(4) X(8) X(16)
constexpr int kPNplMax = 16;
#elif CNS_PIPE_BLOCK == 768 && CNS_PIPE_TESTERS == 4
#define CNS_PNPL_LIST(X) X(1) X(4) X(19)
constexpr int kPNplMax = 19;
#elif CNS_PIPE_BLOCK == 512 && CNS_PIPE_TESTERS == 3
#define CNS_PNPL_LIST(X) X(1) X(4) X(16) X(32)
constexpr int kPNplMax = 32;
#elif CNS_PIPE_BLOCK == 512 && CNS_PIPE_TESTERS == 2
#define CNS_PNPL_LIST(X) X(1) X(4) X(26)
constexpr int kPNplMax = 26;
#elif CNS_PIPE_BLOCK == 1024 && CNS_PIPE_TESTERS == 2
#define CNS_PNPL_LIST(X) X(1) X(4) X(10)
constexpr int kPNplMax = 10;
#elif CNS_PIPE_BLOCK == 1024 && CNS_PIPE_TESTERS == 3
#define CNS_PNPL_LIST(X) X(1) X(4) X(11)
constexpr int kPNplMax = 11;
#elif CNS_PIPE_BLOCK == 1024 && CNS_PIPE_TESTERS == 4
#define CNS_PNPL_LIST(X) X(1) X(4) X(12)
constexpr int kPNplMax = 12;
#elif CNS_PIPE_BLOCK == 1024
#define CNS_PNPL_LIST(X) X(1) X(4) X(13)
constexpr int kPNplMax = 13;
#else
#define CNS_PNPL_LIST(X) X(1) X(4) X(16) X(26)
constexpr int kPNplMax = 26;
#endif
constexpr u32 kPRing = 32;                // task slots (power of two)
constexpr int kPMaxK = 8;                 // node_num handled by the pipeline
static_assert(kPWaves <= kRed, "per-wave exchange slots");

enum PipeTaskState : u32 { kTsFree = 0, kTsPosted = 1, kTsPass = 2, kTsFail = 3, kTsAborted = 4, kTsCommitted = 5 };
enum PipeCmd : u32 { kPcSerial = 3, kPcReload = 4, kPcExit = 5, kPcResume = 6 };
enum PipeKind : u32 { kPkStart = 0, kPkBackfill = 1, kPkFail = 2 };
constexpr u32 kPXRing = 8;                // exchanges the supervisor may lag behind the scanners (power of two)

struct PipeTask {     // one job, selector -> tester
  u32 id;             // task id (1-based, monotone); slot = id % kPRing
  u32 state;          // PipeTaskState
  u32 ji;             // index in the grouped job table
  u32 kind_k;         // PipeKind | node_num << 8
  u32 code[kPMaxK];   // slot codes in cost order
  u32 dep[kPMaxK];    // last older task on that node (0: none)
  u64 cost0[kPMaxK];  // fp64 cost bit pattern of the node before this job
};
struct PipeRes {      // what one scanner wave contributes to the decision of a node_num == 1 job
  u64 ac;             // A: cheapest node of the wave that may start the job now (cost key, slot code, node type)
  u32 ap, aty;
  u64 tc;             // T: cheapest node of the wave whose res_total fits
  u32 tp, tty;
};

__device__ __forceinline__ u32 pslot(u32 code) { return slot_of_code_t<kPScan>(code); }
__device__ __forceinline__ u32 powner(u32 code) { return (u32)kPScanW0 + ((code & 1023u) >> 6); }
// Every word the waves poll lives in LDS: go through the LDS address space explicitly (ds_read / ds_write); a generic
// pointer handed to an out-of-line routine would be a FLAT access (400 of them per job in the first version).
typedef __attribute__((address_space(3))) u32 lds_u32;
__device__ __forceinline__ u32 vld(const u32* p) { return *(const volatile lds_u32*)p; }
__device__ __forceinline__ void vst(u32* p, u32 v) { *(volatile lds_u32*)p = v; }
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void nap() { __builtin_amdgcn_s_sleep(4); }
#ifndef CNS_PIPE_IDLE_NAP
#define CNS_PIPE_IDLE_NAP 4
#endif
__device__ __forceinline__ void nap_idle() { __builtin_amdgcn_s_sleep(CNS_PIPE_IDLE_NAP); }   // nothing to do at all (idle tester / supervisor)   // polling waves must not eat the issue slots of working ones
constexpr u32 kPSpinLimit = 1u << 24;  // x ~130 cycles: ~1 s; a wait for PROGRESS longer than that is a protocol bug

struct PipeShared {
  PipeTask* task;
  u32* flush_job;   // lowest job index whose task contradicted its prediction (kNone: none)
  u32* abort;       // != 0: a device fault was raised; every wave leaves
  u32* posted;      // tasks posted so far
  Res* tres;        // [kPTesters][kPMaxK] allocations of a multi-node task
  u32* tnode;       // [kPTesters][kPMaxK] dense node indices of a multi-node task
};

__device__ __forceinline__ void pipe_fault(const KParams& P, const PipeShared& sh, u32 code, u32 a, u32 b, u32 c) {
  if ((threadIdx.x & 63u) == 0) { set_fault(P, code, a, b, c); vst(sh.abort, 1u); }
}

// The older task `dep` no longer owns its nodes (committed, or it never will commit).
__device__ __forceinline__ bool pipe_wait_dep(const KParams& P, const PipeShared& sh, u32 dep) {
  if (dep == 0) return true;
  const PipeTask* s = &sh.task[dep & (kPRing - 1)];
  for (u32 spin = 0;; ++spin) {
    const u32 id = vld(&s->id), st = vld(&s->state);
    if (id != dep || st >= kTsFail) return true;   // slot recycled (=> final) or final
    if (vld(sh.abort)) return false;
    if (spin > kPSpinLimit) { pipe_fault(P, sh, 20, dep, id, st); return false; }
    nap();
  }
}

// Every task older than `my` has a verdict.  Returns false on abort / fault.
__device__ __forceinline__ bool pipe_wait_verdicts(const KParams& P, const PipeShared& sh, u32 my) {
  const u32 lane = threadIdx.x & 63u;
  for (u32 spin = 0;; ++spin) {
    bool ok = true;
    if (lane + 1 < kPRing && my > lane + 1) {
      const u32 e = my - 1 - lane;
      const PipeTask* s = &sh.task[e & (kPRing - 1)];
      const u32 id = vld(&s->id), st = vld(&s->state);
      ok = id != e || st >= kTsPass;
    }
    if (!__any(!ok)) return true;
    if (vld(sh.abort)) return false;
    if (spin > kPSpinLimit) { pipe_fault(P, sh, 21, my, 0, 0); return false; }
    nap();
  }
}

// Commit of one node of a task from the tester's registers: NodeState::UpdateResourceInNode (JobScheduler.h:340-459),
// MinCpuTimeRatioFirst::UpdateCost (h:47-53), the HBM arrays the scanners reload from, and the placement record.
template <bool kW = true>
// (Pmem: the parameter block for the out-of-line routine of maps longer than 64 entries, G: the GRES layout — both P's own;
// abort: the LDS word that tells every wave of the workgroup to leave)
__device__ __forceinline__ void pipe_commit_node(const KParams& P, const KParams& Pmem, const GresDev& G, u32* abort, NodeHdr* hd, const NodeHdr& h,
                                                 const TlEntry& e, u32 q, u64 cost0, const Res& alloc, i64 start, i64 L,
                                                 u32 orig, u64 rec, u32 lane) {
  const i64 end = start + L;   // job->end_time = start_time + time_limit, JobScheduler.cpp:6772
  Res f = rl_res(e.r, 0);      // entry 0 = the entry at `now`
  if (h.len <= kTlChunk) tl_commit_regs(P, hd, tl_of<kW>(P, hd), e, h.len, start, end, alloc, lane, orig);
  else tl_commit(Pmem, hd, start, end, alloc, lane, orig);
  const double ratio = ((double)alloc.cpu / 256.0) / ((double)h.total.cpu / 256.0);
  const double ncost = __longlong_as_double((long long)cost0) + (double)(end - start) * ratio;
  if (lane == 0) {
    if (cost_key(*as_global(P.cost + q)) != cost0) {   // the selector's cost chain broke
#ifdef CNS_DEBUG_FLUSH_LOG
      u64* const dbg = P.prof + (size_t)P.num_parts * 48 + 2040;
      dbg[0] = cost0; dbg[1] = cost_key(P.cost[q]); dbg[2] = ((u64)orig << 32) | h.node; dbg[3] = (u64)start; dbg[4] = (u64)alloc.cpu; dbg[5] = (u64)h.total.cpu; dbg[6] = (u64)L;
#endif
      set_fault(P, 22, orig, h.node, 0); vst(abort, 1u);
    }
    P.cost[q] = ncost;
    if (start == P.now) {
      res_sub(f, alloc);
      P.f_cpu[q] = clamp_cpu(f.cpu); P.f_mem[q] = mem_mib_ceil(f.mem); P.f_cnt[q] = class_counts(f.gres, G);
    }
    P.o_node[rec] = h.node; P.o_ntasks[rec] = 1;
    P.o_cpu[rec] = alloc.cpu; P.o_mem[rec] = alloc.mem; P.o_clo[rec] = alloc.clo; P.o_chi[rec] = alloc.chi;
    if (kW && P.o_c2) { P.o_c2[rec] = alloc.c2; P.o_c3[rec] = alloc.c3; }
    P.o_gres[rec] = alloc.gres;
  }
}

// One task on a tester wave.  All 64 lanes execute it; every branch is wave-uniform.
template <u32 kS, bool kW>
__device__ __noinline__ void pipe_tester_task(const KParams* Pg, const PipeShared sh, u32 my, u32 tw, u32 qbeg, bool resv_part, u64 jbase) {
  const auto& P = kparams_scalar(Pg);   // (the block's copy in HBM, through scalar loads: select_kernels.hip)
  const GresDev& G = Pg->gres;
  const u32 lane = threadIdx.x & 63u;
  PipeTask* const T = &sh.task[my & (kPRing - 1)];
  const u32 ji = vld(&T->ji), kind_k = vld(&T->kind_k);
  const u32 kind = kind_k & 0xFFu, k = kind_k >> 8;
  Res* const ares = sh.tres + tw * kPMaxK;
  u32* const anode = sh.tnode + tw * kPMaxK;
  // an older task already contradicted its prediction: this selection was made on a wrong premise
  if (vld(sh.flush_job) <= ji) { if (lane == 0) { lds_fence(); vst(&T->state, kTsAborted); } return; }
  const u32 raw = fetch_job(P, (u64)ji + jbase);
  const FastJob F = make_fast_job(P, raw);
  const u32 maxlen = P.max_jobs_per_node;
  bool ok = true;
  i64 st = P.now;
  int reason = CNS_REASON_NONE;
  NodeHdr* hd = nullptr; NodeHdr h; TlEntry e;
  Res alloc = res_zero();
  u32 q = 0;
  h.len = 0;

  if (k == 1) {
    const u32 code = vld(&T->code[0]);
    q = qbeg + slot_of_code_t<kS>(code);
    PROF_T(d0);
    if (!pipe_wait_dep(P, sh, vld(&T->dep[0]))) return;
    PROF_T(d1);
    if (tw == 0) PROF_ADD(13, d0, d1);  // tester 0: waiting for the previous task on the node
    load_block<kW>(P, q, lane, hd, h, e);
    ok = h.len < maxlen;                                            // :6194 on the CURRENT map (the tile's length may be stale)
    if (ok && kind == kPkStart) {
      ok = fits_now(F.mv, block_window_min<kW>(P, hd, h, e, F.E, lane), h.avail0, alloc, G);
    } else if (ok) {
      // backfill on the first node in cost order whose res_total fits (:6335-6368, Backfill_ :6371-6376)
      if (!feasible(F.mv, h.total, alloc, G)) { pipe_fault(P, sh, 3, F.orig, h.node, 0); return; }
      alloc = uni_res(alloc);
      st = block_next_fit<kW>(P, hd, h, e, alloc, F.L, P.now, lane);
      ok = st != kInf && st - P.now <= P.max_window;                // kAlgoMaxTimeWindow, JobScheduler.h:815
      if (ok && st != P.now) reason = later_start_reason(!resv_part && P.first_resv[q] < P.now + F.L, !res_le(alloc, h.avail0));
    }
  } else {
    // node_num 2..8, ntasks == node_num: the nodes one after the other (the task is off the sequential chain)
    const Req& v1 = F.mv;  // tpn_min == 1: the minimum view is the one-task view
    bool notle = false, reserved = false;
    for (u32 i = 0; i < k && ok; ++i) {
      const u32 qi = qbeg + slot_of_code_t<kS>(vld(&T->code[i]));
      if (!pipe_wait_dep(P, sh, vld(&T->dep[i]))) return;
      load_block<kW>(P, qi, lane, hd, h, e);
      if (h.len >= maxlen) { ok = false; break; }
      Res a = res_zero();
      if (kind == kPkStart) {
        ok = fits_now(v1, block_window_min<kW>(P, hd, h, e, F.E, lane), h.avail0, a, G);
      } else {
        if (!feasible(v1, h.total, a, G)) { pipe_fault(P, sh, 3, F.orig, h.node, 2); return; }   // :6354-6356
        notle = notle || !res_le(a, h.avail0);
        reserved = reserved || (!resv_part && P.first_resv[qi] < P.now + F.L);
      }
      if (lane == 0) { ares[i] = a; anode[i] = h.node; }
    }
    lds_fence();
    if (ok && kind == kPkBackfill) {
      st = earliest_start(P, k, [&](u32 i, i64 t) {
        load_block<kW>(P, qbeg + slot_of_code_t<kS>(vld(&T->code[i])), lane, hd, h, e);
        return block_next_fit<kW>(P, hd, h, e, ares[i], F.L, t, lane);
      });
      ok = st != kInf;
      if (ok && st != P.now) reason = later_start_reason(reserved, notle);
    }
  }

  // ---- verdict ------------------------------------------------------------------------------------------
  if (!ok) {
    if (lane == 0) { atomicMin(sh.flush_job, ji); lds_fence(); vst(&T->state, kTsFail); }
    return;
  }
  if (lane == 0) { lds_fence(); vst(&T->state, kTsPass); }
  PROF_T(v0);
  if (!pipe_wait_verdicts(P, sh, my)) return;
  PROF_T(v1);
  if (tw == 0) { PROF_ADD(14, v0, v1); PROF_CNT(15); }  // tester 0: waiting for the older verdicts
  if (vld(sh.flush_job) <= ji) { if (lane == 0) { lds_fence(); vst(&T->state, kTsAborted); } return; }

  // ---- commit (every older task has a passing verdict: the selections up to here were right) ------------------
  if (k == 1) {
    pipe_commit_node<kW>(P, *Pg, G, sh.abort, hd, h, e, q, ((u64)vld((u32*)&T->cost0[0] + 1) << 32) | vld((u32*)&T->cost0[0]), alloc, st, F.L,
                     F.orig, F.poff, lane);
  } else {
    for (u32 i = 0; i < k; ++i) {
      const u32 qi = qbeg + slot_of_code_t<kS>(vld(&T->code[i]));
      load_block<kW>(P, qi, lane, hd, h, e);
      u32 rank = 0;  // placement records are listed by ascending node index
      for (u32 m = 0; m < k; ++m) rank += anode[m] < h.node ? 1u : 0u;
      const u64 c0 = ((u64)vld((u32*)&T->cost0[i] + 1) << 32) | vld((u32*)&T->cost0[i]);
      pipe_commit_node<kW>(P, *Pg, G, sh.abort, hd, h, e, qi, c0, uni_res(narrow<kW>(ares[i])), st, F.L, F.orig, F.poff + rank, lane);
    }
  }
  if (lane == 0) { P.o_start[F.orig] = st; P.o_reason[F.orig] = (uint8_t)reason; }
  drain_stores();   // later tasks on these nodes, and a tile reload, read what was just written
  if (lane == 0) { lds_fence(); vst(&T->state, kTsCommitted); }
}

template <int NPL>
__global__ __launch_bounds__(kPBlock) void k_pipe(const KParams P, const KParams* __restrict__ Pg) {
  const KParams& PG = *Pg;
  const u32 part = P.part_map ? uni32(P.part_map[blockIdx.x]) : blockIdx.x;
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = uni32(tid >> 6);
  // (flat loads are sources of divergence for the compiler: make what steers the control flow uniform)
  const u32 qbeg = uni32(P.part_off[part]);
  const u32 nn = uni32(P.part_off[part + 1]) - qbeg;
  const u64 jbeg = uni64(P.pj_off[part]), jend = uni64(P.pj_off[part + 1]);
  if (jbeg >= jend) return;
  const bool resv_part = part >= P.num_real_parts;
  if (resv_part) {  // a reservation's scheduler exists only while the reservation is active (JobScheduler.cpp:6643,6754-6759)
    const i64 rs = P.resv_se[2 * (part - P.num_real_parts)], re = P.resv_se[2 * (part - P.num_real_parts) + 1];
    if (!(rs <= P.now && P.now < re)) {
      for (u64 x = jbeg + tid; x < jend; x += kPBlock) {
        const u32 orig = P.jobrec[x * kJobRecDwords + kJrOrig];
        P.o_start[orig] = 0;
        P.o_reason[orig] = CNS_REASON_RESERVATION_NOT_FOUND;
      }
      return;
    }
  }
  const u32 njobs = (u32)(jend - jbeg);

  // ---- LDS ------------------------------------------------------------------------------------------------
  // autonomous mode: what the scanner waves exchange per job (a ring, because the supervisor reads it a few jobs later)
  __shared__ PipeRes s_res[kPXRing][kPScanWaves];   // node_num == 1: per-wave A / T argmins
  __shared__ u64 s_xlc[kPXRing][kPScanWaves * kPMaxK];  // node_num 2..8: per-wave sorted candidate lists
  __shared__ u32 s_xlp[kPXRing][kPScanWaves * kPMaxK];
  __shared__ u32 s_xlty[kPXRing][kPScanWaves * kPMaxK];
  __shared__ u32 s_xhalt[kPXRing];                  // the leader saw the supervisor's halt request before this exchange
  __shared__ u32 s_arrive;                          // scanner waves arrived at exchanges (kPScanWaves per exchange)
  __shared__ u32 s_sup_nex;                         // exchanges the supervisor has consumed
  __shared__ u32 s_halt;                            // supervisor -> scanners: stop before the next job
  __shared__ u32 s_scan_pos, s_scan_stops;          // scanners stopped in front of job pos (number of stops so far)
  __shared__ PipeTask s_task[kPRing];
  __shared__ u32 s_last[kPScan * NPL];              // last task posted on a slot (dependency of the next one)
  __shared__ u32 s_cmd[4];                          // kind, job, -, -
  __shared__ u32 s_cmd_seq;
  __shared__ u32 s_done[kRed];                      // per scanner wave: last command finished
  __shared__ u32 s_posted, s_claim, s_flush_job, s_abort;
  __shared__ Res s_tres[kPTesters * kPMaxK];
  __shared__ u32 s_tnode[kPTesters * kPMaxK];
  __shared__ i64 s_tytot[CNS_MAX_NODE_TYPES_DEV];   // res_total.cpu per node type (the cost ratio's denominator)
  // serial mode: the exchange of k_select's sequential protocol
  __shared__ u64 s_wc[2][kRed];
  __shared__ u32 s_wp[2][kRed];
  __shared__ u64 s_tc[kRed];
  __shared__ u32 s_tp[kRed];
  __shared__ int s_flag;
  __shared__ int s_nupd;
  __shared__ UpdRec s_upd[kMaxUpd];
  __shared__ HeapEnt s_heap[kLdsHeap];
  __shared__ JobCtx s_job;
  __shared__ int s_ty_cpu[CNS_MAX_NODE_TYPES_DEV];
  __shared__ u32 s_ty_m16[CNS_MAX_NODE_TYPES_DEV];
  __shared__ u32 s_ty_gn[CNS_MAX_NODE_TYPES_DEV];
  __shared__ u32 s_nme[kMaxNames], s_nmo[kMaxNames];

  // ---- one-time initialisation (all waves), then one barrier ---------------------------------------------------
  for (u32 x = tid; x < kPScan * NPL; x += kPBlock) s_last[x] = 0;
  if (tid < kPRing) { s_task[tid].id = 0; s_task[tid].state = kTsFree; }
  if (tid < (u32)kRed) {
    s_wc[0][tid] = ~0ull; s_wc[1][tid] = ~0ull; s_wp[0][tid] = kNone; s_wp[1][tid] = kNone;
    s_tc[tid] = ~0ull; s_tp[tid] = kNone; s_done[tid] = 0;
  }
  if (tid < kPXRing) s_xhalt[tid] = 0;
  if (tid < CNS_MAX_NODE_TYPES_DEV) {
    const Res tt = tid < P.num_types ? P.type_total[tid] : res_zero();
    s_tytot[tid] = tt.cpu;
    s_ty_cpu[tid] = clamp_cpu(tt.cpu);
    s_ty_m16[tid] = mem_gib16(mem_mib_ceil(tt.mem));
    s_ty_gn[tid] = nibbles_of(class_counts(tt.gres, P.gres));
  }
  if (tid < (u32)kMaxNames) {
    const u32 nb = nibbles_of(P.gres.name_bytes[tid] & 0x0F0F0F0F0F0F0F0Full);
    s_nme[tid] = nb & 0x0F0F0F0Fu;
    s_nmo[tid] = (nb >> 4) & 0x0F0F0F0Fu;
  }
  if (tid == 0) {
    s_cmd_seq = 0; s_posted = 0; s_claim = 0; s_flush_job = kNone; s_abort = 0; s_flag = 0; s_nupd = 0;
    s_arrive = 0; s_sup_nex = 0; s_halt = 0; s_scan_pos = 0; s_scan_stops = 0;
  }
  __syncthreads();

  PipeShared psh;
  psh.task = s_task; psh.flush_job = &s_flush_job; psh.abort = &s_abort; psh.posted = &s_posted;
  psh.tres = s_tres; psh.tnode = s_tnode;
  int par = 0;   // double-buffer parity of the serial protocol's exchange (every wave toggles it alike)

  // ---- the decision of one job from what the scanner waves exchanged: computed alike by every scanner wave (which
  // then updates its own tile rows) and, a few jobs later, by the supervisor (which posts the task) ------------------
  // node_num == 1: start now on the A argmin, else backfill on the T argmin, else fail.  All outputs wave-uniform.
  auto decide_one = [&](u32 xs, u32& kind, u32& code, u64& cst, u32& ty) {
    const u32 l = lane & (kRed - 1);
    const bool valid = l < (u32)kPScanWaves;
    const PipeRes* R = &s_res[xs][valid ? l : 0];
    u64 wc = valid ? R->ac : ~0ull;
    u32 wcode = valid ? R->ap : kNone;
    reduce16(wc, wcode);
    wcode = uni32(wcode);
    if (wcode != kNone) { kind = kPkStart; code = wcode; cst = uni64(wc); ty = s_res[xs][powner(wcode) - (u32)kPScanW0].aty; return; }
    u64 tc = valid ? R->tc : ~0ull;   // nothing can start it now: the res_total argmins
    u32 tcode = valid ? R->tp : kNone;
    reduce16(tc, tcode);
    tcode = uni32(tcode);
    if (tcode != kNone) { kind = kPkBackfill; code = tcode; cst = uni64(tc); ty = s_res[xs][powner(tcode) - (u32)kPScanW0].tty; }
    else { kind = kPkFail; code = kNone; cst = ~0ull; ty = 0; }
  };
  // node_num 2..8: k-way merge of the per-wave sorted lists; lane i < n leaves with node i of the selection
  auto merge_lists = [&](u32 xs, u32 k, u64& mycost, u32& mycode, u32& myty) -> u32 {
    u32 idx = 0, n = 0;
    const u32 l = lane & (kRed - 1);
    const bool valid = l < (u32)kPScanWaves;
    u64 hc = valid ? s_xlc[xs][l * kPMaxK] : ~0ull;
    u32 hp = valid ? s_xlp[xs][l * kPMaxK] : kNone;
    u32 hty = valid ? s_xlty[xs][l * kPMaxK] : 0;
    mycost = ~0ull; mycode = kNone; myty = 0;
    for (u32 i = 0; i < k; ++i) {
      u64 c = hc;
      u32 pc = hp;
      reduce16(c, pc);
      pc = uni32(pc);
      if (pc == kNone) break;
      const u32 src = powner(pc) - (u32)kPScanW0;
      const u32 ty = rl32(hty, src);
      if (lane == i) { mycost = uni64(c); mycode = pc; myty = ty; }
      ++n;
      if (valid && l == src) {  // the winning wave's list advances (in every 16-lane row alike)
        ++idx;
        hc = idx < k ? s_xlc[xs][l * kPMaxK + idx] : ~0ull;
        hp = idx < k ? s_xlp[xs][l * kPMaxK + idx] : kNone;
        hty = idx < k ? s_xlty[xs][l * kPMaxK + idx] : 0;
      }
    }
    return n;
  };
  auto exchange_ready = [&](u32 e) -> bool { return vld(&s_arrive) >= (u32)kPScanWaves * (e + 1u); };

  // Follows one SERIAL job without taking part in it (tester waves): the barrier schedule of k_select's sequential
  // protocol, driven by the same LDS words the scanners read.
  auto serial_follow = [&]() {
    wg_barrier();  // S0: everybody is in serial mode (tile reloaded)
    wg_barrier();  // B1 (round 0)
    u64 c = s_wc[par][lane & (kRed - 1)];
    u32 acode = s_wp[par][lane & (kRed - 1)];
    u64 c2 = s_tc[lane & (kRed - 1)];
    u32 tcode = s_tp[lane & (kRed - 1)];
    reduce16(c, acode);
    reduce16(c2, tcode);
    par ^= 1;
    acode = uni32(acode); tcode = uni32(tcode);
    const u32 kk = s_job.k;
    const bool general = s_job.general;
    int verdict = 0;
    while (acode != kNone) {
      wg_barrier();  // B2
      verdict = s_flag;
      if (verdict == 2) break;
      wg_barrier();  // B1
      u64 cc = s_wc[par][lane & (kRed - 1)];
      acode = s_wp[par][lane & (kRed - 1)];
      reduce16(cc, acode);
      acode = uni32(acode);
      par ^= 1;
    }
    if (verdict != 2) {
      u32 nsel = 0;
      u32 ccode = tcode;
      while (ccode != kNone) {
        if (!general) {
          if (++nsel == kk) break;
        } else {
          wg_barrier();  // B2 (ntasks > node_num only)
          if (s_flag == 1) break;
        }
        wg_barrier();  // B1
        u64 cc = s_wc[par][lane & (kRed - 1)];
        ccode = s_wp[par][lane & (kRed - 1)];
        reduce16(cc, ccode);
        ccode = uni32(ccode);
        par ^= 1;
      }
      wg_barrier();  // B3
    }
    wg_barrier();  // S1: owner updates applied, the selector may go on
  };

  if (wave == 0) {
    // =============================================================================================
    // SUPERVISOR — follows the scanners a few jobs behind: turns their decisions into tasks for the testers, and
    // runs everything that is not the autonomous fast path (serial jobs, flush, the end)
    // =============================================================================================
    WorkerShared sh;
    sh.wc = s_wc; sh.wp = s_wp; sh.flag = &s_flag; sh.nupd = &s_nupd; sh.upd = s_upd; sh.heap = s_heap; sh.part = part;
    HeapEnt* const gheap = P.heap + qbeg + part;
    u32 seq = 0;          // commands posted
    u32 nposted = 0;      // tasks posted

    auto post_cmd = [&](u32 kind, u32 job) {
      ++seq;
      if (lane == 0) { vst(&s_cmd[0], kind); vst(&s_cmd[1], job); lds_fence(); vst(&s_cmd_seq, seq); }
    };
    auto wait_scanners = [&]() -> bool {  // every scanner wave finished command `seq`
      for (u32 spin = 0;; ++spin) {
        const bool ok = lane < (u32)kPScanW0 || lane >= (u32)kPWaves || vld(&s_done[lane]) == seq;
        if (!__any(!ok)) return true;
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { pipe_fault(P, psh, 23, seq, 0, 0); return false; }
        nap();
      }
    };
    auto drain = [&]() -> bool {  // every posted task is final
      for (u32 spin = 0;; ++spin) {
        bool ok = true;
        if (lane < kPRing && nposted > lane) {
          const u32 e = nposted - lane;
          const PipeTask* s = &s_task[e & (kPRing - 1)];
          ok = vld(&s->id) != e || vld(&s->state) >= kTsFail;
        }
        if (!__any(!ok)) return true;
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { pipe_fault(P, psh, 24, nposted, 0, 0); return false; }
        nap();
      }
    };
    auto slot_free = [&](u32 id) -> bool {  // the ring slot of task `id` can be reused
      const PipeTask* s = &s_task[id & (kPRing - 1)];
      for (u32 spin = 0;; ++spin) {
        const u32 st = vld(&s->state);
        if (st == kTsFree || st >= kTsFail) return true;
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { pipe_fault(P, psh, 25, id, st, 0); return false; }
        nap();
      }
    };
    auto wait_exchange = [&](u32 e) -> bool {
      for (u32 spin = 0;; ++spin) {
        if (exchange_ready(e)) return true;
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { pipe_fault(P, psh, 26, e, vld(&s_arrive), 0); return false; }
        nap();
      }
    };
    // One job through k_select's sequential protocol (tile reloaded first: exact lengths and summaries).
    auto serial_job = [&](u32 jl) -> bool {
      PROF_T(sj0);
      post_cmd(kPcReload, jl);
      if (!wait_scanners()) return false;
      post_cmd(kPcSerial, jl);
      const u32 raw = fetch_job(P, jbeg + jl);
      job_to_lds(PG, jbeg + jl, raw, &s_job);
      wg_barrier();  // S0
      wg_barrier();  // B1 (round 0): A and T argmins published by the scanners
      u64 wc = s_wc[par][lane & (kRed - 1)];
      u32 wcode = s_wp[par][lane & (kRed - 1)];
      u64 tc = s_tc[lane & (kRed - 1)];
      u32 tcode = s_tp[lane & (kRed - 1)];
      reduce16(wc, wcode);
      reduce16(tc, tcode);
      par ^= 1;
      wc = uni64(wc); wcode = uni32(wcode); tc = uni64(tc); tcode = uni32(tcode);
      par = worker_job_slow<kPScan, false>(PG, sh, &s_job, par, wc, wcode, tc, tcode, qbeg, gheap);
      drain_stores();
      wg_barrier();  // S1
      PROF_T(sj1);
      PROF_ADD(4, sj0, sj1);  // supervisor: serial-mode job (reload + sequential protocol)
      return !vld(&s_abort);
    };

    u32 sup_pos = 0;       // next job whose decision is to be consumed
    u32 sup_nex = 0;       // next exchange to be consumed
    u32 stops_seen = 0;
    bool halt_sent = false;
    u32 raw = fetch_job(P, jbeg);
    u32 raw_n = njobs > 1 ? fetch_job(P, jbeg + 1) : 0u;
    u32 raw_j = 0;
    PROF_T(loop0);
    for (;;) {
      if (vld(&s_abort)) break;
      const bool flushing = vld(&s_flush_job) != kNone;
      if (flushing && !halt_sent) { if (lane == 0) vst(&s_halt, 1u); halt_sent = true; }
      const bool stopped = vld(&s_scan_stops) != stops_seen;   // read BEFORE the arrival count (see exchange_ready)
      lds_fence();
      if (exchange_ready(sup_nex)) {
        // ---- the scanners decided job sup_pos (or were halted in front of it) -----------------------------------
        PROF_T(w1);
        const u32 xs = sup_nex & (kPXRing - 1);
        if (vld(&s_xhalt[xs])) { ++sup_nex; if (lane == 0) vst(&s_sup_nex, sup_nex); continue; }
        if (raw_j != sup_pos) {
          raw = fetch_job(P, jbeg + sup_pos);
          raw_n = sup_pos + 1 < njobs ? fetch_job(P, jbeg + sup_pos + 1) : 0u;
          raw_j = sup_pos;
        }
        const u32 k = rl32(raw, kJrK);
        u32 kind = kPkFail, nfound = 0;
        u64 mycost = ~0ull;   // lane i < k: node i of the selection
        u32 mycode = kNone, myty = 0;
        if (k == 1) {
          decide_one(xs, kind, mycode, mycost, myty);
          nfound = kind != kPkFail ? 1u : 0u;
          ++sup_nex;
        } else {
          nfound = merge_lists(xs, k, mycost, mycode, myty);
          kind = kPkStart;
          ++sup_nex;
          if (nfound != k) {   // the scanners went on to the res_total lists: one more exchange
            if (!wait_exchange(sup_nex)) break;
            nfound = merge_lists(sup_nex & (kPXRing - 1), k, mycost, mycode, myty);
            kind = nfound == k ? (u32)kPkBackfill : (u32)kPkFail;
            ++sup_nex;
          }
        }
        if (lane == 0) vst(&s_sup_nex, sup_nex);
#ifdef CNS_EXP_NOTASKS   // timing experiment: the scanners' chain alone (no tester work; results are NOT valid)
        if (false) {
#else
        if (!flushing) {   // (a pending flush redoes this job anyway)
#endif
          if (nfound != k) {
            // not even k nodes whose res_total fits: "Resource" (:6335-6343, :6768); nothing changes
            const u32 orig = rl32(raw, kJrOrig);
            if (lane == 0) { P.o_start[orig] = 0; P.o_reason[orig] = CNS_REASON_RESOURCE; }
          } else {
            const u32 id = nposted + 1;
            PROF_T(f0);
            if (!slot_free(id)) break;
            PROF_T(f1);
            PROF_ADD(6, f0, f1);  // supervisor: waiting for a free task slot (testers are the bottleneck)
            PipeTask* const T = &s_task[id & (kPRing - 1)];
            if (lane < k) {
              const u32 sl = pslot(mycode);
              T->code[lane] = mycode;
              T->cost0[lane] = mycost;
              T->dep[lane] = s_last[sl];
              s_last[sl] = id;
            }
            if (lane == 0) {
              T->ji = sup_pos; T->kind_k = kind | (k << 8); T->id = id;
              lds_fence();
              vst(&T->state, kTsPosted);
              lds_fence();
              vst(&s_posted, id);
            }
            nposted = id;
            PROF_CNT(5);
          }
        }
        ++sup_pos;
        raw = raw_n; raw_j = sup_pos;
        raw_n = sup_pos + 1 < njobs ? fetch_job(P, jbeg + sup_pos + 1) : 0u;
        PROF_T(w2);
        PROF_ADD(1, w1, w2);  // supervisor: decision -> task
        continue;
      }
      if (stopped) {
        // ---- the scanners stand in front of job sup_pos: serial job, flush, or the end -----------------------------
        stops_seen = vld(&s_scan_stops);
        if (vld(&s_scan_pos) != sup_pos) { pipe_fault(P, psh, 27, vld(&s_scan_pos), sup_pos, sup_nex); break; }
        if (!drain()) break;
        const u32 fj = vld(&s_flush_job);
        if (lane == 0) { vst(&s_flush_job, kNone); vst(&s_halt, 0u); }
        halt_sent = false;
        lds_fence();
        u32 resume;
        if (fj != kNone) {            // a prediction failed at job fj: reload the committed state, redo it exactly
          PROF_CNT(3);
          if (!serial_job(fj)) break;
          resume = fj + 1;
        } else if (sup_pos >= njobs) {
          break;                      // the end: everything is committed
        } else {                      // a job outside the autonomous fast path
          PROF_CNT(2);
          if (!serial_job(sup_pos)) break;
          resume = sup_pos + 1;
        }
        sup_pos = resume;
        raw_j = kNone;
        post_cmd(kPcResume, resume);
        continue;
      }
      nap_idle();
    }
    PROF_T(loop1);
    PROF_ADD(19, loop0, loop1);  // supervisor: whole queue
    post_cmd(kPcExit, 0);
  } else if (wave < (u32)kPScanW0) {
    // =============================================================================================
    // TESTERS
    // =============================================================================================
    const u32 tw = wave - 1;
    u32 seen = 0;
    u32 my = 0;
    bool have = false;
    for (;;) {
      if (!have) {
        u32 c = 0;
        if (lane == 0) c = atomicAdd(&s_claim, 1u) + 1u;
        my = uni32(c);
        have = true;
      }
      bool leave = false, go = false;
      for (;;) {
        if (vld(&s_abort)) { leave = true; break; }
        const u32 cs = vld(&s_cmd_seq);
        if (cs != seen) {
          const u32 kind = vld(&s_cmd[0]);
          if (vld(&s_cmd_seq) == cs) {   // (seq, kind) read consistently
            seen = cs;
            if (kind == kPcSerial) { serial_follow(); continue; }
            if (kind == kPcExit) { leave = true; break; }
          }
          continue;
        }
        if (vld(&s_posted) >= my) { go = true; break; }
        nap_idle();
      }
      if (leave) break;
      if (go) {
        PROF_T(t0);
        if (P.wide_cores) pipe_tester_task<kPScan, true>(Pg, psh, my, tw, qbeg, resv_part, jbeg);
        else pipe_tester_task<kPScan, false>(Pg, psh, my, tw, qbeg, resv_part, jbeg);
        PROF_T(t1);
        PROF_ADD(8 + tw, t0, t1);  // tester busy cycles
        have = false;
      }
    }
  } else {
    // =============================================================================================
    // SCANNERS — register-resident node tile: slot p = r * kPScan + t, code = r << 10 | t.  They run the queue on
    // their own: scan, exchange the per-wave results, decide (every wave alike), update the own rows, next job.
    // =============================================================================================
    const u32 t = (wave - (u32)kPScanW0) * 64u + lane;
    using RM = u32;  // one bit per row of the lane (NPL <= 26)
    const RM kOne = 1;
    double cost[NPL];
    int fcpu[NPL];
    u32 mw[NPL];   // fmem GiB (16) | len (10) << 16 | type (6) << 26 ; len = 1023 marks "no node"
    u32 gn[NPL];   // per-class free-slot count, 4 bits each
    const u32 maxlen = P.max_jobs_per_node;
    RM okbits = 0;
    u64 wave_types = 0;
    auto load_tile = [&]() {
      okbits = 0;
      wave_types = 0;
#pragma unroll
      for (int r = 0; r < NPL; ++r) {
        const u32 p = (u32)r * kPScan + t;
        if (p < nn) {
          const u32 q = qbeg + p;
          const NodeHdr* hd = hdr_of(P, q);
          cost[r] = P.cost[q];
          fcpu[r] = P.f_cpu[q];
          mw[r] = mem_gib16(P.f_mem[q]) | (hd->len << 16) | ((u32)P.slot_type[q] << 26);
          gn[r] = nibbles_of(P.f_cnt[q]);
        } else {
          cost[r] = 0.0; fcpu[r] = 0; mw[r] = 1023u << 16; gn[r] = 0;
        }
        const u32 len = (mw[r] >> 16) & 0x3FFu;
        okbits |= (RM)(len < maxlen ? 1u : 0u) << r;
        if (len != 1023u) wave_types |= 1ull << (mw[r] >> 26);
      }
      wave_types = wave_or_u64(wave_types);
    };
    const u32 G8 = 0x80808080u;

    struct ScanJob {
      u32 flags, k, shape;
      int rc32;
      u32 rm16, rq, gtot, gmode, gsel, gneed;
      i64 L, mcpu;   // time limit, min-view cpu: the cost update of a selection
      u32 dm16, acnt;  // ... its memory in whole GiB (rounded down) and its GRES slots per class (nibbles)
    };
    auto decode = [&](u32 raw, u64& tyok) {   // the scanners' 12 dwords of the record (k_prep_jobs, kJsHead ff.)
      ScanJob S;
      const u32 head = rl32(raw, kJsHead), mem = rl32(raw, kJsMem), gr = rl32(raw, kJsGres);
      S.flags = head & 0xFFu;
      S.k = (head >> 8) & 0xFFFFu;
      S.shape = head >> 24;
      S.rc32 = (int)rl32(raw, kJsRc32);
      S.rm16 = mem & 0xFFFFu;
      S.dm16 = mem >> 16;
      S.rq = rl32(raw, kJsRq);
      S.gtot = rl32(raw, kJsGtot);
      S.gmode = gr & 0xFu;
      S.gsel = (gr >> 4) & 0xFFFu;
      S.gneed = gr >> 16;
      S.L = (i64)jr64(raw, kJsL);
      S.mcpu = (i64)S.rc32;   // exact whenever the request is satisfiable at all (shape bit 2)
      S.acnt = rl32(raw, kJsAcnt);
      tyok = jr64(raw, kJsTyok);
      return S;
    };
    auto lane_argmin = [&](RM mask, u64& bc, u32& bp) {
      bc = ~0ull;
      u32 br = 0xFFu;
#pragma unroll
      for (int r = 0; r < NPL; ++r) {
        const u64 ck = cost_key(cost[r]);
        const bool take = ((mask >> r) & 1u) & (ck < bc);
        bc = take ? ck : bc;
        br = take ? (u32)r : br;
      }
      bp = br == 0xFFu ? kNone : ((br << 10) | t);
    };
    auto row_type = [&](u32 code) -> u32 {  // node type of one of THIS lane's rows
      const int rr = (int)(code >> 10);
      u32 ty = 0;
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if (r == rr) ty = mw[r] >> 26;
      return ty;
    };
    // Candidate sets of one job as per-lane bitmasks + their lane-local argmins (k_select's scan_job without the
    // pre-scan skip mask).
    auto scan_job = [&](const ScanJob& S, u64 sji, u64 tyok, bool lean, RM& bmask, RM& amask, u64& ac, u32& ap, u64& tcs, u32& tp) {
      RM tybits = (RM)(((u64)1 << NPL) - 1ull);
      if ((tyok & wave_types) != wave_types) {
        tybits = 0;
#pragma unroll
        for (int r = 0; r < NPL; ++r) tybits |= (RM)((tyok >> (mw[r] >> 26)) & 1ull) << r;
      }
      const RM bl = (S.shape & 4u) ? (RM)(okbits & tybits) : (RM)0;
      u32 gme = 0, gmo = 0;
      if (S.gmode & 2u) { gme = uni32(s_nme[S.gsel >> 8]); gmo = uni32(s_nmo[S.gsel >> 8]); }
      RM am = 0;
      ac = ~0ull; tcs = ~0ull;
      u32 ar = 0xFFu, tr = 0xFFu;
      auto rows = [&](auto mode, auto leantag) {
        constexpr u32 M = decltype(mode)::value;
        constexpr bool kLean = decltype(leantag)::value != 0;   // start-now argmin only (T comes from the wave's cache)
        const u32 sh1 = S.gsel & 0xFFu, need1 = S.gneed & 0xFFu, need2 = S.gneed >> 8;
        const u32 rqe = S.rq & 0x0F0F0F0Fu, rqo = (S.rq >> 4) & 0x0F0F0F0Fu;
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
          const bool b = ((bl >> r) & 1u) != 0;
          bool a = b & (S.rc32 <= fcpu[r]) & (S.rm16 <= (mw[r] & 0xFFFFu));
          if (M == 1) {
            const u32 g = gn[r];
            if (S.gmode & 1u) a = a & (((g >> sh1) & 15u) >= need1);
            if (S.gmode & 2u) {
              const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
              a = a & (__builtin_amdgcn_sad_u8(ce & gme, 0u, __builtin_amdgcn_sad_u8(co & gmo, 0u, 0u)) >= need2);
            }
          }
          if (M == 4) {
            const u32 g = gn[r];
            const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
            a = a & ((((ce | G8) - rqe) & G8) == G8) & ((((co | G8) - rqo) & G8) == G8);
#pragma unroll
            for (int n = 0; n < kMaxNames; ++n) {
              const u32 tot = (S.gtot >> (8 * n)) & 0xFFu;
              const u32 have = __builtin_amdgcn_sad_u8(ce & s_nme[n], 0u, __builtin_amdgcn_sad_u8(co & s_nmo[n], 0u, 0u));
              a = a & ((tot == 0) | (have >= (tot > 15u ? 15u : tot)));
            }
          }
          const u64 ck = cost_key(cost[r]);
          const bool ta = a & (ck < ac);
          ac = ta ? ck : ac;
          ar = ta ? (u32)r : ar;
          if (!kLean) {
            const bool tt = b & (ck < tcs);
            tcs = tt ? ck : tcs;
            tr = tt ? (u32)r : tr;
            am |= (RM)(a ? 1u : 0u) << r;
          }
        }
      };
      if (lean) {
        if (S.gmode == 0) rows(ModeTag<0>{}, ModeTag<1>{});
        else if (S.gmode < 4) rows(ModeTag<1>{}, ModeTag<1>{});
        else rows(ModeTag<4>{}, ModeTag<1>{});
      } else {
        if (S.gmode == 0) rows(ModeTag<0>{}, ModeTag<0>{});
        else if (S.gmode < 4) rows(ModeTag<1>{}, ModeTag<0>{});
        else rows(ModeTag<4>{}, ModeTag<0>{});
      }
      bmask = bl; amask = am;
      ap = ar == 0xFFu ? kNone : ((ar << 10) | t);
      tp = tr == 0xFFu ? kNone : ((tr << 10) | t);
      if (S.flags & kJfExclusive) {  // exclusive: the node must be completely free now (necessary for :6251-6257)
        amask = 0;
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
          const u32 w = mw[r];
          const u32 ty = w >> 26;
          const bool a = ((bmask >> r) & 1u) & (fcpu[r] >= s_ty_cpu[ty]) & ((w & 0xFFFFu) >= s_ty_m16[ty]) &
                         (gn[r] == s_ty_gn[ty]);
          amask |= (RM)(a ? 1u : 0u) << r;
        }
        lane_argmin(amask, ac, ap);
      }
      if (S.flags & (kJfIncl | kJfExcl)) {  // included / excluded node lists (rare)
        const RM lm = (RM)list_mask<kPScan>(Pg, S.flags, sji, bmask, qbeg + t, (u32)NPL);
        bmask &= lm;
        amask &= lm;
        lane_argmin(amask, ac, ap);
        lane_argmin(bmask, tcs, tp);
      }
    };
    // exact refresh after a SERIAL job (what the committing wave read from the node block)
    auto apply_upd = [&](const UpdRec& u, u32 up) {
      const int rr = (int)(up >> 10);
      const bool own = (up & 1023u) == t;
      const double ucost = u.cost;
      const u32 ulen = u.len, ufront = u.has_front;
      const int ucpu = u.fcpu;
      const u32 um16 = mem_gib16(u.fmem), ugn = nibbles_of(u.fcnt);
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if (r == rr) {
          u32 w = (mw[r] & ~(0x3FFu << 16)) | (ulen << 16);
          if (ufront) w = (w & ~0xFFFFu) | um16;
          cost[r] = own ? ucost : cost[r];
          mw[r] = own ? w : mw[r];
          okbits = own ? (RM)((okbits & ~(kOne << r)) | ((RM)(ulen < maxlen ? 1u : 0u) << r)) : okbits;
          fcpu[r] = (own && ufront) ? ucpu : fcpu[r];
          gn[r] = (own && ufront) ? ugn : gn[r];
        }
    };
    // predicted effect of a selection on the row that holds node `code` (the commit itself happens later, on a tester
    // wave): MinCpuTimeRatioFirst::UpdateCost (JobScheduler.h:47-53: ratio first, then x seconds, then +=; end - start is
    // the time limit whatever the start) and, for a start-now selection, the front summary minus the allocation.
    // `code` is wave-uniform, so the row select is a scalar branch: read the row, compute once, write it back.
    auto apply_sel = [&](const ScanJob& S, u32 code, u64 cost0, u32 ty, bool front) {
      const int rr = (int)(code >> 10);
      const bool own = (code & 1023u) == t;
      const double ratio = ((double)S.mcpu / 256.0) / ((double)s_tytot[ty] / 256.0);
      const double ucost = __longlong_as_double((long long)cost0) + (double)S.L * ratio;
      u32 w = 0, g = 0;
      int fc = 0;
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if (r == rr) { w = mw[r]; g = gn[r]; fc = fcpu[r]; }
      if (front) {
        const u32 m16 = w & 0xFFFFu, dm = S.dm16;
        const u32 n16 = m16 == 0xFFFFu ? m16 : (m16 > dm ? m16 - dm : 0u);   // whole GiB, rounded down: stays an upper bound
        w = (w & ~0xFFFFu) | n16;
        fc -= S.rc32;
        const u32 dg = S.acnt;
        if (dg) {
          u32 ng = 0;
#pragma unroll
          for (int c = 0; c < 8; ++c) {   // per class: a saturated count ("15 or more") stays, else it drops
            const u32 o = (g >> (4 * c)) & 15u, d = (dg >> (4 * c)) & 15u;
            ng |= (o == 15u ? 15u : (o > d ? o - d : 0u)) << (4 * c);
          }
          g = ng;
        }
      }
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if (r == rr) {
          cost[r] = own ? ucost : cost[r];
          mw[r] = own ? w : mw[r];
          gn[r] = own ? g : gn[r];
          fcpu[r] = own ? fc : fcpu[r];
        }
    };

    const bool leader = wave == (u32)kPScanW0;
    const u32 sid = wave - (u32)kPScanW0;
    u32 seen = 0;
    u32 pos = 0;                // next job of the autonomous run
    u32 nex = 0;                // exchanges so far
    u32 stops = 0;
    bool running = true;        // autonomous (else: waiting for the supervisor's commands)
    u32 have_raw_j = kNone;     // job whose record sits in `raw`
    u32 raw = 0;
    RM bmask = 0, amask = 0;
    ScanJob J;
    u64 typeok = 0;
    J.k = 1; J.flags = 0; J.shape = 0;
    bool boot = true;           // the first pass loads the tile
#ifndef CNS_PIPE_LEAN
#define CNS_PIPE_LEAN 1
#endif
    // Per-wave cache of the res_total argmin T (wave-uniform).  For a node_num == 1 job without node lists that may use
    // every node type of the wave, T does not depend on the job: it is kept until the cached node itself is selected
    // (its cost grows) or the tile is reloaded.  With T cached the row loop only tracks the start-now argmin.
    // (Measured: a second entry for other type masks, the cached node's type, or bounds on the free cpu / memory that
    // would skip the row loop each cost more registers than they save work - the tile leaves ~80 of 168 VGPRs.)
#ifdef CNS_PIPE_CHECK
    u32 dbg_fill = 0, dbg_napp = 0;
#endif
    bool tvalid = false;
    u64 tc_c = ~0ull;
    u32 tp_c = kNone;
    auto stop_at = [&](u32 j) {
      ++stops;
      if (leader && lane == 0) { vst(&s_scan_pos, j); lds_fence(); vst(&s_scan_stops, stops); }
      running = false;
    };
    auto arrive_and_wait = [&]() -> bool {   // one exchange: everything this wave published is visible to the others after it
      if (lane == 0) { lds_fence(); atomicAdd(&s_arrive, 1u); }
      const u32 want = (u32)kPScanWaves * (nex + 1u);
      for (u32 spin = 0;; ++spin) {
        if (vld(&s_arrive) >= want) break;
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { pipe_fault(P, psh, 28, nex, vld(&s_arrive), wave); return false; }
        __builtin_amdgcn_s_sleep(1);
      }
      ++nex;
      return true;
    };
    // this wave's k best candidates of `m`, sorted, into exchange slot xs
    auto post_lists = [&](u32 xs, RM m, u32 k) {
      const u32 base = sid * kPMaxK;
      bool dry = false;
      for (u32 i = 0; i < k; ++i) {
        u64 c = ~0ull;
        u32 pc = kNone;
        if (!dry) {
          lane_argmin(m, c, pc);
          wave_argmin(c, pc);
        }
        if (pc != kNone && (pc & 1023u) == t) { s_xlty[xs][base + i] = row_type(pc); m &= ~(kOne << (pc >> 10)); }
        if (lane == 0) { s_xlc[xs][base + i] = c; s_xlp[xs][base + i] = pc; }
        if (pc == kNone) dry = true;
      }
    };
    for (;;) {
      // ---- what next: the autonomous run, or a command of the supervisor -----------------------------------------
      u32 kind = 0, cj = 0;
      PROF_T(c0);
      if (boot) kind = kPcReload;
      while (!boot && !running) {
        if (vld(&s_abort)) { kind = kPcExit; break; }
        const u32 cs = vld(&s_cmd_seq);
        if (cs != seen) {
          kind = vld(&s_cmd[0]); cj = vld(&s_cmd[1]);
          if (vld(&s_cmd_seq) == cs) { seen = cs; break; }
          continue;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if (!boot && running && vld(&s_abort)) kind = kPcExit;
      PROF_T(c1);
      if (leader) PROF_ADD(17, c0, c1);  // first scanner wave: waiting for a command
      if (kind == kPcExit) break;
      if (kind == kPcReload) {
        load_tile();
        tvalid = false;
        have_raw_j = kNone;
        if (!boot && lane == 0) { lds_fence(); vst(&s_done[wave], seen); }
        boot = false;
        continue;
      }
      if (kind == kPcResume) { pos = cj; running = true; have_raw_j = kNone; continue; }
      const bool serial = kind == kPcSerial;
      const u32 j = serial ? cj : pos;
      if (!serial && j >= njobs) { stop_at(j); continue; }
      // ---- the one scan of the job: candidate sets + lane-local argmins -------------------------------------------
      if (serial || have_raw_j != j) raw = fetch_job(P, jbeg + j);
      J = decode(raw, typeok);
      if (!serial) {
        const bool piped = !(J.flags & kJfExclusive) && (J.shape & 11u) == 2u && J.k >= 1 && J.k <= (u32)kPMaxK;
        if (!piped) { have_raw_j = kNone; stop_at(j); continue; }   // the supervisor runs it through the sequential protocol
      }
      if (!serial && j + 1 < njobs) { raw = fetch_job(P, jbeg + j + 1); have_raw_j = j + 1; }   // in flight during this scan
      else have_raw_j = kNone;
      u64 ac = ~0ull, tcs = ~0ull;
      u32 ap = kNone, tp = kNone;
      PROF_T(q1);
      // jobs whose T set is static: node_num == 1, satisfiable, no node lists (T then follows from the allowed types)
      const bool stat = CNS_PIPE_LEAN && !serial && J.k == 1 && (J.shape & 4u) && !(J.flags & (kJfExclusive | kJfIncl | kJfExcl));
      const bool lean = stat && tvalid && (typeok & wave_types) == wave_types;
      scan_job(J, jbeg + j, typeok, lean, bmask, amask, ac, ap, tcs, tp);
      if (leader && !serial) { if (lean) PROF_CNT(25); else PROF_CNT(28); }
      PROF_T(q2);
      if (leader) PROF_ADD(22, q1, q2);  // first scanner wave: row loop (filters + lane-local argmins)
      if (serial || J.k == 1) {
        if (__any(ap != kNone)) wave_argmin(ac, ap);   // (else: every lane already holds "none")
        if (lean) {
          tcs = tc_c;
          tp = tp_c;
        } else {
          wave_argmin(tcs, tp);
          if (stat && (typeok & wave_types) == wave_types) {
            tc_c = uni64(tcs); tp_c = uni32(tp); tvalid = true;
#ifdef CNS_PIPE_CHECK
            dbg_fill = j; dbg_napp = 0;
#endif
          }
        }
      }
#ifdef CNS_PIPE_CHECK   // debug build: every shortcut against the full scan
      if (lean) {
        u64 ac2 = ~0ull, tc2 = ~0ull;
        u32 ap2 = kNone, tp2 = kNone;
        RM b2 = 0, a2 = 0;
        scan_job(J, jbeg + j, typeok, false, b2, a2, ac2, ap2, tc2, tp2);
        wave_argmin(ac2, ap2);
        wave_argmin(tc2, tp2);
        if (uni32(tp2) != uni32(tp) || uni64(tc2) != uni64(tcs)) { pipe_fault(P, psh, 30, j | (wave << 24), (uni32(tp2) & 0xFFFFu) | (dbg_fill << 16), (uni32(tp) & 0xFFFFu) | (dbg_napp << 16)); break; }
        if (uni32(ap2) != uni32(ap) || uni64(ac2) != uni64(ac)) { pipe_fault(P, psh, 32, j, uni32(ap2), uni32(ap)); break; }
      }
#endif
      PROF_T(q3);
      if (leader) PROF_ADD(23, q2, q3);  // ... two wave argmins (DPP)
      if (serial) {
        // ---- one job through the sequential protocol (mirror of worker_job_slow) -----------------------------
        const u32 kk = J.k;
        const bool general = (J.shape & 1u) != 0;
        wg_barrier();  // S0
        if (lane == 0) { s_wc[par][wave] = ac; s_wp[par][wave] = ap; s_tc[wave] = tcs; s_tp[wave] = tp; }
        wg_barrier();  // B1
        u64 wc = s_wc[par][lane & (kRed - 1)];
        u32 wcode = s_wp[par][lane & (kRed - 1)];
        u64 tc = s_tc[lane & (kRed - 1)];
        u32 tcode = s_tp[lane & (kRed - 1)];
        reduce16(wc, wcode);
        reduce16(tc, tcode);
        par ^= 1;
        wcode = uni32(wcode); tcode = uni32(tcode);
        // Phase A walks the start-now set, Phase B the res_total set: ONE loop over (phase, candidate) so that the tile
        // is only touched from one lane_argmin site
        int verdict = 0;
        RM used = 0;
        u32 nsel = 0;
        bool phase_b = wcode == kNone;
        u32 cur = phase_b ? tcode : wcode;
        bool b3 = phase_b;         // Phase B ends with B3
        for (;;) {
          if (cur == kNone) {
            if (!phase_b) { phase_b = true; b3 = true; used = 0; cur = tcode; continue; }   // :6335 ff.
            break;
          }
          if ((cur & 1023u) == t) used |= kOne << (cur >> 10);
          if (!phase_b) {
            wg_barrier();  // B2
            verdict = s_flag;
            if (verdict == 2) break;
          } else if (!general) {
            if (++nsel == kk) break;
          } else {
            wg_barrier();  // B2 (ntasks > node_num only)
            if (s_flag == 1) break;
          }
          u64 c = ~0ull;
          u32 pc = kNone;
          lane_argmin((phase_b ? bmask : amask) & ~used, c, pc);
          wave_argmin(c, pc);
          if (lane == 0) { s_wc[par][wave] = c; s_wp[par][wave] = pc; }
          wg_barrier();  // B1
          u64 c2 = s_wc[par][lane & (kRed - 1)];
          cur = s_wp[par][lane & (kRed - 1)];
          reduce16(c2, cur);
          cur = uni32(cur);
          par ^= 1;
        }
        if (b3 && verdict != 2) {
          wg_barrier();  // B3
          verdict = s_flag;
        }
        if (verdict == 2) {   // owners refresh their registers with the exact values
          const int nu = s_nupd;
          const UpdRec* const ub = nu <= kMaxUpd ? (const UpdRec*)s_upd : (const UpdRec*)(P.g_upd + qbeg);
          for (int i = 0; i < nu; ++i) {
            const u32 up = uni32(ub[i].p);
            if (powner(up) == wave) apply_upd(ub[i], up);
          }
          tvalid = false;
        }
        wg_barrier();  // S1
        continue;
      }
      // ---- autonomous: exchange, decide, update the own rows -----------------------------------------------------
      u32 xs = nex & (kPXRing - 1);
      if (leader) {
        // the supervisor reads the exchange ring a few jobs later: do not lap it; and pass its halt request on
        for (u32 spin = 0; nex + 2u >= vld(&s_sup_nex) + kPXRing; ++spin) {
          if (vld(&s_abort)) break;
          if (spin > kPSpinLimit) { pipe_fault(P, psh, 29, nex, vld(&s_sup_nex), 0); break; }
          nap();
        }
        if (lane == 0) vst(&s_xhalt[xs], vld(&s_halt));
      }
      if (J.k == 1) {
        if (ap != kNone && (ap & 1023u) == t) s_res[xs][sid].aty = row_type(ap);
        if (tp != kNone && (tp & 1023u) == t) s_res[xs][sid].tty = row_type(tp);
        if (lane == 0) { s_res[xs][sid].ac = ac; s_res[xs][sid].ap = ap; s_res[xs][sid].tc = tcs; s_res[xs][sid].tp = tp; }
      } else {
        post_lists(xs, amask, J.k);
      }
      if (!arrive_and_wait()) break;
      PROF_T(q4);
      if (leader) PROF_ADD(24, q3, q4);  // first scanner wave: publish + exchange wait
      if (vld(&s_xhalt[xs])) { have_raw_j = kNone; stop_at(j); continue; }   // halted in front of job j: nothing applied
      const u32 k = J.k;
      u32 dkind = kPkFail, nfound = 0;
      u64 mycost = ~0ull;
      u32 mycode = kNone, myty = 0;
      if (k == 1) {
        decide_one(xs, dkind, mycode, mycost, myty);
        nfound = dkind != kPkFail ? 1u : 0u;
      } else {
        nfound = merge_lists(xs, k, mycost, mycode, myty);
        dkind = kPkStart;
        if (nfound != k) {   // fewer than k nodes can start it now -> first k by res_total + backfill (:6335-6376)
          xs = nex & (kPXRing - 1);
          if (leader) {
            for (u32 spin = 0; nex + 2u >= vld(&s_sup_nex) + kPXRing; ++spin) {
              if (vld(&s_abort)) break;
              if (spin > kPSpinLimit) { pipe_fault(P, psh, 29, nex, vld(&s_sup_nex), 1); break; }
              nap();
            }
            if (lane == 0) vst(&s_xhalt[xs], 0u);
          }
          post_lists(xs, bmask, k);
          if (!arrive_and_wait()) break;
          nfound = merge_lists(xs, k, mycost, mycode, myty);
          dkind = nfound == k ? (u32)kPkBackfill : (u32)kPkFail;
        }
      }
      if (nfound == k) {
        for (u32 i = 0; i < k; ++i) {
          const u32 code = k == 1 ? mycode : rl32(mycode, i);
          if (powner(code) != wave) continue;
          const u64 c0 = k == 1 ? mycost : rl64(mycost, i);
          const u32 ty = k == 1 ? myty : rl32(myty, i);
          apply_sel(J, code, c0, ty, dkind == kPkStart);
          if (code == tp_c) tvalid = false;   // the cached T argmin got more expensive
#ifdef CNS_PIPE_CHECK
          ++dbg_napp;
#endif
        }
      }
      ++pos;
      PROF_T(q5);
      if (leader) { PROF_ADD(20, q4, q5); PROF_ADD(16, c1, q5); PROF_CNT(18); }  // decision + own-row update; whole job
    }
  }
}

#define CNS_PIPE_INSTANTIATE(w) template __global__ void k_pipe<w>(const KParams, const KParams*);
CNS_PNPL_LIST(CNS_PIPE_INSTANTIATE)
#undef CNS_PIPE_INSTANTIATE
