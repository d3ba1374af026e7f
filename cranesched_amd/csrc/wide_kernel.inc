// k_wide<NPL> — k_pipe's protocol with the sequential chain of a partition spread over MANY compute units.
// Included from select_kernels.hip after pipe_kernel.inc (inside namespace cns); shares the task ring, the tester
// routine and every device routine with k_pipe / k_select.
//
// Why: k_pipe's chain (scan -> LDS exchange -> replicated decision -> own-row update) is bound by the instruction
// issue of ONE CU that 12 waves share (DESIGN.md 5.1: 59 % VALU busy, 8 scanner waves x 16 rows, 3 waves per SIMD).
// Here a partition gets 1 + 8 workgroups:
//
//   workgroup 0 ("home")      wave 0 SUPERVISOR, waves 1-7 TESTERS — k_pipe's roles, unchanged in what they do
//                             (round 6: up to three more home workgroups behind the scanners' — "MORE THAN ONE HOME WORKGROUP PER PARTITION")
//   workgroups 1-8            4 SCANNER waves each, ONE PER SIMD (waves 4-7 leave at once): 32 scanner waves x 64 lanes x
//                             NPL <= 8 rows = up to 16 384 nodes; each wave has its SIMD to itself
//
// The scanners' per-job exchange goes through HBM instead of LDS: every wave writes its A / T argmin (or its top-k
// list) as 16-byte data-tagged granules {exchange number, slot code | node type, fp64 cost key} with ONE write-through
// (sc1) store per granule, and every wave — plus the supervisor, a few jobs later — polls the 64 granules of the
// exchange with sc1 loads until all carry the current exchange number (MI355X_MICROARCH.md "handoff-1to1": ~1 us, no
// separate flag, no fence).  Then every wave computes the same decision and the owner updates its row: k_pipe's
// replicated decision, unchanged.  All workgroups of a partition are placed on one XCD (block b runs on XCD b % 8 —
// a speed heuristic only; nothing below depends on it).
//
// Control words (halt request, commands, stop reports, abort) are agent-scope relaxed atomics in the partition's
// WideCtl block; payload-before-flag ordering is an explicit s_waitcnt vmcnt(0) between the sc1 stores.  The tile
// reload after a flush / serial job reads state that the HOME workgroup committed with plain stores: the supervisor
// issues an agent-scope release fence before the Resume command and every scanner wave an agent-scope acquire fence
// after it (guide: "plain stores -> release -> flag; poll -> acquire -> plain loads").
//
// Serial jobs (everything outside the pipelined shapes, and the redo after a flush) stay INSIDE the home workgroup:
// the supervisor runs worker_job_slow as in k_pipe, and the seven tester waves serve it as MEMORY scanners — the same
// candidate protocol (A / T argmin per round, used-masks, B1/B2/B3 barriers) over the committed HBM arrays
// (cost, front summaries, map lengths) instead of a register tile.  They are rare (C4: 30 per 125 000 jobs).
//
// Every wait is bounded and raises a device fault instead of hanging.

#ifndef CNS_WIDE_SPW
#define CNS_WIDE_SPW 4                         // scanner waves per scanner workgroup: 4 (one per SIMD) or 8 (two per SIMD)
#endif
#ifndef CNS_WIDE_WGS
#define CNS_WIDE_WGS 8                         // scanner workgroups per partition
#endif
#if CNS_WIDE_SPW * CNS_WIDE_WGS == 32
#define CNS_WNPL_LIST(X) X(1) X(2) X(4) X(8)
constexpr int kWNplMax = 8;
constexpr u32 kWShift = 11;
#elif CNS_WIDE_SPW * CNS_WIDE_WGS == 64
#define CNS_WNPL_LIST(X) X(1) X(2) X(4) X(8) X(16)
constexpr int kWNplMax = 16;                   // 4 096 lanes x 16 rows = 65 536 nodes per partition (8 / 16 rows: the last-task table of
constexpr u32 kWShift = 12;                    // the home workgroup moves from LDS to HBM, KParams::wide_last)
#elif CNS_WIDE_SPW * CNS_WIDE_WGS == 16
#define CNS_WNPL_LIST(X) X(1) X(2) X(4) X(8)
constexpr int kWNplMax = 8;                    // 1 024 lanes x 8 rows = 8 192 nodes per partition: clusters of 25..48 partitions (5 workgroups each)
constexpr u32 kWShift = 10;
#elif CNS_WIDE_SPW * CNS_WIDE_WGS == 8
#define CNS_WNPL_LIST(X) X(1) X(2) X(4) X(8)
constexpr int kWNplMax = 8;                    // 512 lanes x 8 rows = 4 096 nodes per partition: clusters of 49..80 partitions (3 workgroups each)
constexpr u32 kWShift = 9;
#else
#error "k_wide: 8, 16, 32 or 64 scanner waves per partition"
#endif
#ifndef CNS_WIDE_BLOCK
#define CNS_WIDE_BLOCK 512
#endif
constexpr int kWBlock = CNS_WIDE_BLOCK;        // 8 waves; scanner workgroups use kWScanPerWg of them (measured in round 3: 768 / 1024 threads = 11 / 15
                                               // tester waves at 168 / 128 VGPRs: C4 307 / 394 ms against 308 — the chain of the scanners is as long, DESIGN 5.3)
constexpr int kWTesters = kWBlock / 64 - 1;    // home workgroup: waves 1..7
constexpr int kWScanPerWg = CNS_WIDE_SPW;      // scanner waves per scanner workgroup
constexpr int kWSW = CNS_WIDE_WGS * kWScanPerWg;   // scanner waves per partition
constexpr u32 kWXr = 2u * (u32)kWSW;           // granules of a node_num == 1 exchange
// A WINDOW OF JOBS PER EXCHANGE (round 5; the 64-wave build): the scanner waves exchange their CANDIDATE POOL — every wave's kWM cheapest
// rows with their state, and the key of its next row — once, and then decide up to kWJ consecutive one-node jobs of the steady-state shape
// on their copies of the pool without further communication ("A WINDOW OF JOBS PER EXCHANGE" in the scanners' loop; the rule and why it is
// exact: tests/test_exchange_pairs_model.py).  A pool exchange is kWPG granules per wave in a ring of its own (tag: the window's number).
#ifndef CNS_WIDE_WIN
#define CNS_WIDE_WIN 32      // (round 6: 16 -> 32 — with two home workgroups per partition the testers keep up with longer bursts: C5 146.6 -> 144.0 ms, C2 113.9 -> 112.6; 48: the same)
#endif
#ifndef CNS_WIDE_POOL
#define CNS_WIDE_POOL 2
#endif
#if CNS_WIDE_SPW * CNS_WIDE_WGS == 64 && CNS_WIDE_WIN >= 2
#define CNS_WIDE_WINDOWS 1
constexpr u32 kWJ = CNS_WIDE_WIN;              // jobs per window at most (the decision ring must hold them: lap_guard)
#else
constexpr u32 kWJ = 0;
#endif
constexpr u32 kWB = 4;                         // ... decided in chunks of kWB records (the record queue of the window path)
constexpr u32 kWM = CNS_WIDE_POOL;             // rows per wave in the pool
constexpr u32 kWPG = 2u * kWM + 1u;            // granules per wave and pool exchange: per row {payload | dip << 30, cost} and {front cpu, mem | len | type, GRES counts}; the bound
constexpr u32 kWPRing = 4;                     // pool exchanges in flight (a wave is at most one window ahead of the slowest)
constexpr u32 kWXrow = kWXr;                   // granules per ring row of the single-job exchange
constexpr u32 kWLl = (u32)kWSW * 8u / 64u;     // granules per lane of a list exchange
constexpr u32 kWLanes = (u32)kWSW * 64u;       // 2048 scanner lanes = nodes per tile row; slot p = r * kWLanes + gt = its code
static_assert(kWLanes == (1u << kWShift), "code = slot");
constexpr int kWScanWgs = kWSW / kWScanPerWg;  // 8
constexpr int kWGroup = 1 + kWScanWgs;         // workgroups per partition without extra home workgroups (KParams::wide_aux adds up to kWAuxMax)
// MORE THAN ONE HOME WORKGROUP PER PARTITION (round 6).  One supervisor wave and seven testers give a partition ~2 600 (C5) to ~4 400 (C4)
// cycles of test + commit capacity per task; the scanners deliver faster than that wherever the pool windows work (C5, C2), and more tester
// waves on the SAME compute unit do not help (168 VGPRs: spills).  So a partition may get up to kWAuxMax further home workgroups, on CUs of
// its XCD that the launch left idle.  Every home runs the same code: its supervisor reads the SAME decision ring, numbers the tasks of the
// stream identically (gid 1, 2, ...: a pure function of the stream), posts task gid into its OWN LDS ring iff (gid - 1) % H is its index
// and only notes the others in its last-task table.  What crosses workgroups — through 16-byte granules in the XCD's L2, written and read
// by the supervisors, off every tester's path:
//   * "every older task has a verdict" (the condition of a commit): home g exports wv[g] = the gid up to which all ITS tasks have one; a task
//     gid of home h may retire once wv[g] >= the last gid below it that g owns, for every g != h (WideHome::allow);
//   * a misprediction: the flushing job's index travels in the SAME granule as wv, so whoever sees wv pass the failed task sees the flush;
//   * a dependency on a task of another home (same node, rare): wait for that home's watermark of FINAL tasks, wf[g];
//   * stops: every home drains, the extra homes report (and the failed task's cause, if it is theirs), home 0 mends the chain as before and
//     its Resume command — the one the scanners read — restarts every supervisor at the same job.
// Node blocks written on one CU are read on another: the testers invalidate their L1 behind the dependency wait (the XCD's L2 is the
// point of coherence); with the partition's workgroups on several XCDs (the census says so) the extra homes leave and home 0 works alone.
// Model of the protocol against a sequential commit order: tests/test_multi_home_model.py.
// (the file is compiled once per scanner-wave count: the constant is derived afresh each time; -DCNS_WIDE_AUX_CAP=<n> caps it in experiment builds)
#if CNS_WIDE_SPW * CNS_WIDE_WGS == 64
constexpr u32 kWAuxBuild = 3;                  // 20 workgroups per partition at most: 8 partitions -> 160 of 256 CUs, 20 of the 32 of an XCD
#elif CNS_WIDE_SPW * CNS_WIDE_WGS == 32
constexpr u32 kWAuxBuild = 1;                  // 10 workgroups: still three partitions per XCD (24 per launch)
#else
constexpr u32 kWAuxBuild = 1;                  // 5 / 3 workgroups per partition: one more where the launch leaves a CU per partition (up to 40 / 64
                                               // partitions: C4p64 = 64 x 4 workgroups = all 256 CUs); the host drops it where it does not fit
#endif
#ifdef CNS_WIDE_AUX_CAP
constexpr u32 kWAuxMax = kWAuxBuild < (u32)(CNS_WIDE_AUX_CAP) ? kWAuxBuild : (u32)(CNS_WIDE_AUX_CAP);
#else
constexpr u32 kWAuxMax = kWAuxBuild;
#endif
constexpr u32 kWHomesMax = 1u + kWAuxMax;
static_assert(kWHomesMax <= 4u && (u32)kWGroup + kWAuxMax <= 32u, "WideCtl::hx / WideCtl::xcc");
constexpr u32 kWDepLocal = 0x80000000u;        // WideTask::dep / the last-task table: bit 31 = a task id of THIS home's ring, else the gid of another home's task
#ifndef CNS_WIDE_RING
#define CNS_WIDE_RING 64
#endif
constexpr u32 kWRing = kWSW == 64 ? CNS_WIDE_RING : 32;   // exchanges the supervisor may lag behind the scanners (power of two; 64 where a window decides up to kWJ jobs in one burst)
static_assert(kWJ + 8u < kWRing, "the decisions of a window must fit the decision ring next to what the supervisor has not consumed yet");
constexpr u32 kWTRing = 64;                    // task slots of the home workgroup (power of two, <= 64: one lane per slot in drain)
constexpr u32 kWNonePay = 0x3FFFFFFFu;         // payload "no node": code 0xFFFFFF, type 63
constexpr u32 kWMs = (u32)kWTesters * 64u;     // memory-scanner lanes of a serial job
constexpr u32 kWMsTrip = 4;                    // ... rows of one lane per trip of its scan (every load of a trip in flight before any is looked at; 64 % kWMsTrip == 0)
constexpr u32 kWMemWords = 5;                  // ... each with up to 64 x kWMemWords rows: 448 x 320 = 143 360 slots (an ALL partition over 65 536 nodes
                                               // next to partitions that cover them once more = 131 072)
constexpr u32 kWMemWordsGiant = 19;            // the giant instantiation of the serial-only mode (k_wide<1, false, kWMemWordsGiant>): 448 x 1 216 = 544 768
                                               // slots >= 524 288 (an ALL partition over 262 144 nodes next to subsets that cover it once more)
constexpr u32 kWSpinLimit = 1u << 22;          // polls of an exchange (>= ~0.5 us each): > 2 s without progress is a protocol bug
constexpr u32 kWCmdSpinLimit = 1u << 23;       // polls for a command (the supervisor may be in a long serial job)
constexpr u32 kWMaxParts = (32u / (u32)kWGroup) * 8u;   // (without extra homes; the host sizes KParams::wide_aux so that the launch still fits) every workgroup must be resident at once, and block b lands on XCD b % 8 (32 CUs, one workgroup each): 8 partitions at 17 workgroups, 24 at 9, 48 at 5, 80 at 3

#ifndef CNS_WIDE_POLL_NAP
#define CNS_WIDE_POLL_NAP 1
#endif
// (closed A/B experiments — record fetch behind the first poll, own-row arithmetic in the poll's shadow, the winner's row written
// where its code is a scalar, vote instead of an argmin over the granules, both argmin cascades in one pass, pre-decoded next record,
// dip filter: profiles/r03_ab_*.txt, r02_wide_variants_ab.txt — are resolved in the source; what is still switchable: CNS_WIDE_POLL_NAP,
// CNS_WIDE_BLOCK, CNS_WIDE_NO_FAST_K1, CNS_WIDE_NO_PREFETCH, the CNS_PROF* probe builds and CNS_DEBUG_FLUSH_LOG)
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
#if defined(CNS_PROF) && !defined(CNS_PROF_SCAN_ONLY)   // cycle counters of the -DCNS_PROF build, 32 per PARTITION (tools/prof_wide.py names the slots)
#define WPROF_T(var) const long long var = clock64()
#define WPROF_ADD(slot, a, b) do { if (lane == 0 && hix == 0u) P.prof[(size_t)part * 32 + (slot)] += (u64)((b) - (a)); } while (0)   // (home 0 only)
#define WPROF_CNT(slot) do { if (lane == 0 && hix == 0u) P.prof[(size_t)part * 32 + (slot)] += 1; } while (0)
#else
#define WPROF_T(var)
#define WPROF_ADD(slot, a, b)
#define WPROF_CNT(slot)
#endif

struct WideCtl {                 // one per partition, in HBM, zeroed before every launch; every hot word on its own line
  u32 sup_nex;  u32 pad0[15];    // supervisor -> leader: exchanges consumed
  u32 halt;     u32 pad1[7];     // supervisor -> leader: stop in front of the next job
  u32 homes;    u32 pad5[7];     // home 0 -> the extra homes: home workgroups that work on this partition (0: not decided yet; written once at start)
  u32 cmd_seq, cmd_kind, cmd_job; u32 pad2[13];           // supervisor -> scanners
  u32 scan_stops, scan_pos, scan_nex; u32 pad3[13];       // leader -> supervisor: stopped in front of job scan_pos after scan_nex exchanges
  u32 abort;    u32 pad4[15];    // anyone -> everyone: a device fault was raised
  u32 xcc[32];                   // workgroup m of the partition runs on XCD xcc[m] - 1 (written once at start)
  u32 excl_n; u32 excl_code[15]; // Resume: slots the job at cmd_job must NOT take as a start-now candidate (their exact test failed)
  u32x4 xr[kWRing][kWXrow];      // node_num == 1: A granule of wave w at [w], T granule at [kWSW + w]
  u32x4 xl[kWRing][kWSW * kPMaxK];   // node_num 2..8: entry i of wave w's sorted candidate list at [w * 8 + i]
  u32x4 xd[kWRing][kPMaxK];          // the DECISION of exchange e, written by the scanner wave(s) that own the selected
                                     // node(s): entry i = node i of the selection in cost order (see kWd* below)
  u32x4 xp[kWPRing][kWPG][kWSW];     // the POOL of window w (tag w + 1) at [w % kWPRing]: granule g of wave v at [g][v]
  // what home h tells the others (one 64-byte line each, 16-byte granules, written by its supervisor only):
  //   [0] {wv: all its tasks with gid <= wv have a verdict, wf: ... are final, flush job + 1 (0: none), epoch = stops handled}
  //   [1] {exchanges consumed, stop number at which it drained, gid of its failed task for the flush job (0: none), cause | node_num << 8}
  //   [2] {slot code of that task's first node, job (orig), the job's index in the partition's table + 1 (0: no failed task reported), -}
  u32x4 hx[4][4];
};
// Decision granule {tag e, word, fp64 cost key}: word = payload (code << 6 | node type, < 2^22; 0x3FFFFF: no node)
//   | node_num of the job << 22 | entries in the selection << 26 (lists: min(total, k))
//   | backfill << 30 (node_num == 1: the T argmin won) | halt << 31 (the scanners stopped in front of the job: a void exchange).
// The supervisor reads ONLY these (one 16-byte load per lane < 8, the next exchange's in flight while it posts the task):
// in round 2 it re-derived every decision from the scanners' granules — an argmin cascade over 128 granules, or a k-way
// merge of 64 lists, per job — and was what bounded C4 (profiles/r02_wide_home_counters.txt: 6 299 cycles per job).
// always-on protocol counters, 16 slots per partition behind the cycle counters (cns_debug_get_prof, index 32 * P + 16 * part + x)
// kWsFar: 1 when the workgroups of the partition were NOT all found on one XCD (the census of WideCtl::xcc): its exchange then goes
// through write-through stores and HBM-side coherence instead of that XCD's L2 — ~2.5x slower, never wrong (bench.py reports the sum)
enum { kWsEmpty = 0, kWsBatches = 1, kWsLapWait = 2, kWsStops = 3, kWsFlushes = 4, kWsRedoExcl = 5, kWsSerial = 6, kWsResourceVerdicts = 7, kWsFar = 8,
       kWsWindows = 9, kWsWinJobs = 10, kWsWinDry = 11, kWsPrefetchQuit = 12, kWsHomes = 13 };   // windows (pool exchanges) | jobs decided in them | windows that decided nothing
constexpr u32 kWsSlots = 16;
constexpr u32 kWdPayMask = 0x003FFFFFu, kWdNone = 0x003FFFFFu, kWdBackfill = 1u << 30, kWdHalt = 1u << 31;
constexpr u32 kWdKShift = 22, kWdNfShift = 26;
static_assert(((u32)kWNplMax << kWShift) <= (1u << 16), "a payload (slot code << 6 | node type) fits 22 bits");

// Control words are read at a wave-uniform address; the compiler treats an atomic load as a source of divergence, and
// everything that depends on one — the job position, the whole decoded job — then lives in vector registers behind
// exec-masked control flow.  gld() therefore hands the value back through v_readfirstlane (gld_raw: per-lane addresses, or a
// load that must stay in flight).
__device__ __forceinline__ u32 gld_raw(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 gld(const u32* p) { return uni32(gld_raw(p)); }
__device__ __forceinline__ void gst(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// 16-byte granule traffic.  Loads: buffer_load_dwordx4 sc1 (agent scope: bypasses the CU's L1, served by L2 or beyond); the
// empty asm keeps the compiler from hoisting or merging the polls.  Stores: sc1 (write-through, visible to every XCD) or,
// when all workgroups of the partition were found on ONE XCD (`near`), plain: the line then stays in that XCD's L2, which
// is the point of coherence of its CUs, and the readers' L1-bypassing loads hit it there (~4x less latency per exchange).
__device__ __forceinline__ u32x4 gran_ld(__amdgpu_buffer_rsrc_t rs, u32 byte_off) {
  asm volatile("" ::: "memory");
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 16);
  asm volatile("" ::: "memory");
  return v;
}
__device__ __forceinline__ void gran_st(__amdgpu_buffer_rsrc_t rs, u32 byte_off, u32x4 v, bool near) {
  if (near) __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)byte_off, 0, 0);
  else __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)byte_off, 0, 16);
}
__device__ __forceinline__ void gran_decode(const u32x4& g, u64& c, u32& p) {
  p = g.y & 0x7FFFFFFFu;
  c = ((u64)g.w << 32) | g.z;
  if (p == kWNonePay) { p = kNone; c = ~0ull; }
}
// One lane's share of a node_num == 1 exchange: 32 scanner waves -> 64 granules, lane l holds granule l (A of wave l, or T of
// wave l - 32); 64 scanner waves -> 128 granules, lane l holds the A and the T granule of wave l.
struct XrGran {
  u32x4 a;
#if CNS_WIDE_SPW * CNS_WIDE_WGS > 32
  u32x4 t;
#endif
};
__device__ __forceinline__ XrGran xr_ld(__amdgpu_buffer_rsrc_t rs, u32 xs, u32 lane) {
  XrGran g;
#if CNS_WIDE_SPW * CNS_WIDE_WGS > 32
  g.a = gran_ld(rs, (xs * kWXrow + lane) * 16u);
  g.t = gran_ld(rs, (xs * kWXrow + 64u + lane) * 16u);
#else
  g.a = gran_ld(rs, (xs * kWXrow + (lane & (kWXr - 1u))) * 16u);   // (16 waves: the upper lanes see the lower lanes' granules again)
#endif
  return g;
}
__device__ __forceinline__ bool xr_ready(const XrGran& g, u32 e) {
#if CNS_WIDE_SPW * CNS_WIDE_WGS > 32
  return !__any(g.a.x != e || g.t.x != e);
#else
  return !__any(g.a.x != e);
#endif
}
__device__ __forceinline__ u32 xr_halt(const XrGran& g) { return rl32(g.a.y, 0) >> 31; }   // the leader's A granule
// this lane's entry for the decision: T candidates carry bit 63 (behind every A candidate: cost keys are >= 0)
__device__ __forceinline__ void xr_entry(const XrGran& g, u32 lane, u64& c, u32& p) {
  gran_decode(g.a, c, p);
#if CNS_WIDE_SPW * CNS_WIDE_WGS > 32
  if (p == kNone) {
    gran_decode(g.t, c, p);
    if (p != kNone) c |= 1ull << 63;
  }
#else
  if ((lane & (kWXr - 1u)) >= (u32)kWSW && p != kNone) c |= 1ull << 63;
#endif
}
__device__ __forceinline__ void wide_fault(const KParams& P, WideCtl* ctl, u32 code, u32 a, u32 b, u32 c) {
  if ((threadIdx.x & 63u) == 0) { set_fault(P, code, a, b, c); gst(&ctl->abort, 1u); }
}

// ---------------------------------------------------------------------------------------------------------------------
// Home workgroup: test and commit are SEPARATE work items.  In k_pipe a tester keeps its task from the test to the
// commit and waits in between until every older task has a verdict; on C4 that wait was 18 k cycles per task (a
// node_num = 8 task holds its verdict for ~20 us and the six other testers stand still behind it).  Here the tester
// writes the verdict AND the result (allocations, start, reason) into the task slot and goes on; tasks are RETIRED in
// id order by whichever tester finds the next one ready: claim (one compare-and-swap on `commit`), then — if every
// older task passed (flush_job) — commit from the slot (the node block is read again: nobody else may have touched
// the node in between, the next task on it waits for this one), in parallel with the retirement of younger tasks.
// ---------------------------------------------------------------------------------------------------------------------
struct WideTask {     // PipeTask + what the commit needs
  u32 id;             // task id IN THIS HOME'S RING (1-based, monotone); slot = id % kWTRing
  u32 state;          // PipeTaskState
  u32 ji;             // index in the partition's job table
  u32 kind_k;         // PipeKind | node_num << 8
  u32 gid;            // the task's number in the partition's decision stream (1-based; one home: gid == id)
  u32 code[kPMaxK];   // slots in cost order
  u32 dep[kPMaxK];    // last older task on that node (0: none; kWDepLocal | id: of this ring; else the gid of another home's task)
  u64 cost0[kPMaxK];  // fp64 cost bit pattern of the node before this job
  i64 st, L;          // start time, time limit
  u64 poff;           // first placement record
  u32 reason, orig;
  u32 node[kPMaxK];   // dense node indices
  Res alloc[kPMaxK];  // allocated_res per node
};
#ifdef CNS_PROF_TESTER   // (-DCNS_PROF -DCNS_PROF_HOME_ONLY -DCNS_PROF_TESTER: tester 0's test and commit by phase, in the slots the
#define TPROF_T(var) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const long long var = clock64()   // leader scanner has in the other builds; every probe waits for the loads in flight, so that a phase pays for its own)
#define TPROF_ADD(slot, a, b) do { if (sh.tp && lane == 0) sh.tp[slot] += (u64)((b) - (a)); } while (0)
#define TPROF_CNT(slot) do { if (sh.tp && lane == 0) sh.tp[slot] += 1; } while (0)
#else
#define TPROF_T(var)
#define TPROF_ADD(slot, a, b)
#define TPROF_CNT(slot)
#endif
// The words the waves of a home workgroup poll, in ONE LDS struct: WideHome hands the out-of-line tester routines two pointers.  (With its
// eight pointers of the first multi-home version the aggregate no longer fitted the registers the calling convention gives the arguments
// — 16 in all — and went through scratch memory: every `vld(&sh.w->retired)` a scratch load first, C5 185 -> 235 ms with ONE home.)
struct WideHomeWords {
  u32 posted;       // tasks posted so far
  u32 claim;        // task ids handed to the testers so far
  u32 retired;      // tasks retired so far (claimed for commit / dropped), in id order
  u32 flush_job;    // lowest job index whose task contradicted its prediction (kNone: none)
  u32 abort;
  // several homes per partition (kept by this home's supervisor; one home: allow = 0xFFFFFFFF, homes = 1)
  u32 allow;        // a task of this ring may retire once its gid <= allow: every older task of the OTHER homes has a verdict
  u32 homes;        // home workgroups at work on the partition (> 1: node blocks are written on other CUs too — the testers invalidate their L1)
  u32 wfm[4];       // home g's tasks with gid <= wfm[g] are final (a dependency on one of them is over)
};
struct WideHome {
#ifdef CNS_PROF_TESTER
  u64* tp;
#endif
  WideTask* task;
  WideHomeWords* w;
};
// Everything cached in this CU's L1 is dropped (the next loads come from the XCD's L2, where the other homes' drained stores are).
__device__ __forceinline__ void l1_inv() { asm volatile("buffer_inv sc1" ::: "memory"); }
__device__ __forceinline__ void wide_home_fault(const KParams& P, const WideHome& sh, u32 code, u32 a, u32 b, u32 c) {
  if ((threadIdx.x & 63u) == 0) { set_fault(P, code, a, b, c); vst(&sh.w->abort, 1u); }
}

// Retires the next task if it has a verdict.  Returns true when it made progress (so the caller looks again).
template <bool kW>
__device__ __noinline__ bool wide_retire_one(const KParams* Pg, const WideHome sh, u32 qbeg) {
  const u32 lane = threadIdx.x & 63u;
  const u32 c = vld(&sh.w->retired) + 1u;
  if (c > vld(&sh.w->posted)) return false;
  WideTask* const T = &sh.task[c & (kWTRing - 1)];
  if (vld(&T->id) != c) return false;
  const u32 st0 = vld(&T->state);
  if (st0 < kTsPass) return false;                 // posted, not tested yet
  // several homes: a passing task waits until every older task of the OTHER homes has its verdict too — unless an older job already
  // flushed (then it is dropped below whatever the others say: tasks behind a flush may wait for verdicts that never come).
  // Order: `allow` is read BEFORE the flush word is (re)read below — whoever publishes a watermark past a failed task published the flush first.
  if (st0 == kTsPass && vld(&T->gid) > vld(&sh.w->allow) && vld(&sh.w->flush_job) > vld(&T->ji)) return false;
  u32 won = 0;
  TPROF_T(c0);
  if (lane == 0) won = atomicCAS(&sh.w->retired, c - 1u, c) == c - 1u ? 1u : 0u;
  if (!uni32(won)) return true;                    // another tester took it
  if (st0 != kTsPass) return true;                 // failed / aborted: nothing to commit
  const u32 ji = vld(&T->ji);
  if (vld(&sh.w->flush_job) <= ji) { if (lane == 0) { lds_fence(); vst(&T->state, kTsAborted); } return true; }
  // ---- commit: every older task has a passing verdict ------------------------------------------------------------
  const auto& P = kparams_scalar(Pg);   // (the block's copy in HBM, through scalar loads: select_kernels.hip)
  const GresDev& G = Pg->gres;
  const u32 k = vld(&T->kind_k) >> 8;
  const i64 st = (i64)(((u64)vld((u32*)&T->st + 1) << 32) | vld((u32*)&T->st));
  const i64 L = (i64)(((u64)vld((u32*)&T->L + 1) << 32) | vld((u32*)&T->L));
  const u64 poff = ((u64)vld((u32*)&T->poff + 1) << 32) | vld((u32*)&T->poff);
  const u32 orig = vld(&T->orig), reason = vld(&T->reason);
  NodeHdr* hd = nullptr; NodeHdr h; TlEntry e;
  TPROF_T(c1);
  TPROF_ADD(17, c0, c1); TPROF_CNT(16);            // commits | claim + the task's fields
  if (vld(&sh.w->homes) > 1u) l1_inv();                // (the nodes' previous writers may sit on other CUs; nobody writes them between the test and here)
  for (u32 i = 0; i < k; ++i) {
    const u32 qi = qbeg + vld(&T->code[i]);
    TPROF_T(c2);
    load_block<kW>(P, qi, lane, hd, h, e);
    TPROF_T(c3);
    TPROF_ADD(18, c2, c3);                         // node block (header + map) from L2 / HBM
    u32 rank = 0;  // placement records are listed by ascending node index
    for (u32 mm = 0; mm < k; ++mm) rank += vld(&T->node[mm]) < h.node ? 1u : 0u;
    const u64 c0 = ((u64)vld((u32*)&T->cost0[i] + 1) << 32) | vld((u32*)&T->cost0[i]);
    pipe_commit_node<kW>(P, *Pg, G, &sh.w->abort, hd, h, e, qi, c0, uni_res(narrow<kW>(T->alloc[i])), st, L, orig, poff + rank, lane);
    TPROF_T(c4);
    TPROF_ADD(19, c3, c4);                         // map update + cost + scanner arrays + placement record (incl. the wait for the stores)
  }
  TPROF_T(c5);
  if (lane == 0) { P.o_start[orig] = st; P.o_reason[orig] = (uint8_t)reason; }
  drain_stores();   // later tasks on these nodes, and a tile reload, read what was just written
  if (lane == 0) { lds_fence(); vst(&T->state, kTsCommitted); }
  TPROF_T(c6);
  TPROF_ADD(20, c5, c6);
  return true;
}

// The older task `dep` no longer owns its nodes (committed, or it never will commit).  While waiting the tester helps
// with the retirement (the task it waits for may sit tested-but-uncommitted behind older ones).
template <bool kW>
__device__ __forceinline__ bool wide_wait_dep(const KParams& P, const KParams* Pg, const WideHome& sh, u32 dep, u32 qbeg) {
  if (dep == 0) return true;
  if (!(dep & kWDepLocal)) {
    // a task of ANOTHER home (gid `dep`): over once that home's watermark of final tasks has passed it (this home's supervisor mirrors it)
    const u32 hn = vld(&sh.w->homes);
    const u32* const wf = &sh.w->wfm[(dep - 1u) % (hn ? hn : 1u)];
    for (u32 spin = 0;; ++spin) {
      if (vld(wf) >= dep) return true;
      if (vld(&sh.w->abort)) return false;
      if (spin > kPSpinLimit) { wide_home_fault(P, sh, 20, dep, vld(wf), 0x80000000u | hn); return false; }
      if (!wide_retire_one<kW>(Pg, sh, qbeg)) nap();
    }
  }
  dep &= ~kWDepLocal;
  const WideTask* s = &sh.task[dep & (kWTRing - 1)];
  for (u32 spin = 0;; ++spin) {
    const u32 id = vld(&s->id), st = vld(&s->state);
    if (id != dep || st >= kTsFail) return true;   // slot recycled (=> final) or final
    if (vld(&sh.w->abort)) return false;
    if (spin > kPSpinLimit) { wide_home_fault(P, sh, 20, dep, id, st); return false; }
    if (!wide_retire_one<kW>(Pg, sh, qbeg)) nap();
  }
}

// The exact test of one task (pipe_tester_task without the commit): verdict + result into the slot.
template <bool kW>
__device__ __noinline__ void wide_test_task(const KParams* Pg, const WideHome sh, u32 my, u32 qbeg, bool resv_part, u64 jbase) {
  const u32 lane = threadIdx.x & 63u;
  const auto& P = kparams_scalar(Pg);   // (the block's copy in HBM, through scalar loads: select_kernels.hip)
  const GresDev& G = Pg->gres;
  WideTask* const T = &sh.task[my & (kWTRing - 1)];
  const u32 ji = vld(&T->ji), kind_k = vld(&T->kind_k);
  const u32 kind = kind_k & 0xFFu, k = kind_k >> 8;
  // an older task already contradicted its prediction: this selection was made on a wrong premise
  if (vld(&sh.w->flush_job) <= ji) { if (lane == 0) { lds_fence(); vst(&T->state, kTsAborted); } TPROF_CNT(14); return; }
  TPROF_T(t0);
  // One-node tasks (round 5): the record's load and the node block's loads go out back to back and come back together — the block's address
  // is in the task slot, not in the record — instead of one round trip after the other (load_block's own vmcnt(0) used to sit between them).
  drain_stores();   // (this wave's earlier commit: it may re-read a block it stored to)
  const u32 raw = fetch_job(P, (u64)ji + jbase);
  NodeHdr* hd = nullptr; NodeHdr h; TlEntry e;
  h.len = 0;
  bool early = false;
  const bool multi = vld(&sh.w->homes) > 1u;   // several homes: a node's previous writer may sit on another CU — drop this CU's L1 behind every dependency wait
  if (k == 1 && P.wide_tester_opt != 0u) {
    if (!wide_wait_dep<kW>(P, Pg, sh, vld(&T->dep[0]), qbeg)) return;   // (LDS; a retirement it helps with drains its own stores)
    if (multi) l1_inv();
    load_block<kW, false>(P, qbeg + vld(&T->code[0]), lane, hd, h, e);
    early = true;
  }
  const FastJob F = make_fast_job(P, raw);
  const u32 maxlen = P.max_jobs_per_node;
  TPROF_T(t1);
  bool ok = true;
  // why a verdict contradicts the prediction: 1 the node's map is full (:6194: the reference would have SKIPPED the node),
  // 2 the one start-now candidate fails the exact test (the reference goes on to the next node), 3 a node of a multi-node
  // start fails it, 4 no start inside the window on the res_total nodes (Backfill_ fails: the job gets "Resource")
  u32 cause = 0;
  i64 st = P.now;
  int reason = CNS_REASON_NONE;
  if (k == 1) {
    Res alloc = res_zero();
    const u32 q = qbeg + vld(&T->code[0]);
    if (!early && !wide_wait_dep<kW>(P, Pg, sh, vld(&T->dep[0]), qbeg)) return;
    TPROF_T(t2);
    if (!early) { if (multi) l1_inv(); load_block<kW>(P, q, lane, hd, h, e); }
    TPROF_T(t3);
    if (kind == kPkStart) { TPROF_CNT(0); TPROF_ADD(1, t0, t1); TPROF_ADD(2, t1, t2); TPROF_ADD(3, t2, t3); }   // node_num 1, start now: record | dependency | node block
    ok = h.len < maxlen;                                            // :6194 on the CURRENT map (the tile's length may be stale)
    cause = ok ? 0u : 1u;
    if (ok && kind == kPkStart) {
      ok = fits_now(F.mv, block_window_min<kW>(P, hd, h, e, F.E, lane), h.avail0, alloc, G);
      if (!ok) { cause = 2; record_dip(P, G, q, e, h.len, F.mv, F.E, lane); }
      TPROF_T(t4);
      TPROF_ADD(4, t3, t4);                                         // window minimum + the exact test
    } else if (ok) {
      // backfill on the first node in cost order whose res_total fits (:6335-6368, Backfill_ :6371-6376)
      if (!feasible(F.mv, h.total, alloc, G)) { wide_home_fault(P, sh, 3, F.orig, h.node, 0); return; }
      alloc = uni_res(alloc);
      st = block_next_fit<kW>(P, hd, h, e, alloc, F.L, P.now, lane);
      ok = st != kInf && st - P.now <= P.max_window;                // kAlgoMaxTimeWindow, JobScheduler.h:815
      if (!ok) cause = 4;
      if (ok && st != P.now) reason = later_start_reason(!resv_part && P.first_resv[q] < P.now + F.L, !res_le(alloc, h.avail0));
    }
    // ---- the task that is next to retire commits AT ONCE, from the registers of its test (round 5): every older task has been claimed
    // for its commit (retirement is in id order) and none contradicted its prediction — no verdict through the slot, no claim by another
    // wave, no second load of the node block (nobody else may touch the node: a younger task on it waits for this one).  (Waiting a few
    // hundred cycles for the predecessors' claims so that more tasks take this path was measured and does not pay: profiles/r05_ab_fuse_spin.txt)
    if (ok && P.wide_tester_opt != 0u && h.len <= kTlChunk && vld(&sh.w->retired) + 1u == my && vld(&T->gid) <= vld(&sh.w->allow) && vld(&sh.w->flush_job) > ji) {
      u32 won = 0;
      if (lane == 0) won = atomicCAS(&sh.w->retired, my - 1u, my) == my - 1u ? 1u : 0u;
      if (uni32(won)) {
        const u64 c0 = ((u64)vld((u32*)&T->cost0[0] + 1) << 32) | vld((u32*)&T->cost0[0]);
        pipe_commit_node<kW>(P, *Pg, G, &sh.w->abort, hd, h, e, q, c0, uni_res(alloc), st, F.L, F.orig, F.poff, lane);
        if (lane == 0) { P.o_start[F.orig] = st; P.o_reason[F.orig] = (uint8_t)reason; }
        drain_stores();   // later tasks on this node, and a tile reload, read what was just written
        if (lane == 0) { T->orig = F.orig; lds_fence(); vst(&T->state, kTsCommitted); }
        return;
      }
    }
    if (ok && lane == 0) { T->alloc[0] = uni_res(alloc); T->node[0] = h.node; }
  } else {
    // node_num 2..8, ntasks == node_num: the nodes one after the other (the task is off the sequential chain)
    const Req& v1 = F.mv;  // tpn_min == 1: the minimum view is the one-task view
    bool notle = false, reserved = false;
    // Warm-up of the k node blocks (first 1 KB each: header + 19 entries) in ONE round trip — L1-bypassing loads (sc1), so
    // that nothing stale can be served later: the loop below then takes k L2 hits instead of k dependent HBM misses.
    u32 touch = 0;
    if ((lane >> 3) < k) touch = gld_raw((const u32*)((const char*)hdr_of(P, qbeg + vld(&T->code[lane >> 3])) + (lane & 7u) * 128u));
    for (u32 i = 0; i < k && ok; ++i) {
      const u32 qi = qbeg + vld(&T->code[i]);
      if (!wide_wait_dep<kW>(P, Pg, sh, vld(&T->dep[i]), qbeg)) return;
      if (multi) l1_inv();
      load_block<kW>(P, qi, lane, hd, h, e);
      if (i == 0) asm volatile("" :: "v"(touch));   // (keeps the warm-up loads; they have arrived by now: vmcnt is in order)
      if (h.len >= maxlen) { ok = false; cause = 1; break; }
      Res a = res_zero();
      if (kind == kPkStart) {
        ok = fits_now(v1, block_window_min<kW>(P, hd, h, e, F.E, lane), h.avail0, a, G);
        if (!ok) { cause = 3; record_dip(P, G, qi, e, h.len, v1, F.E, lane); }
      } else {
        if (!feasible(v1, h.total, a, G)) { wide_home_fault(P, sh, 3, F.orig, h.node, 2); return; }   // :6354-6356
        notle = notle || !res_le(a, h.avail0);
        reserved = reserved || (!resv_part && P.first_resv[qi] < P.now + F.L);
      }
      if (lane == 0) { T->alloc[i] = uni_res(a); T->node[i] = h.node; }
    }
    lds_fence();
    if (ok && kind == kPkBackfill) {
      st = earliest_start(P, k, [&](u32 i, i64 t) {
        load_block<kW>(P, qbeg + vld(&T->code[i]), lane, hd, h, e);
        return block_next_fit<kW>(P, hd, h, e, T->alloc[i], F.L, t, lane);
      });
      ok = st != kInf;
      if (!ok) cause = 4;
      if (ok && st != P.now) reason = later_start_reason(reserved, notle);
    }
  }
  // ---- verdict (+ the result the commit needs) ----------------------------------------------------------------
  TPROF_T(t8);
  if (k == 1 && kind != kPkStart) { TPROF_CNT(10); TPROF_ADD(11, t0, t8); }   // node_num 1, backfill: whole test
  if (k != 1) { TPROF_CNT(12); TPROF_ADD(13, t0, t8); }                       // node_num > 1: whole test
  if (!ok) {
    drain_stores();   // (a recorded dip must be in L2 before the flush lets the scanners reload)
    if (lane == 0) { T->reason = cause; T->orig = F.orig; atomicMin(&sh.w->flush_job, ji); lds_fence(); vst(&T->state, kTsFail); }
    return;
  }
  if (lane == 0) {
    T->st = st; T->L = F.L; T->poff = F.poff; T->reason = (u32)reason; T->orig = F.orig;
    lds_fence();
    vst(&T->state, kTsPass);
  }
  TPROF_T(t9);
  TPROF_ADD(5, t8, t9);                                             // verdict + result into the slot
}

// ---------------------------------------------------------------------------------------------------------------------
// k_giant: the serial-only mode of the giant instantiation (k_wide<1, false, kWMemWordsGiant>) with HELPER workgroups
// (KParams::giant_nh > 0, launch_giant).  A partition wider than k_wide's tile or a group wider than k_mem's ordinary masks
// scans every slot of the job's partition per job; on the 448 memory-scanner lanes of the home alone that is ~1.9 ns per slot
// (profiles/r07_giant_partitions.txt).  Here nh workgroups of 512 lanes each own a stripe of the job's slot range (lane gl of the
// helpers: slots rb + gl, rb + gl + 512 nh, ...): per job they evaluate their rows exactly as the memory scanners do (eval_node,
// own-partition tag, exclusive test) and answer with their stripe's lexicographic (cost key, slot) minimum of the start-now set
// and of the res_total set.  The home reduces the answers: that is round 0 of the walk.  The walk goes on in the home alone: its
// memory scanners build their row masks only when a job needs a second candidate (a failed exact test, node_num > 1, ntasks >
// node_num) — the masks do not depend on round 0, so the walk is the one of k_mem, step for step.  Jobs with include / exclude
// lists are scanned by the home itself.
//   hand-off: home tester wave 1 -> helpers: the commits of earlier jobs (plain stores, drained) -> agent-scope release ->
//   GiantCtl::job = seq << 32 | job; helpers: poll (wave 0, bounded) -> acquire -> plain loads of the arrays.  Helper -> home:
//   its answer (agent-scope atomic stores) -> release -> tag = seq; home: poll the nh tags (bounded) -> atomic loads.
// Workgroups land on any XCD: coherence is the agent scope's, not an L2's.  Every workgroup of the launch must be resident
// (the host proves it with the occupancy figure, else k_mem runs); a home that waits for an answer longer than kGiantAnsSpin polls
// raises device fault 43 and scans the job itself (exact; the host re-runs the cycle on k_mem).
constexpr u32 kGiantHelpersMax = 64;           // helper workgroups per partition at most (one answer per lane of the home's tester wave 1)
constexpr u32 kGiantTrip = 4;                  // slots of one helper lane per trip of giant_scan
constexpr u32 kGiantExit = 0xFFFFFFFFu;        // GiantCtl::job >> 32: the home is done
constexpr u32 kGiantAnsSpin = 1u << 22;        // home: polls for the helpers' answers to one job (> 1 s)
constexpr u32 kGiantHelperSpin = 1u << 24;     // helper: polls for the next job (the home may scan a job with node lists alone meanwhile)
struct GiantAns { u64 ac, tc; u32 ap, tp, tag, pad[9]; };   // one 64-byte line per helper
struct GiantCtl { u64 job; u32 pad0[14]; GiantAns ans[kGiantHelpersMax]; };   // one per partition, zeroed before the launch
static_assert(sizeof(GiantAns) == 64 && offsetof(GiantCtl, ans) == 64, "one line per word");

// Slot p (relative to the partition) for the job: (a: start now, b: res_total fits); returns the cost key.  The body of the memory
// scanners' row loop (mem_scan_serial), one slot at a time.
__device__ __forceinline__ u64 giant_eval(const KParams& P, const FastJob& F, u64 tyok, u32 qbeg, u32 p, bool own_range, u32 jt, bool& a, bool& b) {
  const u32 q = qbeg + p;
  NodeSum ns;
  ns.cost = 0; ns.code = p; ns.len = (P.serial_only && P.f_len) ? P.f_len[q] : hdr_of(P, q)->len; ns.type = P.slot_type[q];
  ns.fcpu = P.f_cpu[q]; ns.fmem = P.f_mem[q]; ns.fcnt = P.f_cnt[q];
  const u64 ck = cost_key(P.cost[q]);
  const u32 tg = (P.slot_tag && !own_range) ? (u32)P.slot_tag[q] : jt;
  eval_node(P, F.mv, F.flags, tyok, ns, b, a);
  if (tg != jt) { b = false; a = false; }
  if (F.flags & kJfExclusive) {
    const Res tt = P.type_total[ns.type];
    a = b && ns.fcpu >= clamp_cpu(tt.cpu) && ns.fmem >= mem_mib_ceil(tt.mem) && ns.fcnt == class_counts(tt.gres, P.gres);
  }
  return ck;
}

// Lexicographic (cost key, slot) minima of the start-now set (ac, ap) and the res_total set (tc, tp) over the slots
// [rb + first, rb + rn) with stride `stride`, four slots per trip with every load in flight.
__device__ __forceinline__ void giant_scan(const KParams& P, const FastJob& F, u64 tyok, u32 qbeg, u32 rb, u32 rn, bool own_range, u32 jt,
                                           u32 first, u32 stride, u64& ac, u32& ap, u64& tc, u32& tp) {
  ac = ~0ull; tc = ~0ull; ap = kNone; tp = kNone;
  for (u32 o = first; o < rn; o += kGiantTrip * stride) {
    bool a[kGiantTrip], b[kGiantTrip];
    u64 ck[kGiantTrip];
#pragma unroll
    for (u32 u = 0; u < kGiantTrip; ++u) {
      const u32 off = o + u * stride;
      const bool in = off < rn;
      ck[u] = giant_eval(P, F, tyok, qbeg, rb + (in ? off : 0u), own_range, jt, a[u], b[u]);
      a[u] = a[u] && in; b[u] = b[u] && in;
    }
#pragma unroll
    for (u32 u = 0; u < kGiantTrip; ++u) {   // (slots ascend and `<` is strict: the smallest slot among equal keys)
      if (a[u] && ck[u] < ac) { ac = ck[u]; ap = rb + o + u * stride; }
      if (b[u] && ck[u] < tc) { tc = ck[u]; tp = rb + o + u * stride; }
    }
  }
}

// The helper workgroup h of partition `part`: answers every job the home posts until the home's exit (or kGiantHelperSpin polls).
__device__ __noinline__ void giant_helper(const KParams& P, u32 part, u32 qbeg, u32 nn, u64 jbeg, u32 h, u32 nh,
                                          u64 (*s_wc)[kRed], u32 (*s_wp)[kRed], u64* s_tc, u32* s_tp, u32* s_cmd) {
  GiantCtl* const gc = (GiantCtl*)(P.giant_ctl + (size_t)part * sizeof(GiantCtl));
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = uni32(tid >> 6);
  const u32 stride = nh * (u32)kWBlock, gl = h * (u32)kWBlock + tid;
  if (tid < (u32)kRed) { s_wc[0][tid] = ~0ull; s_wp[0][tid] = kNone; s_tc[tid] = ~0ull; s_tp[tid] = kNone; }
  u32 seen = 0;
  for (;;) {
    if (wave == 0) {
      u64 w = 0;
      u32 sq = kGiantExit;
      for (u32 spin = 0; spin < kGiantHelperSpin; ++spin) {
        w = uni64(__hip_atomic_load(&gc->job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if ((u32)(w >> 32) != seen) { sq = (u32)(w >> 32); break; }
        __builtin_amdgcn_s_sleep(2);
      }
      if (lane == 0) { s_cmd[0] = sq; s_cmd[1] = (u32)w; }
    }
    __syncthreads();
    const u32 sq = s_cmd[0], jl = s_cmd[1];
    __syncthreads();
    if (sq == kGiantExit) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const u32 raw = fetch_job(P, jbeg + jl);
    const FastJob F = make_fast_job(P, raw);
    const u64 tyok = jr64(raw, kJsTyok);
    const bool own_range = P.serial_only && P.slot_tag && P.tag_off;
    const u32 jt = (F.flags >> 8) & 0xFFu;
    u32 rb = 0, rn = nn;
    if (own_range) { const u32 tb = P.tag_base[part] + jt; rb = P.tag_off[tb]; rn = P.tag_off[tb + 1] - rb; }
    u64 ac, tc;
    u32 ap, tp;
    giant_scan(P, F, tyok, qbeg, rb, rn, own_range, jt, gl, stride, ac, ap, tc, tp);
    wave_argmin(ac, ap);
    wave_argmin(tc, tp);
    if (lane == 0) { s_wc[0][wave] = ac; s_wp[0][wave] = ap; s_tc[wave] = tc; s_tp[wave] = tp; }
    __syncthreads();
    if (wave == 0) {
      u64 c1 = s_wc[0][lane & (kRed - 1)], c2 = s_tc[lane & (kRed - 1)];
      u32 p1 = s_wp[0][lane & (kRed - 1)], p2 = s_tp[lane & (kRed - 1)];
      reduce16(c1, p1);
      reduce16(c2, p2);
      if (lane == 0) {
        GiantAns* const an = &gc->ans[h];
        __hip_atomic_store(&an->ac, c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&an->ap, p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&an->tc, c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&an->tp, p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(&an->tag, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    seen = sq;
  }
}

// kWinK: the instantiation that carries the window path ("A WINDOW OF JOBS PER EXCHANGE").  A kernel of its own because the path's mere
// presence costs the single-job loops ~8 % (C4 280 against 258 ms: registers and code layout of one big function,
// profiles/r05_ab_window_code_presence.txt); the engine launches it when a window may hold two jobs or more (KParams::wide_window).
// MW: 64-bit words per memory-scanner lane in each row mask of the serial-only mode (kWMemWords everywhere but in the one instantiation
// that serves groups wider than that: k_wide<1, false, kWMemWordsGiant>, launch_mem).
template <int NPL, bool kWinK = false, u32 MW = kWMemWords>
__global__ __launch_bounds__(kWBlock) void k_wide(const KParams P, const KParams* __restrict__ Pg) {
  const KParams& PG = *Pg;
  constexpr bool kGiantMW = MW == kWMemWordsGiant;
  const u32 gnh = kGiantMW ? P.giant_nh : 0u;  // k_giant: helper workgroups per partition (0: k_mem)
  const u32 nlaunch = P.part_map ? P.launch_parts : P.num_parts;
  // block b runs on XCD b % 8 (observed; speed only): all workgroups of a partition share b % 8
  const u32 bslot = blockIdx.x >> 3;
  const u32 grp = (u32)kWGroup + (P.wide_aux < kWAuxMax ? P.wide_aux : kWAuxMax);   // workgroups per partition of THIS launch
  // (k_giant: the home of partition i is block i, its helper h block (h + 1) * nlaunch + i)
  const u32 pidx = gnh ? blockIdx.x % nlaunch : (bslot / grp) * 8u + (blockIdx.x & 7u);   // position among the partitions of THIS launch
  const u32 m = gnh ? blockIdx.x / nlaunch : bslot % grp;   // 0: home, 1..8: scanner workgroups, behind them: the extra home workgroups (k_giant: 1 + helper)
  const bool home = m == 0u || (m > (u32)kWScanWgs && !gnh);
  const u32 hix = (m > (u32)kWScanWgs && !gnh) ? m - (u32)kWScanWgs : 0u;   // which home (0: the one that talks to the scanners)
  if (pidx >= (P.part_map ? P.launch_parts : P.num_parts)) return;
  const u32 part = P.part_map ? uni32(P.part_map[pidx]) : pidx;   // (a cycle may be split over two launches: KParams::part_map)
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = uni32(tid >> 6);
  // (loads through the pointers of the by-value KParams are FLAT loads, which the compiler treats as sources of divergence:
  // without the readfirstlanes the job position, the decoded job and every branch on them end up in vector registers
  // behind exec-masked control flow)
  const u32 qbeg = uni32(P.part_off[part]);
  const u32 nn = uni32(P.part_off[part + 1]) - qbeg;
  const u64 jbeg = uni64(P.pj_off[part]), jend = uni64(P.pj_off[part + 1]);
  if (jbeg >= jend) return;
  if (P.serial_only && m != 0 && !gnh) return;   // (the home workgroup does everything: see the supervisor; k_giant: and its helpers)
  const bool resv_part = part >= P.num_real_parts;
  if (resv_part) {  // a reservation's scheduler exists only while the reservation is active (JobScheduler.cpp:6643,6754-6759)
    const i64 rs = P.resv_se[2 * (part - P.num_real_parts)], re = P.resv_se[2 * (part - P.num_real_parts) + 1];
    if (!(rs <= P.now && P.now < re)) {
      if (m == 0)
        for (u64 x = jbeg + tid; x < jend; x += kWBlock) {
          const u32 orig = P.jobrec[x * kJobRecDwords + kJrOrig];
          P.o_start[orig] = 0;
          P.o_reason[orig] = CNS_REASON_RESERVATION_NOT_FOUND;
        }
      return;
    }
  }
  const u32 njobs = (u32)(jend - jbeg);
  WideCtl* const ctl = (WideCtl*)(P.wide_ctl + (size_t)part * sizeof(WideCtl));
  // (the descriptors are wave-uniform: built from scalar halves, else every buffer access becomes a waterfall loop)
  // ONE descriptor over both rings (scalar registers are the scarce resource of this kernel): xr at byte 0, xl at kXl
  const u64 xr_addr = uni64((u64)(uintptr_t)&ctl->xr[0][0]);
  constexpr u32 kXl = (u32)(offsetof(WideCtl, xl) - offsetof(WideCtl, xr));
  constexpr u32 kXd = (u32)(offsetof(WideCtl, xd) - offsetof(WideCtl, xr));
  constexpr u32 kXp = (u32)(offsetof(WideCtl, xp) - offsetof(WideCtl, xr));
  constexpr u32 kXh = (u32)(offsetof(WideCtl, hx) - offsetof(WideCtl, xr));
  static_assert(offsetof(WideCtl, xd) == offsetof(WideCtl, xl) + sizeof(ctl->xl) && offsetof(WideCtl, xp) == offsetof(WideCtl, xd) + sizeof(ctl->xd) &&
                offsetof(WideCtl, hx) == offsetof(WideCtl, xp) + sizeof(ctl->xp) && offsetof(WideCtl, hx) % 64 == 0, "one descriptor over the four rings and the homes' granules");
  const __amdgpu_buffer_rsrc_t rs_xr = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)xr_addr, 0, (int)(sizeof(ctl->xr) + sizeof(ctl->xl) + sizeof(ctl->xd) + sizeof(ctl->xp) + sizeof(ctl->hx)), 0x00020000);

  // ---- LDS (the union of what the two kinds of workgroup use) -------------------------------------------------------
  __shared__ i64 s_tytot[CNS_MAX_NODE_TYPES_DEV];    // res_total.cpu per node type (the cost ratio's denominator)
  __shared__ int s_ty_cpu[CNS_MAX_NODE_TYPES_DEV];
  __shared__ u32 s_ty_m16[CNS_MAX_NODE_TYPES_DEV];
  __shared__ u32 s_ty_gn[CNS_MAX_NODE_TYPES_DEV];
  __shared__ u32 s_nme[kMaxNames], s_nmo[kMaxNames];
  // home workgroup
  __shared__ WideTask s_task[kWTRing];
  constexpr bool kLastInLds = NPL <= 4;              // (8 / 16 rows per lane: 128 / 256 KB — in HBM instead, KParams::wide_last)
  __shared__ u32 s_last[kLastInLds ? kWLanes * NPL : 1];   // last task posted on a slot (dependency of the next one)
  u32* const glast = kLastInLds ? nullptr : P.wide_last + (size_t)part * (kWLanes * (u32)kWNplMax);   // (zeroed by the host before the launch)
  __shared__ u32 s_cmd[4];
  __shared__ u32 s_cmd_seq;
  __shared__ WideHomeWords s_hw;
#define s_posted s_hw.posted
#define s_claim s_hw.claim
#define s_retired s_hw.retired
#define s_flush_job s_hw.flush_job
#define s_abort s_hw.abort
#define s_allow s_hw.allow
#define s_homes s_hw.homes
#define s_wfm s_hw.wfm
  __shared__ u64 s_wc[2][kRed];                      // serial mode: the exchange of k_select's sequential protocol
  __shared__ u32 s_wp[2][kRed];
  __shared__ u64 s_tc[kRed];
  __shared__ u32 s_tp[kRed];
  __shared__ int s_flag;
  __shared__ int s_nupd;
  __shared__ UpdRec s_upd[kMaxUpd];
  __shared__ HeapEnt s_heap[kLdsHeap];
  __shared__ JobCtx s_job;

  if (home) {
    if constexpr (kLastInLds)
      for (u32 x = tid; x < kWLanes * NPL; x += kWBlock) s_last[x] = 0;
    if (tid < kWTRing) { s_task[tid].id = 0; s_task[tid].state = kTsFree; }
    if (tid < 4u) s_wfm[tid] = 0;
    if (tid == 0) { s_allow = 0xFFFFFFFFu; s_homes = 1u; }
    if (tid < (u32)kRed) {
      s_wc[0][tid] = ~0ull; s_wc[1][tid] = ~0ull; s_wp[0][tid] = kNone; s_wp[1][tid] = kNone;
      s_tc[tid] = ~0ull; s_tp[tid] = kNone;
    }
    if (tid == 0) { s_cmd_seq = 0; s_posted = 0; s_claim = 0; s_retired = 0; s_flush_job = kNone; s_abort = 0; s_flag = 0; s_nupd = 0; }
  } else {
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
  }
  __syncthreads();
  if constexpr (kGiantMW) {
    if (gnh && m != 0u) { giant_helper(P, part, qbeg, nn, jbeg, m - 1u, gnh, s_wc, s_wp, s_tc, s_tp, s_cmd); return; }
  }
  if (!home && wave >= (u32)kWScanPerWg) {   // scanner workgroups: one wave per SIMD
#if !defined(CNS_WIDE_NO_PREFETCH) && !defined(CNS_PROF)
    // One of the spare waves follows the DECISION ring and touches the node block of every selected node (header + the first entries:
    // 1 KB) with L1-bypassing loads nobody waits for: when a tester of the home workgroup loads the block for the exact test, and again for the
    // commit, it finds it in the XCD's L2 instead of in HBM (+ 1 % when the testers paced the kernel: profiles/r04_ab_prefetch_wave.txt).  Read-only and best-effort: it may lag, skip or resynchronise;
    // it leaves with the kernel's exit command (or an abort, or after a bounded number of idle polls).
    if (m == (u32)kWScanWgs && wave == (u32)kWScanPerWg && !P.slot_block) {
      u32 e = 1, idle = 0, sink = 0;
      for (;;) {
        const u32 xs = (e - 1u) & (kWRing - 1);
        const u32x4 g = gran_ld(rs_xr, kXd + (xs * (u32)kPMaxK + (lane & 7u)) * 16u);
        const u32 tag0 = rl32(g.x, 0);
        if (tag0 == e) {
          idle = 0;
          const u32 hw = rl32(g.y, 0);
          if (!(hw & kWdHalt) && (hw & kWdPayMask) != kWdNone) {
            const u32 k = (hw >> kWdKShift) & 15u, en = lane >> 3;   // lane l: line (l & 7) of the block of entry (l >> 3)
            const u32 tg = (u32)__builtin_amdgcn_ds_bpermute((int)(en * 4u), (int)g.x);
            const u32 py = (u32)__builtin_amdgcn_ds_bpermute((int)(en * 4u), (int)g.y);
            if (en < k && tg == e && (py & kWdPayMask) != kWdNone) {
              const char* const line = (const char*)hdr_raw(P, qbeg + ((py & kWdPayMask) >> 6)) + (lane & 7u) * 128u;
              sink = gld_raw((const u32*)line);   // (an L1-bypassing load the compiler tracks: round 4's inline asm wrote a register behind its back)
            }
          }
          ++e;
          continue;
        }
        if ((int)(tag0 - e) > 0) { e = tag0; continue; }   // lapped by the ring: resynchronise on what is there
        if ((++idle & 31u) == 0u) {
          if (gld(&ctl->abort) || gld(&ctl->cmd_kind) == (u32)kPcExit) break;
          if (idle > (1u << 22)) {   // (a long serial job: the ring stood still; counted, so that a launch without its prefetcher shows)
            if (lane == 0) P.prof[(size_t)P.num_parts * 32 + (size_t)part * kWsSlots + kWsPrefetchQuit] = 1;
            break;
          }
        }
        __builtin_amdgcn_s_sleep(16);
      }
      asm volatile("" : : "v"(sink) : "memory");   // (keeps the last load: nothing else reads it)
    }
#endif
    return;
  }
  // ---- placement census: are the 9 workgroups of this partition on one XCD (then its L2 carries the exchange)? ----------
  bool near = false;
  if (!P.serial_only) {
    const u32 my_xcc = (u32)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 15u;   // HW_REG_XCC_ID[3:0]
    if (wave == 0 && lane == 0) gst(&ctl->xcc[m], my_xcc + 1u);
    u32 v = my_xcc + 1u;
    for (u32 spin = 0; spin < (1u << 20); ++spin) {
      if (lane < grp) v = gld_raw(&ctl->xcc[lane]);
      if (!__any(v == 0u)) break;
      __builtin_amdgcn_s_sleep(8);
    }
    near = !__any(v != my_xcc + 1u);   // (a workgroup that never reported leaves v == 0 somewhere: far mode, still correct)
  }

  if (home && wave == 0) {
    // =============================================================================================
    // SUPERVISOR (home workgroups, wave 0)
    // =============================================================================================
    // How many homes work on this partition: home 0 decides (all workgroups on one XCD, the last-task table in LDS, at least one extra home
    // in the launch) and tells the others, which leave at once when they are not wanted.
    u32 Hx = 1;
    if (hix == 0u) {
      if (near && kLastInLds && !P.serial_only && grp > (u32)kWGroup) Hx = 1u + (grp - (u32)kWGroup);
      if (lane == 0) gst(&ctl->homes, Hx);
    } else {
      u32 hv = 0;
      for (u32 spin = 0; spin < (1u << 22); ++spin) {
        hv = gld(&ctl->homes);
        if (hv != 0u || gld(&ctl->abort)) break;
        __builtin_amdgcn_s_sleep(8);
      }
      Hx = hv;
      if (hix >= Hx) {   // not wanted (or home 0 never said): the testers leave with the exit command
        if (lane == 0) { vst(&s_cmd[0], (u32)kPcExit); vst(&s_cmd[1], 0u); lds_fence(); vst(&s_cmd_seq, 1u); }
        return;
      }
    }
    const u32 H = Hx;   // (const: the out-of-line serial_job captures it by reference — a variable would live in scratch)
    if (lane == 0) vst(&s_homes, H);
    int par = 0;
    WorkerShared sh;
    sh.wc = s_wc; sh.wp = s_wp; sh.flag = &s_flag; sh.nupd = &s_nupd; sh.upd = s_upd; sh.heap = s_heap; sh.part = part;
    HeapEnt* const gheap = P.heap + qbeg + part;
    WideHome psh;
    psh.task = s_task; psh.w = &s_hw;
#ifdef CNS_PROF_TESTER
    psh.tp = nullptr;
#endif
    u32 lseq = 0;         // commands posted to the tester waves (LDS)
    u32 gseq = 0;         // home 0: commands posted to the scanner workgroups (HBM); the other homes: the last one they followed
    u32 nposted = 0;      // tasks posted into THIS ring
    u32 gid_seen = 0;     // tasks of the decision stream numbered so far (every home counts alike; one home: == nposted)
    u32 epoch = 0;        // stops handled so far: a home's flush word counts in the epoch it carries
    u32 sup_pos = 0;      // next job whose decision is to be consumed
    u32 sup_nex = 0;      // next exchange to be consumed (its tag is sup_nex + 1)
    // several homes: this ring's watermarks, what was last exported, and what the other homes last said
    u32 lvf = 0, lff = 0;                                   // ids of this ring up to which every task has a verdict / is final
    u32 ex_wv = 0, ex_wf = 0, ex_fl = 0, ex_ep = 0;         // granule 0 as last written
    u32 ex_sn = 0, my_drained = 0, my_fgid = 0, my_fck = 0; // granule 1 as last written / to be written
    u32 o_supnex[kWHomesMax], o_drained[kWHomesMax];
#pragma unroll
    for (u32 g = 0; g < kWHomesMax; ++g) { o_supnex[g] = 0; o_drained[g] = 0; }
    u32 pub_supnex = 0;   // home 0: what the leader scanner was last told (the least of all homes)

    auto post_lcmd = [&](u32 kind, u32 job) __attribute__((always_inline)) {
      ++lseq;
      if (lane == 0) { vst(&s_cmd[0], kind); vst(&s_cmd[1], job); lds_fence(); vst(&s_cmd_seq, lseq); }
    };
    auto post_gcmd = [&](u32 kind, u32 job) __attribute__((always_inline)) {
      ++gseq;
      if (lane == 0) { gst(&ctl->cmd_kind, kind); gst(&ctl->cmd_job, job); }
      vm_drain();
      if (lane == 0) gst(&ctl->cmd_seq, gseq);
    };
    // ---- several homes: what the others say -> this home's LDS; this ring's watermarks -> the others ------------------------------------
    // (called wherever the supervisor may wait: a home that stood still without it would starve the others of the watermarks they wait for)
    auto house_ld = [&]() __attribute__((always_inline)) -> u32x4 { return gran_ld(rs_xr, kXh + (lane & 15u) * 16u); };   // lane l: granule (l & 3) of home (l >> 2)
    auto house_apply = [&](const u32x4& gh) __attribute__((always_inline)) {
      u32 allow = 0xFFFFFFFFu, fmin = kNone;
#pragma unroll
      for (u32 g = 0; g < kWHomesMax; ++g)
        if (g < H && g != hix) {
          const u32 wv = rl32(gh.x, 4u * g), wf = rl32(gh.y, 4u * g), fl = rl32(gh.z, 4u * g), ep = rl32(gh.w, 4u * g);
          o_supnex[g] = rl32(gh.x, 4u * g + 1u);
          o_drained[g] = rl32(gh.y, 4u * g + 1u);
          const u32 d = (hix + H - g) % H;         // behind a gid of home g, this home's next gid is d further on
          const u32 a = wv > 0xFFFFFFFFu - d ? 0xFFFFFFFFu : wv + d;
          allow = a < allow ? a : allow;
          if (ep == epoch && fl != 0u && fl - 1u < fmin) fmin = fl - 1u;
          if (lane == 0) vst(&s_wfm[g], wf);
        }
      if (lane == 0 && fmin < vld(&s_flush_job)) atomicMin(&s_flush_job, fmin);
      lds_fence();   // (the flush word before the watermark: a tester reads them in the other order)
      if (lane == 0) vst(&s_allow, allow);
      // this ring: how far every task has a verdict / is final (lane l looks at the task l behind the frontier)
      const u32 ret = vld(&s_retired);
      lvf = ret > lvf ? ret : lvf;
      const u32 ev = lvf + 1u + lane, ef = lff + 1u + lane;
      const WideTask* const tv = &s_task[ev & (kWTRing - 1)];
      const WideTask* const tf = &s_task[ef & (kWTRing - 1)];
      const bool okv = ev <= nposted && (vld(&tv->id) != ev || vld(&tv->state) >= kTsPass);
      const bool okf = ef <= nposted && (vld(&tf->id) != ef || vld(&tf->state) >= kTsFail);
      const u64 bv = ~__ballot(okv), bf = ~__ballot(okf);
      lvf += bv ? (u32)__builtin_ctzll(bv) : 64u;
      lff += bf ? (u32)__builtin_ctzll(bf) : 64u;
      const u32 fl = vld(&s_flush_job);   // (read AFTER the states: a failed task writes the flush word before its state)
      const u32 wv = lvf >= nposted ? gid_seen : vld(&s_task[(lvf + 1u) & (kWTRing - 1)].gid) - 1u;
      const u32 wf = lff >= nposted ? gid_seen : vld(&s_task[(lff + 1u) & (kWTRing - 1)].gid) - 1u;
      const u32 fe = fl == kNone ? 0u : fl + 1u;
      if (wv != ex_wv || wf != ex_wf || fe != ex_fl || epoch != ex_ep) {
        ex_wv = wv; ex_wf = wf; ex_fl = fe; ex_ep = epoch;
        if (lane == 0) {
          u32x4 v;
          v.x = wv; v.y = wf; v.z = fe; v.w = epoch;
          gran_st(rs_xr, kXh + (hix * 4u) * 16u, v, true);
        }
      }
    };
    auto house = [&]() __attribute__((always_inline)) { if (H > 1u) { const u32x4 gh = house_ld(); house_apply(gh); } };
    auto export_g1 = [&]() __attribute__((always_inline)) {   // {exchanges consumed, the stop at which this home drained, its failed task: gid, cause | node_num << 8}
      if (lane == 0) {
        u32x4 v;
        v.x = sup_nex; v.y = my_drained; v.z = my_fgid; v.w = my_fck;
        gran_st(rs_xr, kXh + (hix * 4u + 1u) * 16u, v, true);
      }
      ex_sn = sup_nex;
    };
    // what the leader scanner may overwrite in the rings: what EVERY home has consumed
    auto publish_supnex = [&]() __attribute__((always_inline)) {
      if (hix == 0u) {
        u32 mn = sup_nex;
#pragma unroll
        for (u32 g = 1; g < kWHomesMax; ++g)
          if (g < H) mn = o_supnex[g] < mn ? o_supnex[g] : mn;
        if (mn != pub_supnex) { pub_supnex = mn; if (lane == 0) gst(&ctl->sup_nex, mn); }
      } else if (sup_nex != ex_sn) export_g1();
    };
    auto drain = [&]() __attribute__((always_inline)) -> bool {  // every posted task is final
      for (u32 spin = 0;; ++spin) {
        bool ok = true;
        if (lane < kWTRing && nposted > lane) {
          const u32 e = nposted - lane;
          const WideTask* s = &s_task[e & (kWTRing - 1)];
          ok = vld(&s->id) != e || vld(&s->state) >= kTsFail;
        }
        if (!__any(!ok) && vld(&s_retired) == nposted) return true;   // (every task retired in order, every commit finished)
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { wide_home_fault(P, psh, 24, nposted, vld(&s_retired), 0); return false; }
        if (H > 1u) {
          house();
          if ((spin & 63u) == 63u && gld(&ctl->abort)) { if (lane == 0) vst(&s_abort, 1u); return false; }
        }
        nap();
      }
    };
    auto slot_free = [&](u32 id) __attribute__((always_inline)) -> bool {  // the ring slot of task `id` can be reused
      const WideTask* s = &s_task[id & (kWTRing - 1)];
      for (u32 spin = 0;; ++spin) {
        const u32 st = vld(&s->state);
        if ((st == kTsFree || st >= kTsFail) && id <= vld(&s_retired) + kWTRing) return true;   // final AND retired (the retirement never skips an id)
        if (vld(&s_abort)) return false;
        if (spin > kPSpinLimit) { wide_home_fault(P, psh, 25, id, st, vld(&s_retired)); return false; }
        if (H > 1u) {
          house();
          if ((spin & 63u) == 63u && gld(&ctl->abort)) { if (lane == 0) vst(&s_abort, 1u); return false; }
        }
        nap();
      }
    };
    // One job through k_select's sequential protocol, inside the home workgroup: the testers are its memory scanners.
    auto serial_job = [&](u32 jl) -> bool {
      if (H > 1u) l1_inv();   // (it reads node blocks and arrays that other homes committed; all of them have drained)
      post_lcmd(kPcSerial, jl);
      const u32 raw = fetch_job(P, jbeg + jl);
      job_to_lds(PG, jbeg + jl, raw, &s_job);
      wg_barrier();  // S0
      wg_barrier();  // B1 (round 0): A and T argmins published by the memory scanners
      u64 wc = s_wc[par][lane & (kRed - 1)];
      u32 wcode = s_wp[par][lane & (kRed - 1)];
      u64 tc = s_tc[lane & (kRed - 1)];
      u32 tcode = s_tp[lane & (kRed - 1)];
      reduce16(wc, wcode);
      reduce16(tc, tcode);
      par ^= 1;
      wc = uni64(wc); wcode = uni32(wcode); tc = uni64(tc); tcode = uni32(tcode);
      par = worker_job_slow<1024, false>(PG, sh, &s_job, par, wc, wcode, tc, tcode, qbeg, gheap);
      drain_stores();
      wg_barrier();  // S1
      return !vld(&s_abort);
    };

    if (P.serial_only) {
      // ---- the whole queue through the sequential protocol (k_select's general path with MEMORY scanners): groups of partitions
      // that share nodes and do not fit k_select's register tile (an "ALL" partition over a large cluster,
      // JobScheduler.cpp:6585-6617).  One job at a time; every tester wave scans its rows of the committed HBM arrays per round.
      u32 n_ser = 0;
      for (u32 jl = 0; jl < njobs; ++jl) {
        if (!serial_job(jl)) break;
        ++n_ser;
      }
      if (vld(&s_abort) && lane == 0) gst(&ctl->abort, 1u);
      if (gnh && lane == 0)   // k_giant: the helpers leave
        __hip_atomic_store(&((GiantCtl*)(P.giant_ctl + (size_t)part * sizeof(GiantCtl)))->job, (u64)kGiantExit << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0) P.prof[(size_t)P.num_parts * 32 + (size_t)part * kWsSlots + kWsSerial] = n_ser;
      post_lcmd(kPcExit, 0);
      return;
    }
    u32 stops_seen = 0;
    bool halt_sent = false;
    u32 idle = 0;
    u32 n_empty = 0, n_batch = 0;  // production counters (registers; written once at the end): who waits for whom ...
    u32 n_stops = 0, n_flush = 0, n_redo = 0, n_serial = 0, n_resv = 0;   // ... and how often the chain was broken, and how it was mended
    u32 excl_job = kNone, excl_cnt = 0;   // start-now candidates of job excl_job whose exact test failed so far
    WPROF_T(loop0);
    for (;;) {
      if (vld(&s_abort)) { if (lane == 0) gst(&ctl->abort, 1u); break; }
      const u32 fjm = vld(&s_flush_job);
      const bool flushing = fjm != kNone;
      if (hix == 0u && flushing && !halt_sent) { if (lane == 0) gst(&ctl->halt, 1u); halt_sent = true; }
      if (sup_pos < njobs) {
        // ---- the decisions of the next kWin exchanges in ONE look: lane l holds entry (l & 7) of exchange sup_nex + (l >> 3).
        // Everything the supervisor needs of a decided job is in its decision granules (node_num included), so this load is
        // the only global access of the loop: as many consecutive ready exchanges as the window holds are turned into tasks
        // from registers (round 2: one exchange per iteration, ~5 k cycles each — a record fetch, 128 granules, an argmin
        // cascade or a k-way merge, and an L2 round trip between any two of them; profiles/r02_wide_home_counters.txt).
        constexpr u32 kWin = 64u / (u32)kPMaxK;
        const u32 wi = lane >> 3, en = lane & 7u;
        const u32x4 g = gran_ld(rs_xr, kXd + ((((sup_nex + wi) & (kWRing - 1)) * (u32)kPMaxK) + en) * 16u);
        if (H > 1u) { const u32x4 gh = house_ld(); house_apply(gh); }   // (the homes' granules travel with the decisions: one round trip per look)
        const u64 tagok = __ballot(g.x == sup_nex + wi + 1u);
        u32 done = 0;                  // exchanges of the window consumed so far
        bool progress = false;
        WPROF_T(w0);
        // ---- a RUN of one-node decisions is posted in ONE pass (round 5): the scanners' windows decide up to 16 jobs in a burst, and one task
        // at a time — slot check, dependency table, fields, fence, state, fence, counter: six LDS round trips each, ~2 500 cycles — the
        // supervisor paced the whole pipeline (profiles/r05_home_counters_windows_on_off.txt).  Lane 8 w posts the task of exchange w: the
        // slot checks, the dependency reads and the field writes of the run go out together; a node that appears twice in the run chains
        // through the task ids directly, and only its last task writes the dependency table.  (One home only: with several, a supervisor
        // posts every H-th task of the stream and the pass below is short enough.)
#ifndef CNS_WIDE_NO_BATCH_POST
        if constexpr (kLastInLds) {
          if (H == 1u && !flushing && sup_pos < njobs && P.wide_batch_post != 0u) {
            const u32 hwv = g.y;
            const bool smp = en == 0u && g.x == sup_nex + wi + 1u && !(hwv & kWdHalt) && ((hwv >> kWdKShift) & 15u) == 1u && (hwv & kWdPayMask) != kWdNone;
            const u64 sm = __ballot(smp);
            u32 nrun = 0;
            while (nrun < kWin && ((sm >> (8u * nrun)) & 1ull)) ++nrun;
            if (nrun > njobs - sup_pos) nrun = njobs - sup_pos;
            if (nrun >= 2u) {
              const u32 idw = nposted + 1u + wi;
              WideTask* const Tw = &s_task[idw & (kWTRing - 1)];
              const u32 stw = vld(&Tw->state), ret = vld(&s_retired);
              const bool fr = (stw == kTsFree || stw >= kTsFail) && idw <= ret + kWTRing;   // final AND retired (slot_free)
              const u64 fm = __ballot(en == 0u && wi < nrun && fr);
              u32 np = 0;
              while (np < nrun && ((fm >> (8u * np)) & 1ull)) ++np;
              if (np >= 2u) {
                const bool act = en == 0u && wi < np;
                const u32 code = act ? (hwv & kWdPayMask) >> 6 : 0u;
                u32 dep = s_last[code];
                bool last = act;
                for (u32 w2 = 0; w2 < np; ++w2) {
                  const u32 c2 = rl32(code, 8u * w2);
                  if (act && w2 < wi && c2 == code) dep = kWDepLocal | (nposted + 1u + w2);   // (ascending: the latest earlier task on the node)
                  if (act && w2 > wi && c2 == code) last = false;
                }
                if (last) s_last[code] = kWDepLocal | idw;
                if (act) {
                  Tw->code[0] = code;
                  Tw->cost0[0] = ((u64)g.w << 32) | g.z;
                  Tw->dep[0] = dep;
                  Tw->ji = sup_pos + wi; Tw->kind_k = ((hwv & kWdBackfill) ? (u32)kPkBackfill : (u32)kPkStart) | (1u << 8); Tw->gid = idw; Tw->id = idw;
                }
                lds_fence();
                if (act) vst(&Tw->state, kTsPosted);
                lds_fence();
                if (lane == 0) vst(&s_posted, nposted + np);
                nposted += np; gid_seen += np; sup_pos += np; done = np; progress = true;
              }
            }
          }
        }
#endif
        while (done < kWin && sup_pos < njobs) {
          if (!((tagok >> (8u * done)) & 1ull)) break;           // the next exchange has no decision yet
          const u32 hw = rl32(g.y, 8u * done);
          const u32 k = (hw >> kWdKShift) & 15u, nf = (hw >> kWdNfShift) & 15u;
          if (hw & kWdHalt) {                                    // a void exchange: the scanners stopped in front of this job
            ++done; progress = true;
            continue;
          }
          u32 sel = done, used = 1, kind = kPkFail, nfound = 0;  // exchange that holds the selection / exchanges of this job
          const bool none = (hw & kWdPayMask) == kWdNone;
          if (k == 1) {
            if (!none) { nfound = 1; kind = (hw & kWdBackfill) ? (u32)kPkBackfill : (u32)kPkStart; }
          } else if (!none && nf == k) {
            if ((((tagok >> (8u * done)) & 0xFFull) & ((1ull << k) - 1ull)) != ((1ull << k) - 1ull)) break;   // entries still on their way
            nfound = k; kind = kPkStart;
          } else {
            // fewer than k nodes can start it now: the res_total lists follow in the NEXT exchange (never a halt)
            if (done + 1u >= kWin) break;                        // its decision is outside this window: next look
            if (!((tagok >> (8u * (done + 1u))) & 1ull)) break;
            const u32 hw2 = rl32(g.y, 8u * (done + 1u));
            used = 2;
            if ((hw2 & kWdPayMask) != kWdNone && ((hw2 >> kWdNfShift) & 15u) == k) {
              if ((((tagok >> (8u * (done + 1u))) & 0xFFull) & ((1ull << k) - 1ull)) != ((1ull << k) - 1ull)) break;
              nfound = k; kind = kPkBackfill; sel = done + 1u;
            }                                                    // else: not even k nodes fit res_total -> "Resource"
          }
          // Every decision that names its k nodes is a task of the stream, numbered alike by every home — also behind a flush, where
          // nobody posts it (the numbering must not depend on WHEN a home learns of the flush).  A job BEHIND the flushing one is redone
          // anyway; a job in front of it is posted as always (a home may still be in front of a flush that another one found).
          const bool worthy = nfound == k;
          const u32 gid = gid_seen + 1u;
          const bool own = H == 1u || (gid - 1u) % H == hix;
          if (!(flushing && sup_pos >= fjm)) {
            if (!worthy) {
              // not even k nodes whose res_total fits: "Resource" (:6335-6343, :6768); nothing changes
              if (hix == 0u) {
                const u32 orig = uni32(P.jobrec[(jbeg + sup_pos) * kJobRecDwords + kJrOrig]);
                if (lane == 0) { P.o_start[orig] = 0; P.o_reason[orig] = CNS_REASON_RESOURCE; }
              }
            } else if (own) {
              const u32 id = nposted + 1;
              WPROF_T(f0);
              if (!slot_free(id)) break;
              WPROF_T(f1);
              WPROF_ADD(23, f0, f1);   // supervisor: waiting for a free task slot (the testers are behind)
              WideTask* const T = &s_task[id & (kWTRing - 1)];
              if (wi == sel && en < k) {
                const u32 code = (g.y & kWdPayMask) >> 6;
                T->code[en] = code;
                T->cost0[en] = ((u64)g.w << 32) | g.z;
                if constexpr (kLastInLds) { T->dep[en] = s_last[code]; s_last[code] = kWDepLocal | id; }
                else { T->dep[en] = glast[code]; glast[code] = kWDepLocal | id; }   // (this wave alone reads and writes the table)
              }
              if (lane == 0) {
                T->ji = sup_pos; T->kind_k = kind | (k << 8); T->gid = gid; T->id = id;
                lds_fence();
                vst(&T->state, kTsPosted);
                lds_fence();
                vst(&s_posted, id);
              }
              nposted = id;
            } else {
              // another home's task: only the dependency table hears of it (the next task on one of its nodes waits for that home's watermark)
              if constexpr (kLastInLds) {
                if (wi == sel && en < k) s_last[(g.y & kWdPayMask) >> 6] = gid;
              }
            }
          }
          if (worthy) gid_seen = gid;
          done += used;
          ++sup_pos;
          progress = true;
          WPROF_CNT(24);
        }
        if (vld(&s_abort)) continue;
        if (progress) {
          idle = 0;
          ++n_batch;
          sup_nex += done;
          publish_supnex();
          WPROF_T(w1);
          WPROF_ADD(22, w0, w1);   // supervisor: decisions -> tasks (incl. the slot waits)
          continue;
        }
      } else house();
      ++n_empty;                   // supervisor: looks that found nothing to consume (always counted: register, written once at the end)
      if (H > 1u) publish_supnex();   // (home 0: another home may have caught up)
      // ---- nothing to consume: did the scanners stop? ---------------------------------------------------------------
      const u32 st = gld(&ctl->scan_stops);
      if (st != stops_seen) {
        vm_drain();
        const u32 spos = gld(&ctl->scan_pos), snex = gld(&ctl->scan_nex);
        if (snex == sup_nex) {
          if (spos != sup_pos) { wide_fault(P, ctl, 27, spos, sup_pos, sup_nex); if (lane == 0) vst(&s_abort, 1u); continue; }
          stops_seen = st;
          idle = 0;
          if (!drain()) continue;
          // ---- several homes: every home has drained its own ring; the others report and wait for home 0's command --------------
          // (a home's LAST words of the epoch — the flush of a task that failed just before the ring ran dry — must be out before it says
          // "drained": home 0 takes the least flush job of all homes once everyone has said so)
          if (H > 1u) { house(); vm_drain(); }
          if (H > 1u && hix == 0u) {
            bool all = false;
            for (u32 spin = 0;; ++spin) {
              house();
              all = true;
#pragma unroll
              for (u32 g = 1; g < kWHomesMax; ++g)
                if (g < H && o_drained[g] != st) all = false;
              if (all) break;
              if ((spin & 15u) == 15u && (vld(&s_abort) || gld(&ctl->abort))) break;
              if (spin > kWCmdSpinLimit) { wide_fault(P, ctl, 41, st, o_drained[kWHomesMax - 1u], H); break; }
              __builtin_amdgcn_s_sleep(4);
            }
            if (!all) { if (lane == 0) vst(&s_abort, 1u); continue; }
            house();   // (granules 0 and 1 of a home are separate 16-byte units: the flush words as they stand AFTER every home reported)
          }
          const u32 fj = vld(&s_flush_job);   // (several homes: the least over all of them — the mirror took theirs in)
          // the failed task is still in a ring (nothing was posted since): why did it fail?
          u32 fcause = 0, fcode = kNone, forig = 0, fk = 0, fgid = 0;
          if (fj != kNone) {
            const WideTask* s = &s_task[lane & (kWTRing - 1)];
            const u32 sid_ = vld(&s->id);
            const bool mine = sid_ != 0 && vld(&s->ji) == fj && vld(&s->state) == kTsFail;
            const u32 newest = wave_umax32(mine ? sid_ : 0u);   // (an earlier attempt at the same job may still sit in the ring)
            const u64 bal = __ballot(mine && sid_ == newest);
            if (newest != 0 && bal) {
              const u32 src = (u32)__builtin_ctzll(bal);
              const WideTask* f = &s_task[src];
              fcause = vld(&f->reason); fcode = vld(&f->code[0]); forig = vld(&f->orig); fk = vld(&f->kind_k) >> 8; fgid = vld(&f->gid);
            }
          }
          if (hix != 0u) {
            // ---- an extra home: report (the failed task, if it is in this ring), then follow home 0's command to the scanners ----
            if (lane == 0) {
              u32x4 v;
              v.x = fcode; v.y = forig; v.z = fgid != 0u ? fj + 1u : 0u; v.w = 0;   // (WHICH job the report is about: this home's flush word may still fall — another home's older failure — after the scan)
              gran_st(rs_xr, kXh + (hix * 4u + 2u) * 16u, v, true);
            }
            vm_drain();
            my_drained = st; my_fgid = fgid; my_fck = fcause | (fk << 8);
            export_g1();
            u32 kind = kPcExit, cj = 0;
            bool got = false;
            for (u32 spin = 0;; ++spin) {
              const u32 cs = gld(&ctl->cmd_seq);
              if (cs != gseq) {
                vm_drain();
                kind = gld(&ctl->cmd_kind); cj = gld(&ctl->cmd_job);
                gseq = cs; got = true;
                break;
              }
              house();
              if ((spin & 15u) == 15u && (vld(&s_abort) || gld(&ctl->abort))) break;
              if (spin > kWCmdSpinLimit) { wide_fault(P, ctl, 42, st, hix, 0); break; }
              __builtin_amdgcn_s_sleep(8);
            }
            if (!got || kind != kPcResume) break;   // exit / abort
            if (lane == 0) vst(&s_flush_job, kNone);
            lds_fence();
            epoch = st;
            sup_pos = cj;
            continue;
          }
          if (H > 1u && fj != kNone) {
            // whose ring holds the failed task of job fj?  The newest attempt of them all (a redone job may have failed in another home before)
            const u32x4 gh = house_ld();
#pragma unroll
            for (u32 g = 1; g < kWHomesMax; ++g)
              if (g < H) {
                const u32 fl = rl32(gh.z, 4u * g + 2u), og = rl32(gh.z, 4u * g + 1u), ock = rl32(gh.w, 4u * g + 1u);
                if (fl == fj + 1u && og > fgid) { fgid = og; fcause = ock & 0xFFu; fk = ock >> 8; fcode = rl32(gh.x, 4u * g + 2u); forig = rl32(gh.y, 4u * g + 2u); }
              }
          }
          if (lane == 0) vst(&s_flush_job, kNone);
          epoch = st;
          if (halt_sent) { if (lane == 0) gst(&ctl->halt, 0u); halt_sent = false; }
          lds_fence();
          u32 resume;
          u32 nexcl = 0;                // exclusions that go with the Resume command
          WPROF_T(sj0);
          WPROF_CNT(25);
          ++n_stops;
          if (fj != kNone) {            // a prediction failed at job fj: redo it exactly on the committed state
            WPROF_CNT(29);
            ++n_flush;
#ifdef CNS_DEBUG_FLUSH_LOG   // diagnostics: the first 2048 flushes of partition 0 as (job, cause << 24 | slot code)
            if (part == 0 && n_flush <= 2048 && lane == 0) P.prof[(size_t)P.num_parts * 48 + (n_flush - 1)] = ((u64)forig << 32) | (fcause << 24) | (fcode & 0xFFFFFFu);
#endif
            if (fcause == 4) {
              // Backfill_ fails on exactly these nodes in the reference too (no wave could start the job now: the tile
              // holds upper bounds; the res_total nodes and their costs are exact): "Resource", nothing changes (:6768)
              if (lane == 0) { P.o_start[forig] = 0; P.o_reason[forig] = CNS_REASON_RESOURCE; }
              drain_stores();
              resume = fj + 1;
              excl_job = kNone;
              ++n_resv;
            } else if (fcause == 2 && fk == 1 && (excl_job != fj || excl_cnt < 15u)) {
              // the reference walks on to the next node in cost order: the scanners redo the job without this candidate
              if (excl_job != fj) { excl_job = fj; excl_cnt = 0; }
              if (lane == 0) gst(&ctl->excl_code[excl_cnt], fcode);
              ++excl_cnt;
              nexcl = excl_cnt;
              resume = fj;
              ++n_redo;
            } else {
              if (!serial_job(fj)) continue;
              resume = fj + 1;
              excl_job = kNone;
              ++n_serial;
            }
          } else if (sup_pos >= njobs) {
            break;                      // the end: everything is committed
          } else {                      // a job outside the pipelined shapes
            if (!serial_job(sup_pos)) continue;
            resume = sup_pos + 1;
            ++n_serial;
          }
          sup_pos = resume;
          // what this workgroup committed (plain stores, all drained) -> the other workgroups, then the command
          if (lane == 0) gst(&ctl->excl_n, nexcl);
          // (one XCD: every committer drained its plain stores into the shared L2 before its task was marked committed, and the
          // scanners reload with L1-bypassing loads — no write-back / invalidate needed; across XCDs: release here, acquire there)
          if (!near) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          vm_drain();
          post_gcmd(kPcResume, resume);
          WPROF_T(sj1);
          WPROF_ADD(26, sj0, sj1);   // supervisor: stop handling (serial job + release + command)
          continue;
        }
      }
      if ((++idle & 63u) == 0u) {
        if (gld(&ctl->abort)) { if (lane == 0) vst(&s_abort, 1u); continue; }
        if (idle > kWSpinLimit) { wide_fault(P, ctl, 26, sup_pos, sup_nex, st); if (lane == 0) vst(&s_abort, 1u); continue; }
      }
      __builtin_amdgcn_s_sleep(2);
    }
    WPROF_T(loop1);
    WPROF_ADD(28, loop0, loop1);     // supervisor: whole queue
    // always on (two registers, two stores per launch): looks that found no decision (the supervisor waits for the scanners)
    // and looks that consumed at least one (jobs / batches = decisions per look)
    if (hix == 0u) {
      if (lane == 0) {
        u64* const st = P.prof + (size_t)P.num_parts * 32 + (size_t)part * kWsSlots;
        st[kWsEmpty] = n_empty; st[kWsBatches] = n_batch; st[kWsStops] = n_stops; st[kWsFlushes] = n_flush;
        st[kWsRedoExcl] = n_redo; st[kWsSerial] = n_serial; st[kWsResourceVerdicts] = n_resv; st[kWsFar] = near ? 0u : 1u;
        st[kWsHomes] = H;
      }
      post_gcmd(kPcExit, 0);
    }
    post_lcmd(kPcExit, 0);
  } else if (home) {
    // =============================================================================================
    // TESTERS (home workgroups, waves 1-7); in serial mode (home 0 only): memory scanners of the sequential protocol
    // =============================================================================================
    int par = 0;
    WideHome psh;
    psh.task = s_task; psh.w = &s_hw;
    const u32 tw = wave - 1;
#ifdef CNS_PROF_TESTER
    psh.tp = (tw == 0 && hix == 0u) ? P.prof + (size_t)part * 32 : nullptr;
#endif
    const u32 ml = tw * 64u + lane;
    const u32 mrows = (nn + kWMs - 1u) / kWMs;   // rows of a memory-scanner lane: 37 for 16 384 nodes, 147 for 65 536, 1 171 for 524 288
    constexpr u32 kMW = MW;                      // ... one bit per row in kMW 64-bit words (scratch: these masks are not on any fast path)
    struct MMask { u64 w[kMW]; };
    const u32 mwords = (mrows + 63u) >> 6;
    // (serial-only mode, shared nodes: a job scans only the slots of its OWN partition — a contiguous range [rb, rb + rn) of the
    // group, KParams::tag_off; else the whole partition: rb = 0, rn = nn.  Row r of lane ml is slot rb + r * kWMs + ml.)
    u32 rb = 0, rn = nn, jrows = mrows, jwords = mwords;
    u32 gseq = 0;          // k_giant (tester wave 1): jobs posted to the helpers
    bool gdead = false;    // ... a helper's answer did not come: device fault 43, every later job scanned by the home
    auto margmin = [&](const MMask& mask, const MMask* minus, u64& bc, u32& bp) {   // lexicographic (cost key, slot) over the lane's rows in `mask` (and not in `minus`)
      bc = ~0ull; bp = kNone;
      for (u32 w = 0; w < jwords; ++w) {
        u64 m = mask.w[w] & (minus ? ~minus->w[w] : ~0ull);
        while (m) {
          const u32 r = w * 64u + (u32)__builtin_ctzll(m);
          m &= m - 1;
          const u32 p = rb + r * kWMs + ml;
          const u64 ck = cost_key(P.cost[qbeg + p]);
          if (ck < bc) { bc = ck; bp = p; }
        }
      }
    };
    auto mem_scan_serial = [&](u32 jl) {
      wg_barrier();  // S0
      if (vld(&s_homes) > 1u) l1_inv();   // (the arrays scanned below were committed on other CUs too)
      const u32 raw = fetch_job(P, jbeg + jl);
      const FastJob F = make_fast_job(P, raw);
      const u64 tyok = jr64(raw, kJsTyok);
      const u32 kk = F.k;
      const bool general = F.ntasks != F.k;
      MMask bmask, amask, used;
      for (u32 w = 0; w < kMW; ++w) { bmask.w[w] = 0; amask.w[w] = 0; used.w[w] = 0; }
      rb = 0; rn = nn;
      if (P.serial_only && P.slot_tag && P.tag_off) {
        const u32 tb = P.tag_base[part] + ((F.flags >> 8) & 0xFFu);
        rb = P.tag_off[tb]; rn = P.tag_off[tb + 1] - rb;
      }
      jrows = (rn + kWMs - 1u) / kWMs; jwords = (jrows + 63u) >> 6;
      // Four rows per trip, every load of the four issued before any is looked at, and both argmins taken on the way (round 6: one row
      // per trip with its seven loads, then a pass per argmin with a dependent cost load per candidate, was 56 us per decision on
      // c4all64k — latency, not bytes: the arrays of the group sit in the L2).  Rows ascend and `<` is strict: the same (cost, slot)
      // order as margmin's.
      const bool own_range = P.serial_only && P.slot_tag && P.tag_off;   // [rb, rb + rn) are the job's own partition's slots
      const u32 jt = (F.flags >> 8) & 0xFFu;
      u64 ac = ~0ull, tcs = ~0ull;
      u32 ap = kNone, tp = kNone;
      // The bits of the mask word under way collect in registers and go to the scratch masks once per word (a trip's four rows never
      // straddle a word: 64 % kWMsTrip == 0): a read-modify-write of scratch per row and mask kept every trip waiting on the last one.
      const bool hjob = gnh != 0u && !(F.flags & (kJfIncl | kJfExcl));   // k_giant: round 0 comes from the helpers
      bool built = !hjob;                                                // the row masks of this job exist
      auto scan_rows = [&]() {
      u64 wb = 0, wa = 0;
      for (u32 r0 = 0; r0 < jrows; r0 += kWMsTrip) {
        u32 vlen[kWMsTrip], vty[kWMsTrip], vtg[kWMsTrip], vfmem[kWMsTrip];
        int vfcpu[kWMsTrip];
        u64 vfcnt[kWMsTrip], vck[kWMsTrip];
        bool in[kWMsTrip];
#pragma unroll
        for (u32 u = 0; u < kWMsTrip; ++u) {
          const u32 pr = rb + (r0 + u) * kWMs + ml;
          in[u] = r0 + u < jrows && pr < rb + rn;
          const u32 q = qbeg + (in[u] ? pr : rb);
          vlen[u] = (P.serial_only && P.f_len) ? P.f_len[q] : hdr_of(P, q)->len;
          vty[u] = P.slot_type[q];
          vfcpu[u] = P.f_cpu[q]; vfmem[u] = P.f_mem[q]; vfcnt[u] = P.f_cnt[q];
          vck[u] = cost_key(P.cost[q]);
          vtg[u] = (P.slot_tag && !own_range) ? (u32)P.slot_tag[q] : jt;
        }
#pragma unroll
        for (u32 u = 0; u < kWMsTrip; ++u) {
          if (!in[u]) continue;
          const u32 r = r0 + u;
          const u32 pr = rb + r * kWMs + ml;
          NodeSum ns;
          ns.cost = 0; ns.code = pr; ns.len = vlen[u]; ns.type = vty[u];
          ns.fcpu = vfcpu[u]; ns.fmem = vfmem[u]; ns.fcnt = vfcnt[u];
          bool b, a;
          eval_node(P, F.mv, F.flags, tyok, ns, b, a);
          if (vtg[u] != jt) { b = false; a = false; }   // shared nodes: only the slots of the job's own partition
          if (F.flags & kJfExclusive) {   // exclusive: the node must be completely free now (necessary for :6251-6257)
            const Res tt = P.type_total[ns.type];
            a = b && ns.fcpu >= clamp_cpu(tt.cpu) && ns.fmem >= mem_mib_ceil(tt.mem) && ns.fcnt == class_counts(tt.gres, P.gres);
          }
          wb |= (u64)(b ? 1u : 0u) << (r & 63u);
          wa |= (u64)(a ? 1u : 0u) << (r & 63u);
          if (a && vck[u] < ac) { ac = vck[u]; ap = pr; }
          if (b && vck[u] < tcs) { tcs = vck[u]; tp = pr; }
        }
        if (((r0 + kWMsTrip) & 63u) == 0u || r0 + kWMsTrip >= jrows) { bmask.w[r0 >> 6] = wb; amask.w[r0 >> 6] = wa; wb = 0; wa = 0; }
      }
      };
      if (!hjob) scan_rows();
      if constexpr (kGiantMW) {
        if (hjob && tw == 0u) {   // tester wave 1: post the job, collect the helpers' answers (lane i: helper i), reduce below
          GiantCtl* const gc = (GiantCtl*)(P.giant_ctl + (size_t)part * sizeof(GiantCtl));
          if (!gdead) {
            ++gseq;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // (every commit of the earlier jobs is drained: S1, S0)
            if (lane == 0) __hip_atomic_store(&gc->job, ((u64)gseq << 32) | jl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool ok = false;
            for (u32 spin = 0; spin < kGiantAnsSpin; ++spin) {
              const u32 t = lane < gnh ? __hip_atomic_load(&gc->ans[lane].tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gseq;
              if (!__any(t != gseq)) { ok = true; break; }
              __builtin_amdgcn_s_sleep(1);
            }
            if (ok) {
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
              if (lane < gnh) {
                ac = __hip_atomic_load(&gc->ans[lane].ac, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ap = __hip_atomic_load(&gc->ans[lane].ap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                tcs = __hip_atomic_load(&gc->ans[lane].tc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                tp = __hip_atomic_load(&gc->ans[lane].tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            } else {
              if (lane == 0) set_fault(P, 43, jl, gseq, gnh);
              gdead = true;
            }
          }
          if (gdead) giant_scan(P, F, tyok, qbeg, rb, rn, own_range, jt, lane, 64u, ac, ap, tcs, tp);   // exact, one wave
        }
      }
      if (F.flags & (kJfIncl | kJfExcl)) {  // included / excluded node lists (rare)
        for (u32 w = 0; w < jwords; ++w) {
          const u32 rows = jrows - w * 64u < 64u ? jrows - w * 64u : 64u;
          const u64 lm = list_mask<kWMs>(Pg, F.flags, jbeg + jl, bmask.w[w], qbeg + rb + ml + w * 64u * kWMs, rows);
          bmask.w[w] &= lm;
          amask.w[w] &= lm;
        }
        margmin(amask, nullptr, ac, ap);
        margmin(bmask, nullptr, tcs, tp);
      }
      wave_argmin(ac, ap);
      wave_argmin(tcs, tp);
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
      // Phase A walks the start-now set, Phase B the res_total set (mirror of worker_job_slow, as k_pipe's scanners)
      int verdict = 0;
      u32 nsel = 0;
      bool phase_b = wcode == kNone;
      u32 cur = phase_b ? tcode : wcode;
      bool b3 = phase_b;         // Phase B ends with B3
      for (;;) {
        if (cur == kNone) {
          if (!phase_b) {   // :6335 ff.
            phase_b = true; b3 = true; cur = tcode;
            for (u32 w = 0; w < kMW; ++w) used.w[w] = 0;
            continue;
          }
          break;
        }
        if ((cur - rb) % kWMs == ml) { const u32 r = (cur - rb) / kWMs; used.w[r >> 6] |= 1ull << (r & 63u); }
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
        if (!built) { scan_rows(); built = true; }   // k_giant: the walk needs a second candidate
        margmin(phase_b ? bmask : amask, &used, c, pc);
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
      }
      wg_barrier();  // S1 (the committed values are in the HBM arrays: nothing to refresh here)
    };
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
          const u32 kind = vld(&s_cmd[0]), cj = vld(&s_cmd[1]);
          if (vld(&s_cmd_seq) == cs) {   // (seq, kind, job) read consistently
            seen = cs;
            if (kind == kPcSerial) { mem_scan_serial(cj); continue; }
            if (kind == kPcExit) { leave = true; break; }
          }
          continue;
        }
        WPROF_T(r0);
        const bool retired_one = P.wide_cores ? wide_retire_one<true>(Pg, psh, qbeg) : wide_retire_one<false>(Pg, psh, qbeg);   // retirement first: it frees the nodes younger tasks wait for
        WPROF_T(r1);
        if (retired_one) { if (tw == 0 && hix == 0u) { WPROF_ADD(6, r0, r1); WPROF_CNT(15); } continue; }   // tester 0: cycles / calls of retirements that made progress (incl. the commits)
        if (vld(&s_posted) >= my) { go = true; break; }
        if (tw == 0 && hix == 0u) WPROF_CNT(31);                       // tester 0: naps without work
        nap_idle();
      }
      if (leave) break;
      if (go) {
        WPROF_T(t0);
        if (P.wide_cores) wide_test_task<true>(Pg, psh, my, qbeg, resv_part, jbeg); else wide_test_task<false>(Pg, psh, my, qbeg, resv_part, jbeg);
        WPROF_T(t1);
        if (tw == 0 && hix == 0u) { WPROF_ADD(8, t0, t1); WPROF_CNT(9); }   // tester 0: cycles in tests (incl. dependency waits), tasks tested
        have = false;
      }
    }
  } else {
#ifdef CNS_PROF_HOME_ONLY   // (-DCNS_PROF -DCNS_PROF_HOME_ONLY: counters of the home workgroup only — the scanners run at production speed)
#undef WPROF_T
#undef WPROF_ADD
#undef WPROF_CNT
#define WPROF_T(var)
#define WPROF_ADD(slot, a, b)
#define WPROF_CNT(slot)
#endif
#if defined(CNS_PROF) && defined(CNS_PROF_SCAN_ONLY)   // (... -DCNS_PROF_SCAN_ONLY: the scanners' counters only — the home workgroup at production speed;
#undef WPROF_T                                         // every WPROF_ADD is a global read-modify-write: the probes of one side slow that side by 15-25 %)
#undef WPROF_ADD
#undef WPROF_CNT
#define WPROF_T(var) const long long var = clock64()
#ifdef CNS_PROF_REGS   // (... -DCNS_PROF_REGS: the scanners' counters accumulate in registers and are written once at the end — a probe is a
#define CNS_WPROF_REGS_ON 1                            // clock read and an add, not a global read-modify-write with its wait on the chain)
#define WPROF_ADD(slot, a, b) do { wacc[slot] += (u64)((b) - (a)); } while (0)
#define WPROF_CNT(slot) do { wacc[slot] += 1; } while (0)
#else
#define WPROF_ADD(slot, a, b) do { if (lane == 0) P.prof[(size_t)part * 32 + (slot)] += (u64)((b) - (a)); } while (0)
#define WPROF_CNT(slot) do { if (lane == 0) P.prof[(size_t)part * 32 + (slot)] += 1; } while (0)
#endif
#endif
#ifdef CNS_WPROF_REGS_ON
    u64 wacc[32];
#pragma unroll
    for (int x = 0; x < 32; ++x) wacc[x] = 0;
#endif
    // =============================================================================================
    // SCANNERS (workgroups 1-8, waves 0-3: one per SIMD) — register-resident node tile: slot p = r * kWLanes + gt = code
    // =============================================================================================
    const u32 sid = (m - 1u) * (u32)kWScanPerWg + wave;   // scanner wave 0..31
    // Which slot a lane holds.  Interleaved (default): slot gt = lane * kWSW + sid, so that CONSECUTIVE nodes sit on DIFFERENT waves — on a
    // cold cluster (all costs equal: ties go to the lowest node index, JobScheduler.h:503) consecutive jobs take consecutive nodes, and a
    // window of jobs resolves whole only while its winners are spread over the waves (tests/test_exchange_pairs_model.py).  Blocked
    // (-DCNS_WIDE_BLOCKED_ROWS: rounds 2-4): gt = sid * 64 + lane.  Only the tile loads see the difference (strided instead of contiguous).
#ifdef CNS_WIDE_BLOCKED_ROWS
    const u32 gt = sid * 64u + lane;
    auto lane_of = [&](u32 code) __attribute__((always_inline)) -> u32 { return code & 63u; };
#else
    const u32 gt = lane * (u32)kWSW + sid;
    auto lane_of = [&](u32 code) __attribute__((always_inline)) -> u32 { return (code & (kWLanes - 1u)) / (u32)kWSW; };
#endif
    using RM = u32;  // one bit per row of the lane
    const RM kOne = 1;
    double cost[NPL];
    int fcpu[NPL];
    u32 mw[NPL];   // fmem GiB (16) | len (10) << 16 | type (6) << 26 ; len = 1023 marks "no node"
    u32 gn[NPL];   // per-class free-slot count, 4 bits each
    // the node's dip (KParams::dip_*): seconds after now (0xFFFFFFFF: none) | cpus << 16 | GiB | GRES nibbles
    u32 dpt[NPL], dpc[NPL], dpg[NPL];
    bool any_dip = false;       // wave-uniform: some row of this wave has one (else the dip test is skipped: cold clusters)
    const u32 maxlen = P.max_jobs_per_node;
    RM okbits = 0;
    u64 wave_types = 0;
    // The committed state, written by the HOME workgroup with plain stores (drained before a task is marked committed).  All
    // loads bypass this CU's L1 (sc1): on one XCD the L2 is the point of coherence, so no cache invalidation is needed there.
    auto ld32 = [&](const void* p) __attribute__((always_inline)) -> u32 { return __hip_atomic_load((const u32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto ld64 = [&](const void* p) __attribute__((always_inline)) -> u64 { return __hip_atomic_load((const u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto load_tile = [&]() __attribute__((always_inline)) {
      okbits = 0;
      wave_types = 0;
      bool dip_here = false;
#pragma unroll
      for (int r = 0; r < NPL; ++r) {
        const u32 p = (u32)r * kWLanes + gt;
        if (p < nn) {
          const u32 q = qbeg + p;
          const NodeHdr* hd = hdr_of(P, q);
          cost[r] = __longlong_as_double((long long)ld64(&P.cost[q]));
          fcpu[r] = (int)ld32(&P.f_cpu[q]);
          mw[r] = mem_gib16(ld32(&P.f_mem[q])) | (ld32(&hd->len) << 16) | ((u32)P.slot_type[q] << 26);
          gn[r] = nibbles_of(ld64(&P.f_cnt[q]));
          dpt[r] = ld32(&P.dip_t[q]); dpc[r] = ld32(&P.dip_cm[q]); dpg[r] = ld32(&P.dip_g[q]);
        } else {
          cost[r] = 0.0; fcpu[r] = 0; mw[r] = 1023u << 16; gn[r] = 0;
          dpt[r] = 0xFFFFFFFFu; dpc[r] = 0; dpg[r] = 0;
        }
        dip_here = dip_here | (dpt[r] != 0xFFFFFFFFu);
        const u32 len = (mw[r] >> 16) & 0x3FFu;
        okbits |= (RM)(len < maxlen ? 1u : 0u) << r;
        if (len != 1023u) wave_types |= 1ull << (mw[r] >> 26);
      }
      wave_types = wave_or_u64(wave_types);
      any_dip = __any(dip_here);
    };
    const u32 G8 = 0x80808080u;

    struct ScanJob {   // kept as the record's packed dwords (scalar registers are scarce here); unpacked where used
      u32 head;        // flags | node_num << 8 | shape << 24
      u32 mem;         // rm16 | dm16 << 16: the request / the selection's memory in whole GiB (rounded down)
      u32 gr;          // gmode | gsel << 4 | gneed << 16
      int rc32;
      u32 rq, gtot, acnt;   // acnt: the selection's GRES slots per class (nibbles)
      i64 L;           // time limit (the cost update of a selection)
      __device__ __forceinline__ u32 flags() const { return head & 0xFFu; }
      __device__ __forceinline__ u32 k() const { return (head >> 8) & 0xFFFFu; }
      __device__ __forceinline__ u32 shape() const { return head >> 24; }
      __device__ __forceinline__ u32 rm16() const { return mem & 0xFFFFu; }
      __device__ __forceinline__ u32 dm16() const { return mem >> 16; }
      __device__ __forceinline__ u32 gmode() const { return gr & 0xFu; }
      __device__ __forceinline__ u32 gsel() const { return (gr >> 4) & 0xFFFu; }
      __device__ __forceinline__ u32 gneed() const { return gr >> 16; }
      __device__ __forceinline__ i64 mcpu() const { return (i64)rc32; }   // min-view cpu: exact whenever the request is satisfiable at all (shape bit 2)
    };
    auto decode = [&](u32 raw, u64& tyok) __attribute__((always_inline)) {   // the scanners' 12 dwords of the record (k_prep_jobs, kJsHead ff.)
      ScanJob S;
      S.head = rl32(raw, kJsHead); S.mem = rl32(raw, kJsMem); S.gr = rl32(raw, kJsGres);
      S.rc32 = (int)rl32(raw, kJsRc32);
      S.rq = rl32(raw, kJsRq);
      S.gtot = rl32(raw, kJsGtot);
      S.L = (i64)jr64(raw, kJsL);
      S.acnt = rl32(raw, kJsAcnt);
      tyok = jr64(raw, kJsTyok);
      return S;
    };
    auto lane_argmin = [&](RM mask, u64& bc, u32& bp) __attribute__((always_inline)) {
      bc = ~0ull;
      u32 br = 0xFFu;
#pragma unroll
      for (int r = 0; r < NPL; ++r) {
        const u64 ck = cost_key(cost[r]);
        const bool take = ((mask >> r) & 1u) & (ck < bc);
        bc = take ? ck : bc;
        br = take ? (u32)r : br;
      }
      bp = br == 0xFFu ? kNone : ((br << kWShift) | gt);
    };
    auto row_type_r = [&](u32 rr) __attribute__((always_inline)) -> u32 {  // node type of row rr (wave-uniform) of every lane
      u32 ty = 0;
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if ((u32)r == rr) ty = mw[r] >> 26;
      return ty;
    };
    // payload of a wave-uniform winner code of THIS wave: code << 6 | node type
    auto pay_of = [&](u32 code) __attribute__((always_inline)) -> u32 {
      if (code == kNone) return kWNonePay;
      const u32 ty = rl32(row_type_r(uni32(code >> kWShift)), uni32(lane_of(code)));
      return (code << 6) | ty;
    };
    // Candidate sets of one job as per-lane bitmasks + their lane-local argmins (k_pipe's scan_job)
    auto scan_job = [&](const ScanJob& S, u64 sji, u64 tyok, bool lean, RM& bmask, RM& amask, u64& ac, u32& ap, u64& tcs, u32& tp) __attribute__((always_inline)) {
      RM tybits = (RM)(((u64)1 << NPL) - 1ull);
      if ((tyok & wave_types) != wave_types) {
        tybits = 0;
#pragma unroll
        for (int r = 0; r < NPL; ++r) tybits |= (RM)((tyok >> (mw[r] >> 26)) & 1ull) << r;
      }
      const RM bl = (S.shape() & 4u) ? (RM)(okbits & tybits) : (RM)0;
      u32 gme = 0, gmo = 0;
      if (S.gmode() & 2u) { gme = uni32(s_nme[S.gsel() >> 8]); gmo = uni32(s_nmo[S.gsel() >> 8]); }
      RM am = 0;
      ac = ~0ull; tcs = ~0ull;
      u32 ar = 0xFFu, tr = 0xFFu;
      auto rows = [&](auto mode, auto leantag, auto diptag) __attribute__((always_inline)) {
        constexpr u32 M = decltype(mode)::value;
        constexpr bool kLean = decltype(leantag)::value != 0;   // start-now argmin only (T comes from the wave's cache)
        constexpr bool kDip = decltype(diptag)::value != 0;     // some row of this wave has a dip (else the test is not even compiled in)
        const u32 sh1 = S.gsel() & 0xFFu, need1 = S.gneed() & 0xFFu, need2 = S.gneed() >> 8;
        const u32 rqe = S.rq & 0x0F0F0F0Fu, rqo = (S.rq >> 4) & 0x0F0F0F0Fu;
        // the request's GRES part against per-class counts `g` (8 saturating nibbles): the front's, or the dip's
        auto gfit = [&](u32 g) __attribute__((always_inline)) -> bool {
          bool ok = true;
          if (M == 1) {
            if (S.gmode() & 1u) ok = ok & (((g >> sh1) & 15u) >= need1);
            if (S.gmode() & 2u) {
              const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
              ok = ok & (__builtin_amdgcn_sad_u8(ce & gme, 0u, __builtin_amdgcn_sad_u8(co & gmo, 0u, 0u)) >= need2);
            }
          }
          if (M == 4) {
            const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
            ok = ok & ((((ce | G8) - rqe) & G8) == G8) & ((((co | G8) - rqo) & G8) == G8);
#pragma unroll
            for (int n = 0; n < kMaxNames; ++n) {
              const u32 tot = (S.gtot >> (8 * n)) & 0xFFu;
              const u32 have = __builtin_amdgcn_sad_u8(ce & s_nme[n], 0u, __builtin_amdgcn_sad_u8(co & s_nmo[n], 0u, 0u));
              ok = ok & ((tot == 0) | (have >= (tot > 15u ? 15u : tot)));
            }
          }
          return ok;
        };
        const u32 loff = S.L >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (u32)S.L;   // an entry t seconds after now lies in the window iff t < L (:6279)
        const u32 rcpus = (u32)S.rc32 >> 8;                              // whole cpus of the request, rounded down
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
          const bool b = ((bl >> r) & 1u) != 0;
          bool a = b & (S.rc32 <= fcpu[r]) & (S.rm16() <= (mw[r] & 0xFFFFu));
          if (M != 0) a = a & gfit(gn[r]);
          if (kDip) {   // a window that reaches the node's dip must fit the dip too: a second necessary condition
            bool fits = (rcpus <= (dpc[r] >> 16)) & (S.rm16() <= (dpc[r] & 0xFFFFu));
            if (M != 0) fits = fits & gfit(dpg[r]);
            a = a & ((dpt[r] >= loff) | fits);
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
      const bool dips = any_dip;
      if (dips) {          // (rare outside loaded clusters: only after a misprediction recorded one on a node of this wave)
        if (S.gmode() == 0) rows(ModeTag<0>{}, ModeTag<0>{}, ModeTag<1>{});
        else if (S.gmode() < 4) rows(ModeTag<1>{}, ModeTag<0>{}, ModeTag<1>{});
        else rows(ModeTag<4>{}, ModeTag<0>{}, ModeTag<1>{});
      } else if (lean) {
        if (S.gmode() == 0) rows(ModeTag<0>{}, ModeTag<1>{}, ModeTag<0>{});
        else if (S.gmode() < 4) rows(ModeTag<1>{}, ModeTag<1>{}, ModeTag<0>{});
        else rows(ModeTag<4>{}, ModeTag<1>{}, ModeTag<0>{});
      } else {
        if (S.gmode() == 0) rows(ModeTag<0>{}, ModeTag<0>{}, ModeTag<0>{});
        else if (S.gmode() < 4) rows(ModeTag<1>{}, ModeTag<0>{}, ModeTag<0>{});
        else rows(ModeTag<4>{}, ModeTag<0>{}, ModeTag<0>{});
      }
      bmask = bl; amask = am;
      ap = ar == 0xFFu ? kNone : ((ar << kWShift) | gt);
      tp = tr == 0xFFu ? kNone : ((tr << kWShift) | gt);
      if (S.flags() & (kJfIncl | kJfExcl)) {  // included / excluded node lists (rare)
        const RM lm = (RM)list_mask<kWLanes>(Pg, S.flags(), sji, bmask, qbeg + gt, (u32)NPL);
        bmask &= lm;
        amask &= lm;
        lane_argmin(amask, ac, ap);
        lane_argmin(bmask, tcs, tp);
      }
    };
    // predicted effect of a selection on the row that holds node `code` (the commit itself happens later, on a tester
    // wave): MinCpuTimeRatioFirst::UpdateCost (JobScheduler.h:47-53) and, for a start-now selection, the front
    // summary minus the allocation.  Exact for the cost and the front cpu, conservative for memory and GRES counts.
    // The predicted effect of a selection on the row that holds node `code` (wave-uniform), in two steps so that the
    // arithmetic of the wave's OWN candidate can run while the exchange is in flight: pre_sel computes the row's new
    // values, put_sel writes them.  MinCpuTimeRatioFirst::UpdateCost (JobScheduler.h:47-53: ratio first, then x seconds,
    // then +=; end - start is the time limit whatever the start) and, for a start-now selection, the front summary minus
    // the allocation.  Exact for the cost and the front cpu, conservative for memory (whole GiB) and saturated GRES counts.
    struct RowVal { double ucost; u32 w, g; int fc; };
    // ... on the row's values (mem | len | type, GRES counts, front cpu) wherever they are held: the tile (pre_sel) or a copy of the row in a
    // window's pool — ONE piece of arithmetic, so that every copy of a row moves the same way
    auto pre_sel_vals = [&](const ScanJob& S, u64 cost0, u32 ty, bool front, u32 w, u32 g, int fc) __attribute__((always_inline)) -> RowVal {
      const double ratio = ((double)S.mcpu() / 256.0) / ((double)s_tytot[ty] / 256.0);
      RowVal v;
      v.ucost = __longlong_as_double((long long)cost0) + (double)S.L * ratio;
      if (front) {
        const u32 m16 = w & 0xFFFFu, dm = S.dm16();
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
      v.w = w; v.g = g; v.fc = fc;
      return v;
    };
    auto pre_sel = [&](const ScanJob& S, u32 code, u64 cost0, u32 ty, bool front) __attribute__((always_inline)) -> RowVal {
      const u32 rsel = 1u << uni32(code >> kWShift);   // (a one-hot row mask: an `r == rr` chain gets turned into a dynamic array index, which sends the tile to scratch)
      u32 w = 0, g = 0;
      int fc = 0;
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if ((rsel >> r) & 1u) { w = mw[r]; g = gn[r]; fc = fcpu[r]; }
      return pre_sel_vals(S, cost0, ty, front, w, g, fc);
    };
    auto put_sel = [&](u32 code, const RowVal& v) __attribute__((always_inline)) {
      const u32 rsel = 1u << uni32(code >> kWShift);   // (a one-hot row mask: an `r == rr` chain gets turned into a dynamic array index, which sends the tile to scratch)
      const bool own = (code & (kWLanes - 1u)) == gt;
#pragma unroll
      for (int r = 0; r < NPL; ++r)
        if ((rsel >> r) & 1u) {
          cost[r] = own ? v.ucost : cost[r];
          mw[r] = own ? v.w : mw[r];
          gn[r] = own ? v.g : gn[r];
          fcpu[r] = own ? v.fc : fcpu[r];
        }
    };
    auto apply_sel = [&](const ScanJob& S, u32 code, u64 cost0, u32 ty, bool front) __attribute__((always_inline)) {
      const RowVal v = pre_sel(S, code, cost0, ty, front);
      put_sel(code, v);
    };

    const bool leader = sid == 0;
    u32 seen = 0;
    u32 pos = 0;                // next job of the autonomous run
    u32 nex = 0;                // exchanges so far (the next one carries tag nex + 1)
    u32 stops = 0;
    bool running = true;        // autonomous (else: waiting for the supervisor's command)
    u32 have_raw_j = kNone;     // job whose record sits in `raw`
    u32 raw = 0;
    RM bmask = 0, amask = 0;
    ScanJob J, Jn;
    u64 typeok = 0, typeok_n = 0;
    u32 dec_j = kNone;          // job whose decoded record sits in Jn
    J.head = 1u << 8; J.mem = 0; J.gr = 0; J.rc32 = 0; J.rq = 0; J.gtot = 0; J.acnt = 0; J.L = 0;
    Jn = J;
    // Per-wave cache of the res_total argmin T (see k_pipe): valid until the cached node itself is selected or the
    // tile is reloaded.
    bool tvalid = false;
    u64 tc_c = ~0ull;
    u32 tp_c = kNone, tpay_c = kWNonePay;
    u32 sn = 0;                 // leader: last value read from ctl->sup_nex (only grows)
    u32 hreq_n = 0, sn_n = 0;   // ... the loads issued during the PREVIOUS job (their ~1 us must not sit on the chain)
    u32 xj = kNone;             // job xj must not take the slots in WideCtl::excl_code as start-now candidates
    auto stop_at = [&](u32 j) {
      ++stops;
      if (leader) {
        if (lane == 0) { gst(&ctl->scan_pos, j); gst(&ctl->scan_nex, nex); }
        vm_drain();
        if (lane == 0) gst(&ctl->scan_stops, stops);
      }
      running = false;
    };
    // this wave's k best candidates of `mk`, sorted, as granules of exchange e; `hbit`: the halt bit of the leader
    // this wave's k best candidates of the start-now set `ma` AND of the res_total set `mb`, each sorted, in ONE pass (the two
    // argmin cascades of a round alternate their DPP steps): lane i leaves with entry i of both lists; the start-now list is
    // published as the granules of exchange e (`hbit`: the halt bit of the leader), the other one only if the job turns out
    // to need it (publish_list) — without another k rounds then
    auto publish_list = [&](u32 xs, u32 e, u64 c, u32 py, u32 k, u32 hbit) __attribute__((always_inline)) {
      if (lane < k) {
        u32x4 v;
        v.x = e; v.y = py | ((lane == 0 && hbit) ? 0x80000000u : 0u); v.z = (u32)c; v.w = (u32)(c >> 32);
        gran_st(rs_xr, kXl + (xs * (u32)(kWSW * kPMaxK) + sid * (u32)kPMaxK + lane) * 16u, v, near);
      }
    };
    // entry `rank` of the decision of exchange e (WideCtl::xd): one granule, one lane (the caller's wave-uniform values)
    auto put_decision = [&](u32 xs, u32 e, u32 rank, u32 word, u64 c) __attribute__((always_inline)) {
      if (lane == 0) {
        u32x4 v;
        v.x = e; v.y = word; v.z = (u32)c; v.w = (u32)(c >> 32);
        gran_st(rs_xr, kXd + (xs * (u32)kPMaxK + rank) * 16u, v, near);
      }
    };
    auto post_lists = [&](u32 xs, u32 e, RM ma, RM mb, u32 k, u32 hbit, u64& lac, u32& lap, u64& ltc, u32& ltp) __attribute__((always_inline)) {
      lac = ~0ull; lap = kWNonePay; ltc = ~0ull; ltp = kWNonePay;
      for (u32 i = 0; i < k; ++i) {
        u64 ca = ~0ull, cb = ~0ull;
        u32 pa = kNone, pb = kNone;
        lane_argmin(ma, ca, pa);
        lane_argmin(mb, cb, pb);
        wave_argmin2(ca, pa, cb, pb);
        pa = uni32(pa); pb = uni32(pb);
        if (pa == kNone && pb == kNone) break;   // both sets are exhausted
        const u32 pya = pay_of(pa), pyb = pay_of(pb);
        if (pa != kNone && (pa & (kWLanes - 1u)) == gt) ma &= ~(kOne << (pa >> kWShift));
        if (pb != kNone && (pb & (kWLanes - 1u)) == gt) mb &= ~(kOne << (pb >> kWShift));
        if (lane == i) { lac = uni64(ca); lap = pya; ltc = uni64(cb); ltp = pyb; }
      }
      publish_list(xs, e, lac, lap, k, hbit);
    };
    // The list exchange as the scanners read it: the granules stay in registers (lane l: entries l, l + 64, ...).  As for a
    // single node, a scanner wave does not need the merged selection, only which entries of its OWN list are among the first
    // k of all lists together: entry x is, iff fewer than k entries come before it.  One compare per granule and lane and a
    // population count per own entry — and a wave whose best entry is not selected is done after one round (the k-way merge
    // took k argmin cascades on every wave).  The supervisor, which needs the selection itself, still merges.
    struct ListGran { u64 c[kWLl]; u32 p[kWLl]; };
    auto lists_poll = [&](u32 xs, u32 e, u32 k, ListGran& L, u32& halt) __attribute__((always_inline)) -> bool {
      u32x4 g[kWLl];
      bool ok = true;
#pragma unroll
      for (int jj = 0; jj < (int)kWLl; ++jj) {
        const u32 idx = lane + 64u * (u32)jj;
        g[jj] = gran_ld(rs_xr, kXl + (xs * (u32)(kWSW * kPMaxK) + idx) * 16u);
        if ((idx & 7u) < k && g[jj].x != e) ok = false;
      }
      if (__any(!ok)) return false;
#pragma unroll
      for (int jj = 0; jj < (int)kWLl; ++jj) {
        const u32 idx = lane + 64u * (u32)jj;
        u64 c = ~0ull;
        u32 p = kNone;
        if ((idx & 7u) < k) gran_decode(g[jj], c, p);
        L.c[jj] = c;
        L.p[jj] = p;
      }
      halt = rl32(g[0].y, 0) >> 31;
      return true;
    };
    // entries of the exchange (capped at k) and, in `sel`, which entries of this wave's own list (myc / myp, lane i: entry i) are selected
    // ... and hands the supervisor its part of the decision: own entry with `before` entries in front of it is node `before`
    // of the selection (the keys (cost, payload) are distinct); no entry anywhere: the leader says so.
    auto vote_lists = [&](const ListGran& L, u32 k, u64 myc, u32 myp, u32& sel, u32 xsd, u32 ed) __attribute__((always_inline)) -> u32 {
      u32 total = 0;
#pragma unroll
      for (int jj = 0; jj < (int)kWLl; ++jj) total += (u32)__builtin_popcountll(__ballot(L.p[jj] != kNone));
      const u32 nf = total < k ? total : k;
      if (total == 0 && leader) put_decision(xsd, ed, 0, kWdNone | (k << kWdKShift), 0);
      sel = 0;
      for (u32 i = 0; i < k; ++i) {
        const u32 op = rl32(myp, i);
        if (op == kWNonePay) break;
        const u64 oc = rl64(myc, i);
        u32 before = 0;
#pragma unroll
        for (int jj = 0; jj < (int)kWLl; ++jj)
          before += (u32)__builtin_popcountll(__ballot((L.c[jj] < oc) | ((L.c[jj] == oc) & (L.p[jj] < op))));
        if (before >= k) break;   // (the list is sorted: the entries behind it are not selected either)
        sel |= 1u << i;
        put_decision(xsd, ed, before, op | (k << kWdKShift) | (nf << kWdNfShift), oc);
      }
      return nf;
    };
    auto wait_lists = [&](u32 xs, u32 e, u32 k, ListGran& L, u32& halt) -> bool {
      for (u32 spin = 0;; ++spin) {
        if (leader) WPROF_CNT(7);
        if (lists_poll(xs, e, k, L, halt)) return true;
        if ((spin & 63u) == 63u) {
          if (gld(&ctl->abort)) return false;
          if (spin > kWSpinLimit) { wide_fault(P, ctl, 28, nex, sid, 1); return false; }
        }
        __builtin_amdgcn_s_sleep(1);
      }
    };
    u32 n_lapwait = 0;          // leader: polls spent waiting for the supervisor (always counted, written at exit)
    auto lap_guard = [&](u32 ahead) {   // leader: the supervisor reads the rings a few jobs later: do not lap it (`ahead`: exchange numbers about to be used)
      for (u32 spin = 0; nex + 1u + ahead >= sn + kWRing; ++spin) {
        ++n_lapwait;
        sn = gld(&ctl->sup_nex);
        if ((spin & 63u) == 63u) {
          if (gld(&ctl->abort)) break;
          if (spin > kWSpinLimit) { wide_fault(P, ctl, 29, nex, sn, 0); break; }
        }
        if (nex + 1u + ahead >= sn + kWRing) __builtin_amdgcn_s_sleep(2);
      }
    };

#ifdef CNS_PROF_FAST   // (-DCNS_PROF_FAST: the steady-state loop by segment, per wave, in registers; tools/prof_wide.py CNS_PROF_FAST=1)
    u64 fa_pub[2] = {0, 0}, fa_cnt[2] = {0, 0}, fa_wait[2] = {0, 0}, fa_dec[2] = {0, 0}, fa_nl = 0, fa_fr = 0;
    u64 fa_seg[4] = {0, 0, 0, 0};   // inside the first segment: record -> scalars + control words | rows | argmin cascades | payloads + lap guard + publish
    u32 fa_won = 0;   // this wave won the previous job of the loop
#define FPROF_T(var) const long long var = clock64()
#else
#define FPROF_T(var)
#endif
#if defined(CNS_WIDE_WINDOWS) && !defined(CNS_WIDE_NO_FAST_K1) && (!defined(CNS_PROF) || defined(CNS_PROF_HOME_ONLY))
#define CNS_WIDE_WIN_ON 1
    // ---- state of the window path ("A WINDOW OF JOBS PER EXCHANGE", below) ----------------------------------------------------------
    constexpr u32 kWQ = 3u * kWB;        // the records of jobs wq_pos .. wq_pos + kWQ - 1, one register each (lane l: dword l of the record): the chunk at hand + two ahead
    constexpr bool kWinTile = kWinK && NPL <= 2;  // (4 and more rows per lane: the window path's registers on top of the tile spill — 61 / 234 VGPRs at 4 / 8 rows —
                                         // and the configurations of that width are bound by backfills on deep time maps, which the pool does not decide)
    const u32 win_max = (kWinTile && P.wide_inject_stall == 0u) ? (uni32(P.wide_window) < kWJ ? uni32(P.wide_window) : kWJ) : 0u;
    u32 wq[kWQ];
#pragma unroll
    for (u32 s = 0; s < kWQ; ++s) wq[s] = 0;
    u32 wq_pos = 0;
    bool wq_ok = false;
    u32 wseq = 0;                        // windows opened so far (the next pool exchange carries tag wseq + 1)
    u32 wback = 0, wpen = 4;             // single jobs to go before the next window may open | the penalty after a window that decided too little
#ifndef CNS_WIDE_YIELD
#define CNS_WIDE_YIELD 6
#endif
    constexpr u32 kWYield = CNS_WIDE_YIELD;
#ifdef CNS_PROF_WIN   // (-DCNS_PROF_WIN: the window path by segment, per wave, in registers; tools/prof_win.py)
    u64 wa[12];
#pragma unroll
    for (int x = 0; x < 12; ++x) wa[x] = 0;
#define WINP_T(var) const long long var = clock64()
#define WINP_ADD(slot, a, b) wa[slot] += (u64)((b) - (a))
#define WINP_CNT(slot) wa[slot] += 1
#else
#define WINP_T(var)
#define WINP_ADD(slot, a, b)
#define WINP_CNT(slot)
#endif
    u32 n_win = 0, n_winjobs = 0, n_windry = 0;   // leader: windows | jobs they decided | windows that decided nothing (always counted, written at exit)
    // one job went through a single-job exchange (`pos` has advanced): the next window is that much closer; two jobs ahead of it the record
    // queue is filled, so that its loads have landed when the window opens
    auto win_single_done = [&]() __attribute__((always_inline)) {
      if (wback != 0u) {
        --wback;
        if (wback == 2u && win_max >= 2u) {
#pragma unroll
          for (u32 s = 0; s < kWQ; ++s) wq[s] = fetch_job(P, jbeg + (pos + 2u + s < njobs ? pos + 2u + s : njobs - 1u));
          wq_pos = pos + 2u; wq_ok = true;
        }
      }
    };
#endif
    load_tile();   // the state the previous kernels left (kernel boundary: visible)
    for (;;) {
      WPROF_T(q0);
      if (!running) {
        // ---- wait for the supervisor's command ---------------------------------------------------------------------
        u32 kind = kPcExit, cj = 0;
        for (u32 spin = 0;; ++spin) {
          const u32 cs = gld(&ctl->cmd_seq);
          if (cs != seen) {
            vm_drain();
            kind = gld(&ctl->cmd_kind); cj = gld(&ctl->cmd_job);
            seen = cs;
            break;
          }
          if ((spin & 15u) == 15u && gld(&ctl->abort)) break;
          if (spin > kWCmdSpinLimit) { wide_fault(P, ctl, 40, pos, sid, 0); break; }
          __builtin_amdgcn_s_sleep(8);
        }
        if (kind != kPcResume) break;   // exit / abort
        if (!near) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the committed state of the home workgroup
        load_tile();
        tvalid = false;
        have_raw_j = kNone;
        dec_j = kNone;
#ifdef CNS_WIDE_WIN_ON
        wq_ok = false;
#endif
        hreq_n = 0;
        pos = cj;
        xj = gld(&ctl->excl_n) ? cj : kNone;   // the redo of a flushed job with excluded candidates (read when it is scanned)
        running = true;
        WPROF_T(qc);
        if (leader) WPROF_ADD(21, q0, qc);   // leader: waiting for a command + tile reload
        continue;
      }
#ifdef CNS_WIDE_WIN_ON
      // ---- A WINDOW OF JOBS PER EXCHANGE -----------------------------------------------------------------------------------------------
      // Every job moves exactly one row of the tile, and only towards "costlier and emptier" (MinCpuTimeRatioFirst::UpdateCost,
      // JobScheduler.h:526-538,567-575) — so the next several decisions all fall among the few cheapest rows.  Instead of exchanging one
      // candidate per job, a window exchanges the CANDIDATE POOL once: every wave publishes its kWM cheapest rows WITH THEIR STATE (cost,
      // front cpu / memory / GRES counts, type, dip flag) and the key of its next row (the bound).  Every wave then decides up to kWJ
      // consecutive jobs of the steady-state shape on its own copy of the pool (lane l: the rows of wave l) with no further communication:
      // least (cost, code) among the pool rows the job can start on, the same front test and the same row update as on the tile (pre_sel_vals)
      // — every wave applies it to its copy, the wave that owns the row also to its tile and writes the decision granule under the next
      // exchange number, so the supervisor and the decision ring see what they always saw.  A decision is exact as long as its key lies below
      // every wave's bound (no row outside the pool can come before it: those keys are >= the bounds and do not move) and the row carries no
      // dip; the first job for which that does not hold — or that finds no row in the pool, or is not of the shape — closes the window and
      // goes through the single-job exchange below.  Windows that decide (almost) nothing back off (a loaded cluster: every job a backfill).
      // The pool rule against the sequential one: tests/test_exchange_pairs_model.py; semantics: JobScheduler.cpp:6188-6300.
      if constexpr (kWinTile) if (win_max >= 2u && wback == 0u) {   // (wback > 0: jobs to go through the single-job exchange first — counted where `pos` advances)
        WINP_T(w0);
        // the record queue follows `pos`
        if (!wq_ok || pos - wq_pos > kWB) {
#pragma unroll
          for (u32 s = 0; s < kWQ; ++s) wq[s] = fetch_job(P, jbeg + (pos + s < njobs ? pos + s : njobs - 1u));
          wq_pos = pos; wq_ok = true;
        } else if (pos != wq_pos) {
          const u32 d = pos - wq_pos;   // 1 .. kWB: shift left in binary steps, then the last chunk again (its loads have two chunks of jobs to land)
#pragma unroll
          for (u32 b = 1; b <= kWB; b <<= 1)
            if (d & b) {
#pragma unroll
              for (u32 s = 0; s + b < kWQ; ++s) wq[s] = wq[s + b];
            }
#pragma unroll
          for (u32 s = kWQ - kWB; s < kWQ; ++s) wq[s] = fetch_job(P, jbeg + (pos + s < njobs ? pos + s : njobs - 1u));
          wq_pos = pos;
        }
        auto shaped = [&](u32 hd, u32 j) __attribute__((always_inline)) -> bool {   // the steady-state shape (the fast loop's), from the record's head
          return j < njobs && j != xj && ((hd >> 8) & 0xFFFFu) == 1u && ((hd >> 24) & 15u) == 6u && !(hd & (kJfExclusive | kJfIncl | kJfExcl));
        };
        const bool openw = shaped(rl32(wq[0], kJsHead), pos) && shaped(rl32(wq[1], kJsHead), pos + 1u);
        if (!openw) wback = 1u;   // (a job of another shape: through the loops below, then look again)
        if (openw) {
          const u32 hreq = uni32(hreq_n);
          { const u32 snu = uni32(sn_n); sn = snu > sn ? snu : sn; }
          if (leader) { hreq_n = gld_raw(&ctl->halt); sn_n = gld_raw(&ctl->sup_nex); }
          // ---- this wave's kWM cheapest rows and the key of the next one -----------------------------------------------------------------
          u32 gy = kWNonePay, gz = 0xFFFFFFFFu, gw = 0xFFFFFFFFu;   // lane 2m: record m's {payload | dip << 30, cost}; lane 2m + 1: {fcpu, mw, gn}; lane 2 kWM: the bound
          {
            RM mask = okbits;
#pragma unroll
            for (u32 m = 0; m <= kWM; ++m) {
              u64 c; u32 p;
              lane_argmin(mask, c, p);
              wave_argmin(c, p);
              p = uni32(p);
              u32 py = kWNonePay, rfc = 0, rmw = 0, rgn = 0, rdip = 0;
              if (p != kNone) {
                const u32 rsel = 1u << (p >> kWShift);
                const bool own = (p & (kWLanes - 1u)) == gt;
                u32 vfc = 0, vmw = 0, vgn = 0, vdp = 0;
#pragma unroll
                for (int r = 0; r < NPL; ++r)
                  if ((rsel >> r) & 1u) { vfc = (u32)fcpu[r]; vmw = mw[r]; vgn = gn[r]; vdp = dpt[r] != 0xFFFFFFFFu ? 1u : 0u; }
                if (own) mask &= ~(RM)rsel;
                const u32 ol = uni32(lane_of(p));
                rfc = rl32(vfc, ol); rmw = rl32(vmw, ol); rgn = rl32(vgn, ol); rdip = rl32(vdp, ol);
                py = (p << 6) | (rmw >> 26);
              }
              if (m < kWM) {
                if (lane == 2u * m) { gy = py | (rdip << 30); gz = (u32)c; gw = (u32)(c >> 32); }
                if (lane == 2u * m + 1u) { gy = rfc; gz = rmw; gw = rgn; }
              } else if (lane == 2u * kWM) { gy = py; gz = (u32)c; gw = (u32)(c >> 32); }
            }
          }
          WINP_T(w1);
          // ---- publish: ONE store, lane g its granule; the leader's bound granule carries the halt bit --------------------------------------
          if (leader) lap_guard(kWJ);
          const u32 wtag = wseq + 1u;
          const u32 wrow = (wseq & (kWPRing - 1u)) * kWPG;
          if (lane < kWPG) {
            u32x4 v;
            v.x = wtag;
            v.y = gy | ((leader && hreq && lane == 2u * kWM) ? 0x80000000u : 0u);
            v.z = gz; v.w = gw;
            gran_st(rs_xr, kXp + ((wrow + lane) * (u32)kWSW + sid) * 16u, v, near);
          }
          ++wseq;
          // ---- poll: the bound granules first (one load per lane and round), then the records ------------------------------------------------
          u32x4 gb, gr[2u * kWM];
          bool okx = true;
          for (u32 spin = 0;; ++spin) {
            gb = gran_ld(rs_xr, kXp + ((wrow + 2u * kWM) * (u32)kWSW + lane) * 16u);
            WINP_CNT(9);
            if (!__any(gb.x != wtag)) {
              bool all = true;
#pragma unroll
              for (u32 x = 0; x < 2u * kWM; ++x) {
                gr[x] = gran_ld(rs_xr, kXp + ((wrow + x) * (u32)kWSW + lane) * 16u);
                all = all & (gr[x].x == wtag);
              }
              if (!__any(!all)) break;
            }
            if ((spin & 63u) == 63u) {
              if (gld(&ctl->abort)) { okx = false; break; }
              if (spin > kWSpinLimit) { wide_fault(P, ctl, 28, nex, sid, 2); okx = false; break; }
            }
            __builtin_amdgcn_s_sleep(CNS_WIDE_POLL_NAP);
          }
          if (!okx) break;
          WINP_T(w2);
          if (rl32(gb.y, 0) >> 31) {   // halted in front of job pos: nothing applied, one void exchange number (as a halted single-job exchange)
            if (leader) put_decision(nex & (kWRing - 1), nex + 1u, 0, kWdHalt | kWdNone | (1u << kWdKShift), 0);
            ++nex;
            have_raw_j = kNone; dec_j = kNone; wq_ok = false;
            stop_at(pos);
            continue;
          }
          // ---- the pool: lane l holds the rows of wave l --------------------------------------------------------------------------------------
          u64 pc[kWM];
          u32 pp[kWM], pfc[kWM], pmw[kWM], pgn[kWM];   // payload (kWNonePay: no row) | front cpu | mem, len, type | GRES counts
          u32 pdip = 0;                                // bit m: row m has a dip (its start-now test needs the tile: the single-job exchange)
#pragma unroll
          for (u32 m = 0; m < kWM; ++m) {
            pp[m] = gr[2u * m].y & 0x3FFFFFFFu;
            pdip |= ((gr[2u * m].y >> 30) & 1u) << m;
            pc[m] = ((u64)gr[2u * m].w << 32) | gr[2u * m].z;
            pfc[m] = gr[2u * m + 1u].y; pmw[m] = gr[2u * m + 1u].z; pgn[m] = gr[2u * m + 1u].w;
          }
          u64 bndc; u32 bndp;          // the least bound: no row outside the pool has a key below it
          {
            u32 bp = gb.y & 0x7FFFFFFFu;
            u64 bc = ((u64)gb.w << 32) | gb.z;
            if (bp == kWNonePay) { bp = kNone; bc = ~0ull; }
            wave_argmin(bc, bp);
            bndc = bc; bndp = bp;
          }
          WINP_T(w3);
          // ---- the jobs, one after the other, on the pool ----------------------------------------------------------------------------------------
          u32 wdone = 0;
          bool wopen = true, wfull = false;   // wfull: closed because it is full (the next job may open a window at once)
          while (wopen) {
#pragma unroll
            for (u32 i = 0; i < kWB; ++i) {
              if (wopen) {
                const u32 jx = pos;
                if (wdone >= win_max) { wopen = false; wfull = true; }
                else if (!shaped(rl32(wq[i], kJsHead), jx)) wopen = false;
                else {
                  u64 tyok;
                  const ScanJob S = decode(wq[i], tyok);
                  const u32 gmode = S.gmode();
                  u32 gme = 0, gmo = 0;
                  if (gmode != 0u && gmode < 4u && (gmode & 2u)) { gme = uni32(s_nme[(S.gsel() >> 8) & (u32)(kMaxNames - 1)]); gmo = uni32(s_nmo[(S.gsel() >> 8) & (u32)(kMaxNames - 1)]); }
                  // this lane's cheapest row the job can start on now (type, front cpu / memory / GRES: the row loop's test)
                  u64 lc = ~0ull;
                  u32 lp = kNone, lm = 0;
#pragma unroll
                  for (u32 m = 0; m < kWM; ++m) {
                    const u32 g = pgn[m];
                    bool a = (pp[m] != kWNonePay) & (((tyok >> (pmw[m] >> 26)) & 1ull) != 0) & (S.rc32 <= (int)pfc[m]) & (S.rm16() <= (pmw[m] & 0xFFFFu));
                    if (gmode != 0u && gmode < 4u) {
                      if (gmode & 1u) a = a & (((g >> (S.gsel() & 0xFFu)) & 15u) >= (S.gneed() & 0xFFu));
                      if (gmode & 2u) {
                        const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
                        a = a & (__builtin_amdgcn_sad_u8(ce & gme, 0u, __builtin_amdgcn_sad_u8(co & gmo, 0u, 0u)) >= (S.gneed() >> 8));
                      }
                    } else if (gmode >= 4u) {
                      const u32 rqe = S.rq & 0x0F0F0F0Fu, rqo = (S.rq >> 4) & 0x0F0F0F0Fu;
                      const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
                      a = a & ((((ce | G8) - rqe) & G8) == G8) & ((((co | G8) - rqo) & G8) == G8);
#pragma unroll
                      for (int nm = 0; nm < kMaxNames; ++nm) {
                        const u32 tot = (S.gtot >> (8 * nm)) & 0xFFu;
                        const u32 have = __builtin_amdgcn_sad_u8(ce & s_nme[nm], 0u, __builtin_amdgcn_sad_u8(co & s_nmo[nm], 0u, 0u));
                        a = a & ((tot == 0) | (have >= (tot > 15u ? 15u : tot)));
                      }
                    }
                    const bool t = a & ((pc[m] < lc) | ((pc[m] == lc) & (pp[m] < lp)));
                    lc = t ? pc[m] : lc; lp = t ? pp[m] : lp; lm = t ? m : lm;
                  }
                  u64 mc = lc;
                  u32 mp = lp;
                  wave_argmin(mc, mp);
                  const bool below = (mc < bndc) | ((mc == bndc) & (mp < bndp));
                  const bool wl = (lc == mc) & (lp == mp);
                  const bool dipped = mp != kNone && __any(wl & (((pdip >> lm) & 1u) != 0u));
                  if (mp == kNone || !below || dipped) wopen = false;   // nothing in the pool | a row outside it may come first | the row has a dip: the single-job exchange decides
                  else {
                    // every wave: the row as this job leaves it (MinCpuTimeRatioFirst::UpdateCost + the front minus the allocation: pre_sel's arithmetic)
                    u32 cw = 0, cg = 0, cfc = 0;
#pragma unroll
                    for (u32 m = 0; m < kWM; ++m)
                      if (lm == m) { cw = pmw[m]; cg = pgn[m]; cfc = pfc[m]; }
                    const RowVal v = pre_sel_vals(S, mc, mp & 63u, true, cw, cg, (int)cfc);
                    const u64 nck = cost_key(v.ucost);
#pragma unroll
                    for (u32 m = 0; m < kWM; ++m) {
                      const bool u = wl & (lm == m);
                      pc[m] = u ? nck : pc[m]; pmw[m] = u ? v.w : pmw[m]; pgn[m] = u ? v.g : pgn[m]; pfc[m] = u ? (u32)v.fc : pfc[m];
                    }
                    const u64 wmask = __ballot(wl);
                    if ((wmask >> sid) & 1ull) {   // this wave's row: the decision for the supervisor, and the tile
                      const u32 wcode = mp >> 6;
                      put_decision(nex & (kWRing - 1), nex + 1u, 0, mp | (1u << kWdKShift) | (1u << kWdNfShift), mc);
                      RowVal o;
                      o.ucost = __longlong_as_double((long long)rl64(nck, sid));
                      o.w = rl32(v.w, sid); o.g = rl32(v.g, sid); o.fc = (int)rl32((u32)v.fc, sid);
                      put_sel(wcode, o);
                      if (wcode == tp_c) tvalid = false;   // the cached T argmin got more expensive
                    }
                    ++nex; ++pos; ++wdone;
                  }
                }
              }
            }
            if (wopen) {   // the next chunk of records
#pragma unroll
              for (u32 s = 0; s + kWB < kWQ; ++s) wq[s] = wq[s + kWB];
#pragma unroll
              for (u32 s = kWQ - kWB; s < kWQ; ++s) wq[s] = fetch_job(P, jbeg + (pos + s < njobs ? pos + s : njobs - 1u));
              wq_pos = pos;
            }
          }
          {
            WINP_T(w4);
            WINP_CNT(0); WINP_ADD(1, w0, w1); WINP_ADD(2, w1, w2); WINP_ADD(3, w2, w3); WINP_ADD(4, w3, w4);
#ifdef CNS_PROF_WIN
            wa[10] += wdone;
#endif
          }
          ++n_win; n_winjobs += wdone; n_windry += wdone == 0u ? 1u : 0u;
          // a window pays for its exchange from about kWYield jobs on: after a poorer one the next windows wait, twice as long each time (a queue of
          // backfills, of GRES requests the cheap rows cannot serve, of multi-node jobs in between); a good one opens the next at once
          if (wdone >= kWYield) { wback = wfull ? 0u : 1u; wpen = 4u; }   // (the job that closed it goes through the single-job exchange now)
          else { wpen = wpen < 512u ? wpen * 2u : 512u; wback = wpen; }
          {   // the record of the job at `pos` is in the queue: hand it to the loops below
            const u32 qi = pos - wq_pos;
            raw = qi == 0u ? wq[0] : (qi == 1u ? wq[1] : (qi == 2u ? wq[2] : wq[3]));
            have_raw_j = pos < njobs ? pos : kNone; dec_j = kNone;
          }
          continue;
        }
        // one job through the loops below, from the queue's record
        raw = wq[0]; have_raw_j = pos; dec_j = kNone;
      }
#endif
#if !defined(CNS_WIDE_NO_FAST_K1) && (!defined(CNS_PROF) || defined(CNS_PROF_HOME_ONLY))   // (-DCNS_WIDE_NO_FAST_K1: round 3's single loop, for A/B runs)
      // ---- THE STEADY STATE IN A LOOP OF ITS OWN ----------------------------------------------------------------------------
      // node_num == 1 jobs whose res_total set is static (no node lists, not exclusive): the same exchange as below, granule for granule,
      // with the A/B switches resolved, no probes, and nothing but what such a job needs inside the loop.  Any other job leaves
      // the loop where it is met — decoded, its successor's record in flight — and the general code takes it from there.
      // (Round 6: a wave with DIPS runs the loop too, with the dip filter in its rows.  Rounds 4-5 sent it through the general code, granule
      // for granule the same exchange — and after the first misprediction of a cycle that recorded a dip, a few waves of the partition were
      // on the slower path for the rest of the queue, with everybody else waiting for them at every exchange: C4 gained nothing from the
      // loop in round 4 — 269 -> 267 ms where C5, which never mispredicts, went 217 -> 190.  Only in the instantiation WITHOUT the window path:
      // the queues that get the other one — >= 95 % one-node jobs without GRES — mispredict next to never, and the three more row loops
      // cost their single-job exchanges 5 - 8 % by being there: C5 146.6 -> 153.7 ms, C2 114.2 -> 122.3, profiles/r06_ab_fast_loop_dips.txt.)
      constexpr bool kFastDips = !kWinK;
      if (P.wide_inject_stall == 0u && (kFastDips || !any_dip)) {
        bool f_abort = false;
#ifdef CNS_WIDE_WIN_ON
        const u32 f_first = pos;
#endif
        for (;;) {
          const u32 fj = pos;
          if (fj >= njobs) break;
#ifdef CNS_WIDE_WIN_ON
          if (win_max >= 2u && wback == 0u && fj != f_first) break;   // (a window may open in front of this job: every wave looks, at the loop's top)
#endif
          FPROF_T(f0);
          if (dec_j == fj) { J = Jn; typeok = typeok_n; }
          else {
            if (have_raw_j != fj) raw = fetch_job(P, jbeg + fj);
            J = decode(raw, typeok);
            if (fj + 1 < njobs) { raw = fetch_job(P, jbeg + fj + 1); have_raw_j = fj + 1; }
            else have_raw_j = kNone;
          }
          dec_j = kNone;
          const bool fast = J.k() == 1 && (J.shape() & 15u) == 6u && !(J.flags() & (kJfExclusive | kJfIncl | kJfExcl)) && fj != xj;
          if (!fast) { Jn = J; typeok_n = typeok; dec_j = fj; break; }   // (the general code finds it decoded)
          const u32 hreq = uni32(hreq_n);
          { const u32 snu = uni32(sn_n); sn = snu > sn ? snu : sn; }
          if (leader) { hreq_n = gld_raw(&ctl->halt); sn_n = gld_raw(&ctl->sup_nex); }
          FPROF_T(fs0);
          // ---- rows: the start-now argmin, and the res_total argmin when the cached one went stale ------------------------
          // (a job whose res_total set does not cover this wave's node types — a GRES job on a wave that also holds plain nodes —
          // filters the rows by type and takes its T argmin afresh: the cached one is that of the jobs every type fits)
          const bool tyall = (typeok & wave_types) == wave_types;
          const bool lean = tvalid && tyall;
          RM bl = okbits;
          if (!tyall) {
            RM tybits = 0;
#pragma unroll
            for (int r = 0; r < NPL; ++r) tybits |= (RM)((typeok >> (mw[r] >> 26)) & 1ull) << r;
            bl = okbits & tybits;
          }
          u64 ac = ~0ull, tcs = ~0ull;
          u32 ar = 0xFFu, tr = 0xFFu;
          {
            const u32 gmode = J.gmode();
            u32 gme = 0, gmo = 0;
            if (gmode & 2u) { gme = uni32(s_nme[J.gsel() >> 8]); gmo = uni32(s_nmo[J.gsel() >> 8]); }
            const u32 sh1 = J.gsel() & 0xFFu, need1 = J.gneed() & 0xFFu, need2 = J.gneed() >> 8;
            const u32 rqe = J.rq & 0x0F0F0F0Fu, rqo = (J.rq >> 4) & 0x0F0F0F0Fu;
            const u32 rm16 = J.rm16();
            auto frows = [&](auto mode, auto diptag) __attribute__((always_inline)) {
              constexpr u32 M = decltype(mode)::value;
              constexpr bool kDip = decltype(diptag)::value != 0;     // some row of this wave has a dip (else the test is not even compiled in)
              // the request's GRES part against per-class counts `g` (8 saturating nibbles): the front's, or the dip's
              auto gfit = [&](u32 g) __attribute__((always_inline)) -> bool {
                bool ok = true;
                if (M == 1) {
                  if (gmode & 1u) ok = ok & (((g >> sh1) & 15u) >= need1);
                  if (gmode & 2u) {
                    const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
                    ok = ok & (__builtin_amdgcn_sad_u8(ce & gme, 0u, __builtin_amdgcn_sad_u8(co & gmo, 0u, 0u)) >= need2);
                  }
                }
                if (M == 4) {
                  const u32 ce = g & 0x0F0F0F0Fu, co = (g >> 4) & 0x0F0F0F0Fu;
                  ok = ok & ((((ce | G8) - rqe) & G8) == G8) & ((((co | G8) - rqo) & G8) == G8);
#pragma unroll
                  for (int n = 0; n < kMaxNames; ++n) {
                    const u32 tot = (J.gtot >> (8 * n)) & 0xFFu;
                    const u32 have = __builtin_amdgcn_sad_u8(ce & s_nme[n], 0u, __builtin_amdgcn_sad_u8(co & s_nmo[n], 0u, 0u));
                    ok = ok & ((tot == 0) | (have >= (tot > 15u ? 15u : tot)));
                  }
                }
                return ok;
              };
#pragma unroll
              for (int r = 0; r < NPL; ++r) {
                const bool b = ((bl >> r) & 1u) != 0;
                bool a = b & (J.rc32 <= fcpu[r]) & (rm16 <= (mw[r] & 0xFFFFu));
                if (M != 0) a = a & gfit(gn[r]);
                if (kDip) {   // a window that reaches the node's dip must fit the dip too: a second necessary condition (scan_job's)
                  const u32 loff = J.L >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (u32)J.L;   // an entry t seconds after now lies in the window iff t < L (:6279)
                  const u32 rcpus = (u32)J.rc32 >> 8;                              // whole cpus of the request, rounded down
                  bool fits = (rcpus <= (dpc[r] >> 16)) & (rm16 <= (dpc[r] & 0xFFFFu));
                  if (M != 0) fits = fits & gfit(dpg[r]);
                  a = a & ((dpt[r] >= loff) | fits);
                }
                const u64 ck = cost_key(cost[r]);
                const bool ta = a & (ck < ac);
                ac = ta ? ck : ac;
                ar = ta ? (u32)r : ar;
                if (!lean) {
                  const bool tt = b & (ck < tcs);
                  tcs = tt ? ck : tcs;
                  tr = tt ? (u32)r : tr;
                }
              }
            };
            bool dipped = false;
            if constexpr (kFastDips) {
              if (any_dip) {   // (rare outside loaded clusters: only after a misprediction recorded one on a node of this wave)
                dipped = true;
                if (gmode == 0) frows(ModeTag<0>{}, ModeTag<1>{});
                else if (gmode < 4) frows(ModeTag<1>{}, ModeTag<1>{});
                else frows(ModeTag<4>{}, ModeTag<1>{});
              }
            }
            if (!dipped) {
              if (gmode == 0) frows(ModeTag<0>{}, ModeTag<0>{});
              else if (gmode < 4) frows(ModeTag<1>{}, ModeTag<0>{});
              else frows(ModeTag<4>{}, ModeTag<0>{});
            }
          }
          u32 ap = ar == 0xFFu ? kNone : ((ar << kWShift) | gt);
          u32 tp = tr == 0xFFu ? kNone : ((tr << kWShift) | gt);
          const u32 e = nex + 1u;
          const u32 xs = nex & (kWRing - 1);
          FPROF_T(fs1);
          if (leader) lap_guard(1u);
          u32 tpay;
          if (lean) {
            if (__any(ap != kNone)) wave_argmin(ac, ap);
            ap = uni32(ap);
            tcs = tc_c; tp = tp_c; tpay = tpay_c;
          } else {
            wave_argmin2(ac, ap, tcs, tp);
            ap = uni32(ap);
            tp = uni32(tp);
          }
          FPROF_T(fs2);
          if (!lean) {
            tpay = pay_of(tp);
            if (tyall) { tc_c = uni64(tcs); tp_c = tp; tpay_c = tpay; tvalid = true; }
          }
          const u32 apay = pay_of(ap);
#ifdef CNS_PROF_FAST
          fa_seg[0] += (u64)(fs0 - f0); fa_seg[1] += (u64)(fs1 - fs0); fa_seg[2] += (u64)(fs2 - fs1);
#endif
          // ---- publish: lane 0 the A granule, lane 1 the T granule ---------------------------------------------------------
          if (lane < 2u) {
            u32x4 v;
            v.x = e;
            if (lane == 0) { v.y = apay | ((leader && hreq) ? 0x80000000u : 0u); v.z = (u32)ac; v.w = (u32)(ac >> 32); }
            else { v.y = tpay; v.z = (u32)tcs; v.w = (u32)(tcs >> 32); }
            gran_st(rs_xr, (xs * kWXrow + (lane == 0 ? sid : (u32)kWSW + sid)) * 16u, v, near);
          }
          // ---- the next job's record -> scalars (its load went out a whole job ago); the one after it goes out BEHIND the first poll
          if (have_raw_j == fj + 1) {
            Jn = decode(raw, typeok_n);
            dec_j = fj + 1;
            have_raw_j = fj + 2 < njobs ? fj + 2 : kNone;
          }
          FPROF_T(f1);
          XrGran g = xr_ld(rs_xr, xs, lane);
          raw = fetch_job(P, jbeg + (fj + 2 < njobs ? fj + 2 : njobs - 1u));
          // ... and in the shadow of the first poll's loads: what this wave's OWN candidate would do to its row (if it wins)
          RowVal k1pre;
          k1pre.ucost = 0.0; k1pre.w = 0; k1pre.g = 0; k1pre.fc = 0;
          if (ap != kNone) k1pre = pre_sel(J, ap, ac, apay & 63u, true);
          else if (tp != kNone) k1pre = pre_sel(J, tp, tcs, tpay & 63u, false);
#ifdef CNS_PROF_FAST
          if (xr_ready(g, e)) ++fa_fr;
#endif
          if (!xr_ready(g, e)) {
            for (u32 spin = 0;; ++spin) {
              __builtin_amdgcn_s_sleep(CNS_WIDE_POLL_NAP);
              g = xr_ld(rs_xr, xs, lane);
              if (xr_ready(g, e)) break;
              if ((spin & 63u) == 63u) {
                if (gld(&ctl->abort)) { f_abort = true; break; }
                if (spin > kWSpinLimit) { wide_fault(P, ctl, 28, nex, sid, 0); f_abort = true; break; }
              }
            }
            if (f_abort) break;
          }
          FPROF_T(f2);
          ++nex;
          if (xr_halt(g)) {   // halted in front of job fj: nothing applied
            if (leader) put_decision(xs, e, 0, kWdHalt | kWdNone | (1u << kWdKShift), 0);
            have_raw_j = kNone; dec_j = kNone; stop_at(fj);
            break;
          }
          // ---- the decision: is this wave's own published candidate the one nobody's entry comes before? -----------------------
          {
            u64 c; u32 p;
            xr_entry(g, lane, c, p);
            u64 oc = ~0ull;
            u32 op = kNone;
            if (ap != kNone) { oc = ac; op = apay; }
            else if (tp != kNone) { oc = tcs | (1ull << 63); op = tpay; }
            const bool before = (c < oc) | ((c == oc) & (p < op));
            if (op != kNone && !__any(before)) {
              const bool bf = (oc >> 63) != 0;
              put_decision(xs, e, 0, op | (1u << kWdKShift) | (1u << kWdNfShift) | (bf ? kWdBackfill : 0u), oc & ~(1ull << 63));
              const u32 wcode = uni32(op) >> 6;
              put_sel(wcode, k1pre);
              if (wcode == tp_c) tvalid = false;   // the cached T argmin got more expensive
#ifdef CNS_PROF_FAST
              fa_won |= 2u;
#endif
            } else if (leader && !__any(p != kNone)) put_decision(xs, e, 0, kWdNone | (1u << kWdKShift), 0);   // nobody has a candidate: "Resource"
          }
#ifdef CNS_PROF_FAST
          {
            FPROF_T(f3);
            const u32 w = fa_won & 1u;
            fa_pub[w] += (u64)(f1 - f0); fa_wait[w] += (u64)(f2 - f1); fa_dec[w] += (u64)(f3 - f2); fa_cnt[w] += 1; fa_nl += lean ? 0u : 1u;
            fa_won >>= 1;
          }
#endif
          ++pos;
#ifdef CNS_WIDE_WIN_ON
          if constexpr (kWinTile) win_single_done();
#endif
        }
        if (f_abort) break;
        if (!running) continue;
#ifdef CNS_WIDE_WIN_ON
        if (win_max >= 2u && wback == 0u && pos != f_first) continue;
#endif
      }
#endif
      const u32 j = pos;
      if (j >= njobs) { stop_at(j); continue; }
      if (dec_j == j) { J = Jn; typeok = typeok_n; }   // decoded while the previous exchange was in flight
      else {
        if (have_raw_j != j) raw = fetch_job(P, jbeg + j);
        J = decode(raw, typeok);
        if (j + 1 < njobs) { raw = fetch_job(P, jbeg + j + 1); have_raw_j = j + 1; }   // in flight during this scan
        else have_raw_j = kNone;
      }
      dec_j = kNone;
      const bool piped = !(J.flags() & kJfExclusive) && (J.shape() & 11u) == 2u && J.k() >= 1 && J.k() <= (u32)kPMaxK;
      if (!piped) { have_raw_j = kNone; dec_j = kNone; stop_at(j); continue; }   // the home workgroup runs it through the sequential protocol
      const u32 hreq = uni32(hreq_n);   // (a halt request is honoured one job later; a stale sup_nex is merely conservative)
      { const u32 snu = uni32(sn_n); sn = snu > sn ? snu : sn; }
      if (leader) { hreq_n = gld_raw(&ctl->halt); sn_n = gld_raw(&ctl->sup_nex); }   // in flight during this job (made uniform where they are used)
      u64 ac = ~0ull, tcs = ~0ull;
      u32 ap = kNone, tp = kNone;
      // jobs whose T set is static: node_num == 1, satisfiable, no node lists (T then follows from the allowed types)
      const bool stat = J.k() == 1 && (J.shape() & 4u) && !(J.flags() & (kJfExclusive | kJfIncl | kJfExcl));
      const bool lean = stat && tvalid && (typeok & wave_types) == wave_types && j != xj;
      scan_job(J, jbeg + j, typeok, lean, bmask, amask, ac, ap, tcs, tp);
      if (j == xj) {   // the redo of a flushed job: candidates whose exact test already failed are out of the start-now set
        const u32 xn = gld(&ctl->excl_n);
        for (u32 x = 0; x < xn && x < 15u; ++x) {
          const u32 code = gld(&ctl->excl_code[x]);
          if ((code & (kWLanes - 1u)) == gt) amask &= ~(kOne << (code >> kWShift));
        }
        lane_argmin(amask, ac, ap);
        xj = kNone;
      }
      const u32 e = nex + 1u;
      u32 xs = nex & (kWRing - 1);
      WPROF_T(q1);
      if (leader) lap_guard(1u);
      WPROF_T(q2);
      if (leader) { WPROF_ADD(16, q0, q1); WPROF_ADD(17, q1, q2); }   // leader: fetch + decode + row loop | waiting for the supervisor (ring lap)
      u32 dkind = kPkFail, nfound = 0, lsel = 0;
      u64 mycost = ~0ull;
      u32 mypay = kNone;
      const u32 k = J.k();
      RowVal k1pre;
      k1pre.ucost = 0.0; k1pre.w = 0; k1pre.g = 0; k1pre.fc = 0;
      if (k == 1) {
        u32 tpay;
        if (lean) {
          if (__any(ap != kNone)) wave_argmin(ac, ap);   // (else: every lane already holds "none")
          ap = uni32(ap);
          tcs = tc_c; tp = tp_c; tpay = tpay_c;
        } else {
          wave_argmin2(ac, ap, tcs, tp);   // both cascades in one pass
          ap = uni32(ap);
          tp = uni32(tp);
          tpay = pay_of(tp);
          if (stat && (typeok & wave_types) == wave_types) { tc_c = uni64(tcs); tp_c = tp; tpay_c = tpay; tvalid = true; }
        }
        const u32 apay = pay_of(ap);
        WPROF_T(qa);
        // ---- publish: lane 0 the A granule, lane 1 the T granule ------------------------------------------------
        const bool lost = leader && part == 0 && P.wide_inject_stall == j + 1u;   // test hook: this wave's granules never arrive
        if (lane < 2u && !lost) {
          u32x4 v;
          v.x = e;
          if (lane == 0) { v.y = apay | ((leader && hreq) ? 0x80000000u : 0u); v.z = (u32)ac; v.w = (u32)(ac >> 32); }
          else { v.y = tpay; v.z = (u32)tcs; v.w = (u32)(tcs >> 32); }
          gran_st(rs_xr, (xs * kWXrow + (lane == 0 ? sid : (u32)kWSW + sid)) * 16u, v, near);
        }
        // ---- while the granules travel: what this wave's OWN candidate would do to its row (if it wins) ------------
        // ... and the next job's record -> scalars (its load was issued a whole job ago), the one after it -> in flight
        if (have_raw_j == j + 1) {
          Jn = decode(raw, typeok_n);
          dec_j = j + 1;
          have_raw_j = j + 2 < njobs ? j + 2 : kNone;   // (its load goes out BEHIND the first poll's, below)
        }
        // ---- wait until all 64 granules of the exchange carry its tag -------------------------------------------
        XrGran g;
        bool okx = true;
        WPROF_T(qb);
        // The first poll, peeled by hand (behind a branch inside the loop the compiler's wait counters fall back to vmcnt(0)):
        g = xr_ld(rs_xr, xs, lane);
        // ... and BEHIND its loads the record after the next one: vector loads return in order, so a record fetch issued just in
        // FRONT of the poll makes the poll wait for a trip to HBM.  Unconditional, with a clamped index, for the same reason.
        raw = fetch_job(P, jbeg + (j + 2 < njobs ? j + 2 : njobs - 1u));
        if (ap != kNone) k1pre = pre_sel(J, ap, ac, apay & 63u, true);          // (in the shadow of the first poll's loads)
        else if (tp != kNone) k1pre = pre_sel(J, tp, tcs, tpay & 63u, false);
        if (leader) WPROF_CNT(13);
        if (!xr_ready(g, e))
        for (u32 spin = 0;; ++spin) {
          __builtin_amdgcn_s_sleep(CNS_WIDE_POLL_NAP);
          g = xr_ld(rs_xr, xs, lane);
          if (leader) WPROF_CNT(13);
          if (xr_ready(g, e)) break;
          if ((spin & 63u) == 63u) {
            if (gld(&ctl->abort)) { okx = false; break; }
            if (spin > kWSpinLimit) { wide_fault(P, ctl, 28, nex, sid, 0); okx = false; break; }
          }
        }
        if (!okx) break;
        ++nex;
        WPROF_T(q3);
        if (leader) { WPROF_ADD(18, q2, q3); WPROF_ADD(10, q2, qa); WPROF_ADD(11, qa, qb); WPROF_ADD(12, qb, q3); }   // leader: wave argmins | publish + own-row arithmetic + next record | exchange wait
        if (xr_halt(g)) {   // halted in front of job j: nothing applied
          if (leader) put_decision(xs, e, 0, kWdHalt | kWdNone | (1u << kWdKShift), 0);
          have_raw_j = kNone; dec_j = kNone; stop_at(j); continue;
        }
        // ---- the decision: start now on the A argmin, else backfill on the T argmin, else fail.  A scanner wave does not
        // need the winner, only whether its OWN published candidate is it: nobody's entry may come before it in (cost key,
        // code) order, T entries behind every A entry.  One compare per lane and one vote instead of an argmin cascade (the
        // supervisor, which needs the winner, still takes the argmin — off the chain).
        u64 c; u32 p;
        xr_entry(g, lane, c, p);
        {
          u64 oc = ~0ull;
          u32 op = kNone;
          if (ap != kNone) { oc = ac; op = apay; }
          else if (tp != kNone) { oc = tcs | (1ull << 63); op = tpay; }
          const bool before = (c < oc) | ((c == oc) & (p < op));
          if (op != kNone && !__any(before)) {
            dkind = (oc >> 63) ? (u32)kPkBackfill : (u32)kPkStart;
            mypay = op; mycost = oc & ~(1ull << 63); nfound = 1;   // (only the winning wave leaves with nfound == 1)
            // ... and it tells the supervisor (which no longer re-derives the decision from the 128 granules)
            put_decision(xs, e, 0, mypay | (1u << kWdKShift) | (1u << kWdNfShift) | (dkind == (u32)kPkBackfill ? kWdBackfill : 0u), mycost);
            // ... and writes what it computed during the exchange into its row — HERE, where the winner's code is a scalar: behind the
            // merge with the node_num > 1 path (`mypay`: a list, one entry per lane) the compiler takes it for divergent, and with it
            // `tvalid`, `lean` and the branches of the next job's scan that depend on them (exec-masked instead of scalar)
            const u32 wcode = uni32(op) >> 6;
            put_sel(wcode, k1pre);
            if (wcode == tp_c) tvalid = false;   // the cached T argmin got more expensive
          } else if (leader && !__any(p != kNone)) put_decision(xs, e, 0, kWdNone | (1u << kWdKShift), 0);   // nobody has a candidate: "Resource"
        }
        WPROF_T(qd);
        if (leader) WPROF_ADD(14, q3, qd);   // leader: the decision (argmin over the granules)
      } else {
        u64 lc = ~0ull, tc2 = ~0ull;     // this wave's own lists (start-now / res_total): lane i holds entry i
        u32 lp = kWNonePay, tp2 = kWNonePay;
        ListGran LG;
        WPROF_T(l0);
        post_lists(xs, e, amask, bmask, k, (leader && hreq) ? 1u : 0u, lc, lp, tc2, tp2);
        WPROF_T(l1);
        u32 halt = 0;
        if (!wait_lists(xs, e, k, LG, halt)) break;
        WPROF_T(l2);
        ++nex;
        if (halt) {
          if (leader) put_decision(xs, e, 0, kWdHalt | kWdNone | (k << kWdKShift), 0);
          have_raw_j = kNone; dec_j = kNone; stop_at(j); continue;
        }
        nfound = vote_lists(LG, k, lc, lp, lsel, xs, e);
        WPROF_T(l3);
        if (leader) { WPROF_CNT(0); WPROF_ADD(1, l0, l1); WPROF_ADD(2, l1, l2); WPROF_ADD(3, l2, l3); }   // leader, node_num > 1: jobs | building the lists | waiting for the exchange | vote
        dkind = kPkStart;
        if (nfound != k) {   // fewer than k nodes can start it now -> first k by res_total + backfill (:6335-6376)
          xs = nex & (kWRing - 1);
          if (leader) lap_guard(1u);
          const u32 e2 = nex + 1u;
          publish_list(xs, e2, tc2, tp2, k, 0u);
          u32 h2 = 0;
          if (!wait_lists(xs, e2, k, LG, h2)) break;
          ++nex;
          lc = tc2; lp = tp2;
          nfound = vote_lists(LG, k, lc, lp, lsel, xs, e2);
          dkind = nfound == k ? (u32)kPkBackfill : (u32)kPkFail;
          WPROF_T(l4);
          if (leader) { WPROF_CNT(4); WPROF_ADD(5, l3, l4); }   // leader: second list exchanges | their time
        }
        mycost = lc; mypay = lp;   // (own entries; lsel says which of them are part of the selection)
      }
      if (k != 1 && nfound == k) {   // (node_num == 1: the winning wave wrote its row inside the exchange code above, where the winner's code is a scalar)
        for (u32 i = 0; i < k; ++i) {
          if (!((lsel >> i) & 1u)) break;   // (selected entries are a prefix of the own list)
          const u32 py = rl32(mypay, i);
          const u32 code = py >> 6;
          const u64 c0 = rl64(mycost, i);
          apply_sel(J, code, c0, py & 63u, dkind == kPkStart);
          if (code == tp_c) tvalid = false;   // the cached T argmin got more expensive
        }
      }
      ++pos;
#ifdef CNS_WIDE_WIN_ON
      if constexpr (kWinTile) win_single_done();
#endif
      WPROF_T(q4);
      if (leader) { WPROF_ADD(19, q0, q4); WPROF_CNT(20); }   // leader: whole job
    }
    // always on: polls the leader spent in front of a full ring (the scanners wait for the home workgroup)
    if (leader && lane == 0) P.prof[(size_t)P.num_parts * 32 + (size_t)part * kWsSlots + kWsLapWait] = n_lapwait;
#ifdef CNS_WIDE_WIN_ON
    if (leader && lane == 0) {
      u64* const st = P.prof + (size_t)P.num_parts * 32 + (size_t)part * kWsSlots;
      st[kWsWindows] = n_win; st[kWsWinJobs] = n_winjobs; st[kWsWinDry] = n_windry;
    }
#ifdef CNS_PROF_WIN
    if (lane == 0) {   // every wave adds its registers: [0] windows, [1..8] cycles by segment, [9] polls, [10] jobs decided
      unsigned long long* pr = (unsigned long long*)(P.prof + (size_t)part * 32);
#pragma unroll
      for (int x = 0; x < 12; ++x) atomicAdd(pr + x, (unsigned long long)wa[x]);
    }
#endif
#undef WINP_T
#undef WINP_ADD
#undef WINP_CNT
#undef CNS_WIDE_WIN_ON
#endif
#ifdef CNS_PROF_FAST
    if (lane == 0) {   // every wave: [0] jobs it did not win the predecessor of, [1] jobs right behind one it won
      unsigned long long* pr = (unsigned long long*)(P.prof + (size_t)part * 32);
      for (int w = 0; w < 2; ++w) {
        atomicAdd(pr + 0 + w, (unsigned long long)fa_cnt[w]); atomicAdd(pr + 2 + w, (unsigned long long)fa_pub[w]);
        atomicAdd(pr + 4 + w, (unsigned long long)fa_wait[w]); atomicAdd(pr + 6 + w, (unsigned long long)fa_dec[w]);
      }
      atomicAdd(pr + 8, (unsigned long long)fa_nl); atomicAdd(pr + 9, (unsigned long long)fa_fr);
      for (int x = 0; x < 3; ++x) atomicAdd(pr + 10 + x, (unsigned long long)fa_seg[x]);
    }
#endif
#ifdef CNS_WPROF_REGS_ON
    if (leader && lane == 0) {
#pragma unroll
      for (int x = 0; x < 32; ++x) P.prof[(size_t)part * 32 + x] += wacc[x];
    }
#undef CNS_WPROF_REGS_ON
#endif
  }
}

#undef s_posted
#undef s_claim
#undef s_retired
#undef s_flush_job
#undef s_abort
#undef s_allow
#undef s_homes
#undef s_wfm

#define CNS_WIDE_INSTANTIATE(w) template __global__ void k_wide<w, false>(const KParams, const KParams*);
CNS_WNPL_LIST(CNS_WIDE_INSTANTIATE)
#undef CNS_WIDE_INSTANTIATE
#ifdef CNS_WIDE_WINDOWS
template __global__ void k_wide<1, true>(const KParams, const KParams*);
template __global__ void k_wide<2, true>(const KParams, const KParams*);
#endif
#if CNS_WIDE_SPW * CNS_WIDE_WGS == 8
template __global__ void k_wide<1, false, kWMemWordsGiant>(const KParams, const KParams*);   // launch_mem above mem_slots
#endif

// Host side: what engine.hip needs to know about this build of the kernel (the file is included once per scanner-wave
// count, each time inside its own namespace).
struct WideInfo {
  static constexpr u32 group = (u32)kWGroup, waves = (u32)kWSW, lanes = kWLanes, npl_max = (u32)kWNplMax, max_parts = kWMaxParts, block = (u32)kWBlock;
  static constexpr u32 aux_max = kWAuxMax;      // extra home workgroups per partition at most (KParams::wide_aux)
  static constexpr u32 last_in_lds_rows = 4;    // ... which need the last-task table in LDS: tiles of up to 4 rows per lane
  static constexpr size_t ctl_bytes = sizeof(WideCtl);
  static constexpr u32 mem_slots = kWMs * 64u * kWMemWords;   // widest group the serial-only mode (KParams::serial_only) scans
  static constexpr u32 giant_mem_slots = kWMs * 64u * kWMemWordsGiant;   // ... and its giant instantiation (the 8-wave build only)
  // the serial-only mode's loop shapes (cns_serial_shape): scanner lanes and their rows per trip, mask words, a helper lane's slots per trip
  static constexpr u32 mem_lanes = kWMs, mem_trip = kWMsTrip, mem_words = kWMemWords, giant_mem_words = kWMemWordsGiant, giant_trip = kGiantTrip;
  static_assert(64u % kWMsTrip == 0u, "a trip's rows never straddle a mask word");
  // the tile widths (rows per lane) of this build, ascending, and how many of the first ones also have a windows build
#define CNS_WIDE_WIDTH(w) (u32)(w),
  static constexpr u32 widths[] = {CNS_WNPL_LIST(CNS_WIDE_WIDTH)};
#undef CNS_WIDE_WIDTH
#ifdef CNS_WIDE_WINDOWS
  static constexpr u32 window_widths = 2;
#else
  static constexpr u32 window_widths = 0;
#endif
  // the narrowest tile that holds `np` nodes per partition: the kernel and its name (nullptr: none)
  static const void* pick(u32 np, const char** name, bool windows = false) {
#ifdef CNS_WIDE_WINDOWS
    if (windows && np <= kWLanes) { *name = "k_wide<1> windows"; return (const void*)k_wide<1, true>; }
    if (windows && np <= kWLanes * 2u) { *name = "k_wide<2> windows"; return (const void*)k_wide<2, true>; }
#endif
#define CNS_WIDE_PICK(w) if (np <= kWLanes * (u32)(w)) { *name = "k_wide<" #w ">"; return (const void*)k_wide<w, false>; }
    CNS_WNPL_LIST(CNS_WIDE_PICK)
#undef CNS_WIDE_PICK
    return nullptr;
  }
};
#undef CNS_WNPL_LIST
#ifdef CNS_WIDE_WINDOWS
#undef CNS_WIDE_WINDOWS
#endif
#undef WPROF_T
#undef WPROF_ADD
#undef WPROF_CNT
