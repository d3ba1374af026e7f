// Kernels of include/crane_gpu_gate/pending_gate.h (the dependency-event drain and Phase 1 of ScheduleThread_, JobScheduler.cpp:1353-1413,
// for every job of the pending map at once).  Included by engine.hip; host side: gate_host.inc.
//
// A call:
//   (memset)        first_ev[D] = 0xFFFFFFFF                                                       (only when the call has events and entries)
//   k_gate_events   one thread per event: a bisection over job_id for the dependent (:1362), one over that job's list for the dependee
//                   (CtldPublicDefs.cpp:146); a hit at entry x claims it with atomicMin(first_ev[x], e).  The entry's first event in queue
//                   order is the one DependenciesInJob::update applies: it erases the entry (:159), the later ones find nothing.  The
//                   events without their job: a ballot per wave, one atomic per wave that has any.
//   k_gate_jobs     one workgroup per kGateChunk consecutive jobs, one lane per job.  A list of at most kGateLaneMax entries is walked by
//                   its lane; a longer one is handed to its wave, 64 entries per step, the fold by a wave min / max, the erased count by
//                   a ballot (k_cc_check's hand-off).  Then the first failing check in the reference's order; code, ready_sec, dep_erased,
//                   the per-wave count of OK jobs, the counts per code and of claimed entries.
//   k_sort_rowscan  (sort_kernels.inc, one workgroup: scan_counts of sort_call.inc) the exclusive scan of the per-wave counts, kGateScanSpan per step
//   k_gate_scatter  pending[base of the wave + rank inside the wave] = row: the flag again from code, the rank by mbcnt.  No atomic
//                   decides a position: the list is in row order whatever the schedule.
// No workgroup waits for another; the gate's own kernels use no LDS and no barrier; every store is a plain vector store or a returnless
// vector atomic.

#include "csr_dev.h"

namespace cns {

constexpr u32 kGateBlock = 256;
constexpr u32 kGateChunk = 256;      // jobs of one workgroup: one per lane
constexpr u32 kGateLaneMax = 8;      // dependency entries one lane walks alone (DESIGN.md 6)
constexpr u32 kGateScanSpan = kSortScanSpan;   // per-wave counts one step of k_sort_rowscan takes
constexpr u32 kGateUnclaimed = 0xFFFFFFFFu;

struct GateParams {
  u64 J;
  u32 D, E;
  i64 now;
  const u32* job_id;            // [J] strictly ascending
  const uint8_t* held;          // [J] or null
  const i64* begin;             // [J] or null
  const uint8_t* is_or;         // [J] or null: no job has dependencies
  const i64* ready;             // [J]
  const u64* dep_off;           // [J+1] or null: no entries
  const u32* dep_job;           // [D] ascending inside a list
  const u64* dep_delay;         // [D]
  const uint8_t* array_parent;  // [J] or null
  const uint8_t* ap_flags;      // [J]
  const i64* ap_deadline;       // [J]
  const u64* ap_running;        // [J]
  const u64* ap_limit;          // [J]
  const u32* ev_dependent;      // [E]
  const u32* ev_dependee;       // [E]
  const i64* ev_sec;            // [E]
  u32* first_ev;                // [D] or null: no event can claim an entry
  uint8_t* code;                // [J]
  i64* ready_out;               // [J]
  uint8_t* erased;              // [D]
  u32* wave_count;              // [4 * workgroups of k_gate_jobs]
  u32* pending;                 // [J]
  unsigned long long* counts;   // [16] jobs per code, then [16] claimed entries, [17] events without their job
};

// event_time + absl::Seconds(delay) (CtldPublicDefs.cpp:153): an infinite time stays, a delay >= 2^63 is +infinity, else the add saturates
__device__ __forceinline__ i64 gate_ready_of(i64 ev, u64 delay) {
  if (ev == INT64_MAX || ev == INT64_MIN) return ev;
  if (delay >> 63) return INT64_MAX;
  return ev > INT64_MAX - (i64)delay ? INT64_MAX : ev + (i64)delay;
}

__global__ __launch_bounds__(256) void k_gate_events(const GateParams P) {
  const u32 lane = threadIdx.x & 63u;
  const u64 e = (u64)blockIdx.x * kGateBlock + threadIdx.x;
  u32 miss = 0;   // 1: no such pending job (:1363), 2: no such dependency (CtldPublicDefs.cpp:147)
  if (e < P.E) {
    const u32 dj = P.ev_dependent[e];
    u64 lo = 0, hi = P.J;   // the first row with job_id >= dj
    while (lo < hi) {
      const u64 mid = lo + ((hi - lo) >> 1);
      if (P.job_id[mid] < dj) lo = mid + 1; else hi = mid;
    }
    if (lo >= P.J || P.job_id[lo] != dj) miss = 1;
    else if (!P.dep_off || !P.first_ev) miss = 2;
    else {
      const u32 de = P.ev_dependee[e];
      u64 b = P.dep_off[lo], en = P.dep_off[lo + 1];
      if (en > P.D) en = P.D;                        // (the host refused such offsets already)
      miss = 2;
      while (b < en) {
        const u64 mid = b + ((en - b) >> 1);
        const u32 v = P.dep_job[mid];
        if (v == de) { (void)atomicMin(&P.first_ev[mid], (u32)e); miss = 0; break; }
        if (v < de) b = mid + 1; else en = mid;
      }
    }
  }
  // (the events without their entry are not counted here: with the repeats, which do find an entry of the list as uploaded, they are
  // what is left of E beside the claimed entries and these)
  const unsigned long long mk = __ballot(miss == 1);
  if (lane == 0 && mk) (void)__hip_atomic_fetch_add(&P.counts[17], (unsigned long long)__popcll(mk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// entry x of a list folded into (acc, claimed): the event that claimed it, if any
__device__ __forceinline__ bool gate_entry(const GateParams& P, u64 x, bool is_or, i64& acc) {
  const u32 f = P.first_ev ? P.first_ev[x] : kGateUnclaimed;
  const bool claimed = f < P.E;
  if (claimed) {
    const i64 t = gate_ready_of(P.ev_sec[f], P.dep_delay[x]);
    acc = is_or ? (t < acc ? t : acc) : (t > acc ? t : acc);          // CtldPublicDefs.cpp:154-158
  }
  P.erased[x] = claimed ? 1 : 0;                                       // CtldPublicDefs.cpp:159
  return claimed;
}

__global__ __launch_bounds__(256) void k_gate_jobs(const GateParams P) {
  const u32 lane = threadIdx.x & 63u;
  const u64 j = (u64)blockIdx.x * kGateChunk + threadIdx.x;
  const bool valid = j < P.J;
  bool is_or = false;
  i64 ready = INT64_MIN;                                               // CtldPublicDefs.h:458
  u64 b = 0, e = 0;
  if (valid && P.is_or) {
    is_or = P.is_or[j] != 0; ready = P.ready[j];
    if (P.dep_off) { b = P.dep_off[j]; e = P.dep_off[j + 1]; if (e > P.D) e = P.D; if (b > e) b = e; }
  }
  u64 erased = 0;
  const bool wide = e - b > kGateLaneMax;
  if (!wide)
    for (u64 x = b; x < e; ++x) erased += gate_entry(P, x, is_or, ready) ? 1u : 0u;
  // the long lists of this wave, one after the other, 64 entries per step
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const bool o_or = __shfl((int)is_or, owner) != 0;
    const u64 ob = (u64)__shfl((unsigned long long)b, owner), oe = (u64)__shfl((unsigned long long)e, owner);
    i64 acc = o_or ? INT64_MAX : INT64_MIN;                            // the fold's identity
    u64 n = 0;
    for (u64 base = ob; base < oe; base += 64) {
      const u64 x = base + lane;
      const bool claimed = x < oe && gate_entry(P, x, o_or, acc);
      n += (u64)__popcll(__ballot(claimed));
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const i64 t = (i64)__shfl_xor((long long)acc, off);
      acc = o_or ? (t < acc ? t : acc) : (t > acc ? t : acc);
    }
    if ((int)lane == owner) { ready = o_or ? (acc < ready ? acc : ready) : (acc > ready ? acc : ready); erased = n; }
  }
  const u64 remaining = (e - b) - erased;
  u32 code = CNS_GATE_OK;
  if (valid) {
    if (P.held && P.held[j]) code = CNS_GATE_HELD;                                                   // :1380
    else if (P.begin && P.begin[j] > P.now) code = CNS_GATE_BEGIN_TIME;                              // :1384
    else if (!((is_or || remaining == 0) && ready <= P.now))                                         // :1388, is_met
      code = (ready == INT64_MAX && (!is_or || remaining == 0)) ? CNS_GATE_DEPENDENCY_NEVER : CNS_GATE_DEPENDENCY;   // :1389-1393, is_failed
    else if (P.array_parent && P.array_parent[j]) {                                                  // :1397
      const u32 f = P.ap_flags[j];
      if ((f & (CNS_GATE_AP_HAS_META | CNS_GATE_AP_HAS_PARENT)) != (CNS_GATE_AP_HAS_META | CNS_GATE_AP_HAS_PARENT)) code = CNS_GATE_ARRAY_NO_META;   // Array.cpp:687, :237
      else if (f & CNS_GATE_AP_COMPLETE) code = CNS_GATE_ARRAY_COMPLETE;                             // Array.cpp:240
      else if (f & CNS_GATE_AP_CANCEL) code = CNS_GATE_ARRAY_CANCELLED;                              // Array.cpp:243
      else if (P.ap_deadline[j] <= P.now) code = CNS_GATE_ARRAY_DEADLINE;                            // Array.cpp:246
      else if (!(f & CNS_GATE_AP_HAS_NEXT)) code = CNS_GATE_ARRAY_NO_NEXT;                           // Array.cpp:249
      else if (P.ap_running[j] >= P.ap_limit[j]) code = CNS_GATE_ARRAY_TASK_LIMIT;                   // Array.cpp:255
      else code = CNS_GATE_OK_ARRAY_PARENT;                                                          // :1404-1408
    }
    P.code[j] = (uint8_t)code;
    P.ready_out[j] = ready;
  }
  const unsigned long long ok = __ballot(valid && code <= CNS_GATE_OK_ARRAY_PARENT);
  if (lane == 0) P.wave_count[(u64)blockIdx.x * (kGateBlock / 64) + (threadIdx.x >> 6)] = (u32)__popcll(ok);
  #pragma unroll
  for (u32 c = 0; c <= CNS_GATE_ARRAY_TASK_LIMIT; ++c) {
    const unsigned long long mk = __ballot(valid && code == c);
    if (lane == 0 && mk) (void)__hip_atomic_fetch_add(&P.counts[c], (unsigned long long)__popcll(mk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // claimed entries = applied events: the wave's sum, one atomic per wave that has any
  u64 applied = valid ? erased : 0;
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) applied += (u64)__shfl_xor((unsigned long long)applied, off);
  if (lane == 0 && applied) (void)__hip_atomic_fetch_add(&P.counts[16], (unsigned long long)applied, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave_base: the exclusive scan of k_gate_jobs' per-wave counts
__global__ __launch_bounds__(256) void k_gate_scatter(const uint8_t* __restrict__ code, u64 J, const u32* __restrict__ wave_base, u32* __restrict__ pending) {
  const u64 j = (u64)blockIdx.x * kGateChunk + threadIdx.x;
  const bool ok = j < J && code[j] <= CNS_GATE_OK_ARRAY_PARENT;
  const unsigned long long mk = __ballot(ok);
  const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(mk >> 32), __builtin_amdgcn_mbcnt_lo((u32)mk, 0u));   // OK lanes below this one
  if (ok) {
    const u64 pos = (u64)wave_base[(u64)blockIdx.x * (kGateBlock / 64) + (threadIdx.x >> 6)] + rank;
    if (pos < J) pending[pos] = (u32)j;   // (pos <= j: at most j OK rows come before row j)
  }
}

}  // namespace cns
