// Kernels of include/crane_gpu_commit/commit_check.h (the commit loop's resource-changed and preempted-still-alive checks,
// JobScheduler.cpp:1464-1555, for every job of the last cycle at once).  Included by engine.hip; host side: commit_host.inc.
//
// A call:
//   k_fill_i64  change[N] = INT64_MAX                                   (only when the call has node events)
//   k_cc_fold   one thread per (event, node) entry: change[node] = min(change[node], the event's time) — :1479-1483
//   k_cc_check  one workgroup per kCcChunk consecutive jobs of the queue, one lane per job: the first failing check in the reference's
//               order.  The cycle's results are read where they are (start, reason, the node of every placement record).  A job of at
//               most kCcLaneMax records is walked by its lane; a wider one is handed to its wave, which strides over the records 64 at
//               a time and decides with one ballot.  The code byte is written once per job; counts: a ballot per wave and code, one
//               atomic per wave and non-empty code.
// No workgroup waits for another, no LDS; every store is a plain vector store or a returnless vector atomic.

#include "csr_dev.h"

namespace cns {

constexpr u32 kCcBlock = 256;
constexpr u32 kCcChunk = 256;     // jobs of one workgroup: one per lane
constexpr u32 kCcLaneMax = 8;     // placement records one lane walks alone (DESIGN.md 6)
constexpr u32 kCcNoSlot = 0xFFFFFFFFu;
constexpr i64 kCcNever = INT64_MAX;

struct CcParams {
  u64 J;
  u32 N, V, A, R;
  // the cycle's results and tables (read only)
  const i64* start;           // [J]
  const uint8_t* reason;      // [J]
  const u64* place_off;       // [J+1]
  const u32* place_node;      // [place_off[J]]
  // the call
  const i64* limit;           // [J]
  const u32* resv;            // [J] or null
  const uint8_t* gone;        // [J] or null
  const i64* change;          // [N] or null: no node events
  const u32* resv_slot;       // [V] reservation -> affected slot or kCcNoSlot; null: no affected reservation
  const uint8_t* ar_exists;   // [A]
  const i64* ar_end;          // [A]
  const u64* ar_off;          // [A+1]
  const u32* ar_nodes;        // ascending inside a slot
  const u64* pre_off;         // [J+1] or null
  const u32* pre;             // job references
  const uint8_t* alive;       // [R]
  uint8_t* code;              // [J]
  unsigned long long* counts; // [8]
};

__global__ __launch_bounds__(256) void k_cc_fold(const i64* __restrict__ ev_time, const u64* __restrict__ ev_off, const u32* __restrict__ ev_nodes,
                                                 u32 E, u32 entries, u32 N, i64* __restrict__ change) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= entries) return;
  const u32 n = ev_nodes[i];
  if (n >= N) return;                         // (the host refused the call already)
  const u32 e = csr_owner(ev_off, E, (u64)i);
  (void)__hip_atomic_fetch_min((long long*)&change[n], (long long)ev_time[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one placement record against the job's test.  mode 1: outside every reservation, change[n] < end (:1516-1517).  mode 2: inside an
// affected reservation, n not in its current node list (:1530).  A record that carries CNS_NODE_NONE names no node.
__device__ __forceinline__ bool cc_record_fails(const CcParams& P, u32 mode, u32 n, i64 end, u64 lb, u64 le) {
  if (n == CNS_NODE_NONE) return false;
  if (mode == 1) return n < P.N && P.change[n] < end;
  return !sorted_contains(P.ar_nodes, lb, le, n);
}

__global__ __launch_bounds__(256) void k_cc_check(const CcParams P) {
  const u32 lane = threadIdx.x & 63u;
  const u64 j = (u64)blockIdx.x * kCcChunk + threadIdx.x;
  const bool valid = j < P.J;
  u32 code = CNS_COMMIT_OK;
  u32 mode = 0;                 // 0: no walk over the records, 1: node events, 2: the reservation's node list
  u64 rb = 0, re = 0, lb = 0, le = 0;
  i64 end = 0;
  if (valid) {
    if (P.gone && P.gone[j]) code = CNS_COMMIT_GONE;                                   // :1493-1500
    else if (P.reason[j] != 0) code = CNS_COMMIT_NOT_STARTED;                          // :1507-1510
    else {
      const i64 s = P.start[j], l = P.limit[j];
      end = l > 0 ? (s > kCcNever - l ? kCcNever : s + l) : (s < INT64_MIN - l ? INT64_MIN : s + l);   // :6772, saturating as absl::Time
      const u32 rv = P.resv ? P.resv[j] : CNS_RESV_NONE;
      rb = P.place_off[j]; re = P.place_off[j + 1];
      if (rv == CNS_RESV_NONE) {                                                       // :1512
        if (P.change) mode = 1;
      } else if (P.resv_slot && rv < P.V) {
        const u32 a = P.resv_slot[rv];
        if (a != kCcNoSlot) {                                                          // :1521
          if (!P.ar_exists[a]) code = CNS_COMMIT_RESV_DELETED;                         // :1524
          else if (P.ar_end[a] < end) code = CNS_COMMIT_RESV_ENDS_EARLY;               // :1526
          else { mode = 2; lb = P.ar_off[a]; le = P.ar_off[a + 1]; }
        }
      }
      if (re <= rb) mode = 0;
    }
  }
  bool hit = false;
  const bool wide = mode != 0 && re - rb > kCcLaneMax;
  if (mode != 0 && !wide)
    for (u64 x = rb; x < re; ++x) hit |= cc_record_fails(P, mode, P.place_node[x], end, lb, le);   // (no break: :1514-1520)
  // the wide jobs of this wave, one after the other, 64 records per step
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u32 m = (u32)__shfl((int)mode, owner);
    const u64 b = (u64)__shfl((unsigned long long)rb, owner), e = (u64)__shfl((unsigned long long)re, owner);
    const u64 l0 = (u64)__shfl((unsigned long long)lb, owner), l1 = (u64)__shfl((unsigned long long)le, owner);
    const i64 en = (i64)__shfl((long long)end, owner);
    bool any = false;
    for (u64 x = b + lane; x < e; x += 64) any |= cc_record_fails(P, m, P.place_node[x], en, l0, l1);
    const bool job_hit = __ballot(any) != 0ull;
    if ((int)lane == owner) hit = job_hit;
  }
  if (hit) code = mode == 1 ? CNS_COMMIT_RESOURCE_CHANGED : CNS_COMMIT_RESV_CHANGED;     // :1518, :1531
  if (valid && code == CNS_COMMIT_OK && P.pre_off) {                                     // :1542-1555
    const u64 pb = P.pre_off[j], pe = P.pre_off[j + 1];
    for (u64 x = pb; x < pe; ++x) {
      const u32 r = P.pre[x];
      if (r & CNS_PREEMPT_REF_PENDING) continue;                                         // :1545
      if (r < P.R && P.alive[r]) { code = CNS_COMMIT_WAITING_PREEMPTION; break; }        // :1546-1552
    }
  }
  if (valid) P.code[j] = (uint8_t)code;
  #pragma unroll
  for (u32 c = 0; c < 8; ++c) {
    const unsigned long long mk = __ballot(valid && code == c);
    if (lane == 0 && mk) (void)__hip_atomic_fetch_add(&P.counts[c], (unsigned long long)__popcll(mk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace cns
