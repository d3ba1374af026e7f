// Kernels of include/crane_gpu_resv/resv_probe.h (reservation what-ifs: JobScheduler::CreateResv_, JobScheduler.cpp:4383-4419, for Q
// requests at once, at a given start or at the earliest one).  Included by engine.hip; host side: resvq_host.inc.
//
// Tables per NODE (k_rq_latest + the host's CSR): latest_end[N], rv_off[N+1], rv_st / rv_ed sorted by (st, ed) inside a node.
// A call:
//   earliest mode only — (the host lays out the event slots: 1 + reservations on its node per found candidate, one segment per query)
//                        k_rq_emit   per candidate: the starts at which it BECOMES free (plus) and at which it stops being free (minus)
//                        one sort of all event times by (segment, time): the stable radix passes of sort_kernels.inc (k_sort_hist,
//                        k_sort_rowscan, k_sort_scatter: three kernels per 8-bit digit) over the time, k_rq_by_segment, the same passes
//                        over the segment number, k_rq_gather
//                        k_rq_first  per plus time: free count there = plus times <= t  -  minus times <= t; the least t with count >= k
//   both modes         — k_rq_classify  one thread per (query, candidate): the code at the query's evaluated start
//                        k_rq_pick      one workgroup per query: the first k free candidates in list order, num_free, status
// No workgroup waits for another; every store is a plain vector store or a returnless vector atomic.

#include "csr_dev.h"

namespace cns {

constexpr i64 kRqNever = INT64_MAX;   // a time that is never reached (an infinite end), and the filler of unused event slots
constexpr u32 kRqBlock = 256;
constexpr u32 kRqPickGrid = 256;      // k_rq_pick: at most this many workgroups, each strides over the queries

struct RqParams {
  // tables
  u32 N;
  const i64* latest;
  const u32* rv_off;
  const i64* rv_st;
  const i64* rv_ed;
  // queries
  u32 Q;
  u32 L;                   // candidates of the call
  const i64* q_start;
  const i64* q_dur;
  const u32* q_k;          // node_num, or the list length
  const u32* q_flags;      // bit 0: earliest mode, bit 1: in the past
  const u32* cand_off;     // [Q+1]
  const u32* cand;         // [L]
  const u32* chosen_off;   // [Q+1] slot ranges of min(k, list length)
  // earliest mode
  u32 EV;                  // event slots of the call
  const u32* ev_off;       // [L+1] first slot per candidate (1 + reservations on its node for a found candidate of an earliest-start query)
  const u32* seg_off;      // [Q+1] = ev_off[cand_off[q]]
  u64* ev_key;             // [2 EV] event times as ascending unsigned keys: plus times in [0, EV), minus times in [EV, 2 EV)
  u32* ev_seg;             // [2 EV] their segment: q for a plus time, Q + q for a minus time
  const i64* plus_s; const i64* minus_s;   // sorted by (segment, time): plus_s[seg_off[q] ..), minus_s[seg_off[q] ..)
  i64* best;               // [Q] least feasible start, kRqNever: none (or not asked)
  // results
  uint8_t* code;           // [L]
  u32* chosen;             // [chosen_off[Q]]
  uint8_t* status; i64* o_start; u32* num_free;
};

__device__ __forceinline__ i64 rq_add_sat(i64 t, i64 d) { return t > kRqNever - d ? kRqNever : t + d; }   // d > 0
__device__ __forceinline__ i64 rq_sub_sat(i64 t, i64 d) { return t < INT64_MIN + d ? INT64_MIN : t - d; } // d >= 0

// latest_end[node] = max end over the allocations on it; one thread per allocation, its job by bisection of the CSR
__global__ __launch_bounds__(256) void k_rq_latest(const i64* __restrict__ end_sec, const u32* __restrict__ alloc_off, const u32* __restrict__ alloc_node,
                                                   u32 num_jobs, u32 num_allocs, u32 N, i64* __restrict__ latest) {
  const u32 a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= num_allocs) return;
  const u32 n = alloc_node[a];
  if (n >= N) return;                       // (the host refused the call already)
  const u32 j = csr_owner(alloc_off, num_jobs, a);
  (void)__hip_atomic_fetch_max((long long*)&latest[n], (long long)end_sec[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u64 rq_key(i64 t) { return (u64)t ^ 0x8000000000000000ull; }   // signed order -> unsigned order

// The starts t >= start at which the candidate is free are what is left of [max(start, latest_end), never) once every reservation
// has taken its blocked starts [st - (d - 1), ed - 1] out.  The node's reservations come sorted by st, so the blocked ranges come
// sorted by their first start and one pass merges those that overlap (the table does not forbid them).  Every gap [f, a - 1] gives a
// plus time f and a minus time a; the last gap is open: a plus time only.  An end at kRqNever closes the walk: never free again.
__global__ __launch_bounds__(256) void k_rq_emit(const RqParams P) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.L) return;
  const u32 o = P.ev_off[i], slots = P.ev_off[i + 1] - o;
  if (slots == 0) return;
  const u32 q = csr_owner(P.cand_off, P.Q, i);
  const u32 n = P.cand[i];
  const i64 start = P.q_start[q], d = P.q_dur[q];
  u32 np = 0, nm = 0;
  const i64 le = P.latest[n];
  i64 cur = le > start ? le : start;
  bool alive = cur != kRqNever;
  const u32 e1 = P.rv_off[n + 1];
  for (u32 e = P.rv_off[n]; e < e1 && alive; ++e) {
    const i64 st = P.rv_st[e], ed = P.rv_ed[e];
    if (st == kRqNever) continue;           // st < end never holds (the end saturates there)
    i64 a = rq_sub_sat(st, d - 1);
    if (a < start) a = start;
    if (ed <= a) continue;                  // blocks no start of the range
    if (a > cur) { P.ev_key[o + np++] = rq_key(cur); P.ev_key[P.EV + o + nm++] = rq_key(a); }
    if (ed > cur) cur = ed;
    alive = cur != kRqNever;
  }
  if (alive) P.ev_key[o + np++] = rq_key(cur);
  for (; np < slots; ++np) P.ev_key[o + np] = rq_key(kRqNever);
  for (; nm < slots; ++nm) P.ev_key[P.EV + o + nm] = rq_key(kRqNever);
  for (u32 j = 0; j < slots; ++j) { P.ev_seg[o + j] = q; P.ev_seg[P.EV + o + j] = P.Q + q; }
}

// between the two halves of the sort: the times are in order; now the key is the segment and the value the position in that order
__global__ __launch_bounds__(256) void k_rq_by_segment(const u32* __restrict__ seg, u64* __restrict__ key, u32* __restrict__ pos, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { key[i] = seg[i]; pos[i] = i; }
}

__global__ __launch_bounds__(256) void k_rq_gather(const u64* __restrict__ by_time, const u32* __restrict__ pos, i64* __restrict__ out, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (i64)(by_time[pos[i]] ^ 0x8000000000000000ull);   // pos < n: a permutation of 0 .. n-1
}

// One thread per sorted plus time.  The free count changes only at event times; at the LAST plus time of a run of equal ones it is
// (plus times <= t) - (minus times <= t), whatever the order inside the run.  The least t with count >= k wins (signed 64-bit min).
__global__ __launch_bounds__(256) void k_rq_first(const RqParams P, u32 total) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const i64 t = P.plus_s[i];
  if (t == kRqNever) return;
  const u32 q = csr_owner(P.seg_off, P.Q, i);
  const u32 b = P.seg_off[q], e = P.seg_off[q + 1];
  if (i + 1 < e && P.plus_s[i + 1] == t) return;
  const u32 k = P.q_k[q];
  if (k == 0) return;                       // nothing is asked for: the start itself (k_rq_classify's default)
  u32 lo = b, hi = e;                       // first minus time > t
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (P.minus_s[mid] <= t) lo = mid + 1; else hi = mid;
  }
  const u32 up = i - b + 1, down = lo - b;  // up >= down: a node stops being free only after it became free
  if (up - down >= k) (void)__hip_atomic_fetch_min((long long*)&P.best[q], (long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_rq_classify(const RqParams P) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.L) return;
  const u32 q = csr_owner(P.cand_off, P.Q, i);
  uint8_t c = CNS_RESVQ_FREE;
  if (!(P.q_flags[q] & 2u)) {
    const u32 n = P.cand[i];
    if (n >= P.N) {
      c = CNS_RESVQ_NOT_FOUND;                                  // JobScheduler.cpp:4385-4388
    } else {
      const i64 b = P.best[q];
      const i64 t = b != kRqNever ? b : P.q_start[q];
      const i64 end = rq_add_sat(t, P.q_dur[q]);
      if (P.latest[n] > t) {
        c = CNS_RESVQ_RUNNING;                                  // :4395, first
      } else {
        const u32 e1 = P.rv_off[n + 1];
        for (u32 e = P.rv_off[n]; e < e1; ++e)
          if (P.rv_st[e] < end && P.rv_ed[e] > t) { c = CNS_RESVQ_RESERVED; break; }   // :4405
      }
    }
  }
  P.code[i] = c;
}

// One workgroup per query walks its list in chunks of 256: a ballot per wave, the waves' counts through LDS, the count of the chunks
// before in a register.  A free candidate of rank r < k goes to slot r: the first k in list order (:4416).
__global__ __launch_bounds__(256) void k_rq_pick(const RqParams P) {
  __shared__ u32 wave_cnt[kRqBlock / 64];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (u32 q = blockIdx.x; q < P.Q; q += gridDim.x) {
    const u32 b = P.cand_off[q], e = P.cand_off[q + 1], k = P.q_k[q], co = P.chosen_off[q];
    const bool past = (P.q_flags[q] & 2u) != 0;
    u32 carry = 0;
    for (u32 base = b; base < e && !past; base += kRqBlock) {
      const u32 i = base + threadIdx.x;
      const bool is_free = i < e && P.code[i] == CNS_RESVQ_FREE;
      const unsigned long long m = __ballot(is_free);
      if (lane == 0) wave_cnt[wave] = (u32)__popcll(m);
      __syncthreads();
      u32 before = carry, all = 0;
      #pragma unroll
      for (u32 w = 0; w < kRqBlock / 64; ++w) { const u32 c = wave_cnt[w]; if (w < wave) before += c; all += c; }
      const u32 rank = before + (u32)__popcll(m & ((1ull << lane) - 1ull));
      if (is_free && rank < k) P.chosen[co + rank] = P.cand[i];   // rank < min(k, list length): inside the query's slots
      carry += all;
      __syncthreads();                      // wave_cnt is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
      const bool ok = !past && carry >= k;
      const i64 bt = P.best[q];
      P.status[q] = past ? CNS_RESVQ_IN_THE_PAST : ok ? CNS_RESVQ_OK : CNS_RESVQ_NOT_ENOUGH;
      P.o_start[q] = ok ? (bt != kRqNever ? bt : P.q_start[q]) : 0;
      P.num_free[q] = carry;
    }
  }
}

}  // namespace cns
