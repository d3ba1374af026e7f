// Kernels of include/crane_gpu_running/running.h (the running set kept on the device between two cycles: FreeResourceFromNode for the
// jobs that ended, CranedMetaContainer.cpp:226-277, MallocResourceFromNode for the jobs the commit loop started, :178-224, and the
// running jobs folded into the node states, JobScheduler.cpp:6681-6709).  Included by engine.hip; host side: running_host.inc.
//
// A call of cns_running_advance:
//   k_run_keep<false>     one workgroup per kRunChunk consecutive ledger rows, one lane per row, four independent waves (k_gate_jobs'
//                         shape): a bisection of the sorted retire ids; a hit stores found[position] = 1 (equal values from several lanes
//                         are harmless) and drops the row.  Per wave one count of kept rows and one of kept allocation entries.
//   k_sort_rowscan        (sort_kernels.inc, one workgroup: scan_counts of sort_call.inc) the exclusive scan of each count array in place,
//                         kRunScanSpan per step: the ordered compaction of cns_gate_pending.  No atomic hands out a position.
//   k_run_compact<false>  the row goes to base + mbcnt rank, its allocations to base + the wave prefix over the lanes' entry counts.  A
//                         row of at most kRunLaneMax entries is copied by its own lane; a wider one is handed to its wave, 64 entries
//                         per step (k_cc_check's hand-off).
//   k_run_keep<true> / k_sort_rowscan / k_run_compact<true>   the same three steps over the queue of the last cycle: a job is taken
//                         when its admit byte is set, its reason is CNS_REASON_NONE and it starts now; its entries are the placement
//                         records that name a node, read where the cycle left them; the rows are appended behind the kept ones.
//   k_run_seal            one thread: the offset behind the last row.
// The rebuild (also all of cns_running_seed behind the upload):
//   k_run_expand<false>   one thread per allocation entry: its owner row by csr_owner, its target slots — every slot of the node (the
//                         device CSR of Layout::node_slots; empty for an unschedulable node), or inside a reservation the one virtual
//                         slot, by bisection of that reservation's ascending slot range (ResvLayout::resv_slot) — counted per wave.
//   k_sort_rowscan        the ordered scan of the per-wave counts
//   k_run_expand<true>    the (slot, entry) pairs in entry order
//   k_sort_hist / k_sort_rowscan / k_sort_scatter   (sort_kernels.inc: sort_pairs of sort_call.inc) the stable LSD sort of the pairs by slot, ceil(bits(S) / 8) passes:
//                         per slot the entries stay in ledger order, which is build_running's order
//   k_run_fill            per sorted pair rn_end / rn_res; per slot rn_off as a lower bound in the sorted keys, and the time map's
//                         capacity check, a failure recorded in a flag word.  No atomics.
// No workgroup waits for another; the kernels of this file use no LDS and no barrier; every store is a plain vector store.

#include "csr_dev.h"

namespace cns {

constexpr u32 kRunBlock = 256;
constexpr u32 kRunChunk = 256;      // rows of one workgroup: one per lane
constexpr u32 kRunLaneMax = 8;      // allocation entries one lane copies alone: kCcLaneMax, for the same reason (DESIGN.md 6)
constexpr u32 kRunScanSpan = kSortScanSpan;   // per-wave counts one step of k_sort_rowscan takes
static_assert(kRunLaneMax == kCcLaneMax, "the hand-off to the wave at the width k_cc_check uses");

struct RunLedger {   // one copy of the ledger
  u32* id;           // [rows]
  i64* end;          // [rows]
  u32* resv;         // [rows]
  u32* off;          // [rows + 1]
  u32* node;         // [entries]
  Res* res;          // [entries]
};

struct RunSrc {
  u64 n;                      // rows of the source: the ledger, or the queue
  // the ledger as the source
  RunLedger L;
  u32 src_ents;
  u32 nret;
  const u32* ret;             // [nret] ascending
  uint8_t* found;             // [nret]
  // the queue and its results as the source (read only)
  const u32* job_id;          // [n]
  const uint8_t* admit;       // [n] or null
  const u32* jresv;           // [n] or null
  const uint8_t* reason;      // [n]
  const i64* start;           // [n]
  const i64* limit;           // [n]
  const u64* place_off;       // [n + 1]
  u64 places;
  const u32* pnode;           // [places]
  const i64* pcpu;
  const u64 *pmem, *pclo, *pchi, *pgres, *pc2, *pc3;   // pc2 / pc3 null: no node has a core id above 127
  i64 now;
  // the counts per wave: written by k_run_keep, scanned in place, read by k_run_compact
  u32* wave_rows;
  u32* wave_ents;
  // the destination
  RunLedger D;
  u32 cap_rows, cap_ents;
  const u32* base;            // rows and entries already in front (device: the kept rows' totals) or null
};

template <bool ADMIT>
__device__ __forceinline__ bool run_rec_ok(const RunSrc& S, u64 x) {
  return !ADMIT || S.pnode[x] != CNS_NODE_NONE;
}

// row j of the source: is it taken, its entry range [b, e) and how many of those entries count
template <bool ADMIT>
__device__ __forceinline__ void run_row(const RunSrc& S, u64 j, bool valid, u32 lane, bool mark, bool& keep, u64& b, u64& e, u32& cnt) {
  keep = false; b = e = 0; cnt = 0;
  if (valid) {
    if (!ADMIT) {
      const u32 id = S.L.id[j];
      u32 lo = 0, hi = S.nret;   // the first retire id >= id
      while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (S.ret[mid] < id) lo = mid + 1; else hi = mid;
      }
      const bool hit = lo < S.nret && S.ret[lo] == id;
      if (hit && mark) S.found[lo] = 1;
      keep = !hit;
      if (keep) {
        b = S.L.off[j]; e = S.L.off[j + 1];
        if (e > S.src_ents) e = S.src_ents;
        if (b > e) b = e;
        cnt = (u32)(e - b);
      }
    } else {
      keep = (!S.admit || S.admit[j]) && S.reason[j] == CNS_REASON_NONE && S.start[j] == S.now;   // JobScheduler.cpp:1575-1628
      if (keep) {
        b = S.place_off[j]; e = S.place_off[j + 1];
        if (e > S.places) e = S.places;
        if (b > e) b = e;
      }
    }
  }
  if (ADMIT) {
    const bool wide = keep && e - b > kRunLaneMax;
    if (keep && !wide)
      for (u64 x = b; x < e; ++x) cnt += run_rec_ok<ADMIT>(S, x) ? 1u : 0u;
    unsigned long long todo = __ballot(wide);
    while (todo) {
      const int owner = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const u64 ob = (u64)__shfl((unsigned long long)b, owner), oe = (u64)__shfl((unsigned long long)e, owner);
      u32 n = 0;
      for (u64 base = ob; base < oe; base += 64) {
        const u64 x = base + lane;
        n += (u32)__popcll(__ballot(x < oe && run_rec_ok<ADMIT>(S, x)));
      }
      if ((int)lane == owner) cnt = n;
    }
  }
}

template <bool ADMIT>
__global__ __launch_bounds__(256) void k_run_keep(const RunSrc S) {
  const u32 lane = threadIdx.x & 63u;
  const u64 j = (u64)blockIdx.x * kRunChunk + threadIdx.x;
  bool keep; u64 b, e; u32 cnt;
  run_row<ADMIT>(S, j, j < S.n, lane, true, keep, b, e, cnt);
  const u32 rows = (u32)__popcll(__ballot(keep));
  u32 ents = keep ? cnt : 0u;
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) ents += (u32)__shfl_xor((int)ents, off);
  if (lane == 0) {
    const u64 w = (u64)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
    S.wave_rows[w] = rows;
    S.wave_ents[w] = ents;
  }
}

template <bool ADMIT>
__device__ __forceinline__ void run_copy(const RunSrc& S, u64 x, u64 d) {
  if (d >= S.cap_ents) return;
  if (!ADMIT) {
    S.D.node[d] = S.L.node[x];
    S.D.res[d] = S.L.res[x];
  } else {
    Res r;
    r.cpu = S.pcpu[x]; r.mem = S.pmem[x]; r.clo = S.pclo[x]; r.chi = S.pchi[x]; r.gres = S.pgres[x];
    r.c2 = S.pc2 ? S.pc2[x] : 0; r.c3 = S.pc3 ? S.pc3[x] : 0;
    S.D.node[d] = S.pnode[x];
    S.D.res[d] = r;
  }
}

template <bool ADMIT>
__global__ __launch_bounds__(256) void k_run_compact(const RunSrc S) {
  const u32 lane = threadIdx.x & 63u;
  const u64 j = (u64)blockIdx.x * kRunChunk + threadIdx.x;
  bool keep; u64 b, e; u32 cnt;
  run_row<ADMIT>(S, j, j < S.n, lane, false, keep, b, e, cnt);
  const unsigned long long mk = __ballot(keep);
  const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(mk >> 32), __builtin_amdgcn_mbcnt_lo((u32)mk, 0u));   // kept lanes below this one
  const u32 mine = keep ? cnt : 0u;
  u32 inc = mine;
  #pragma unroll
  for (u32 off = 1; off < 64; off <<= 1) {
    const u32 t = (u32)__shfl_up((int)inc, (int)off);
    if (lane >= off) inc += t;
  }
  const u64 w = (u64)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  const u64 drow = (u64)(S.base ? S.base[0] : 0u) + S.wave_rows[w] + rank;
  const u64 dent = (u64)(S.base ? S.base[1] : 0u) + S.wave_ents[w] + (inc - mine);
  const bool ok = keep && drow < S.cap_rows && dent + mine <= S.cap_ents;
  if (ok) {
    if (!ADMIT) {
      S.D.id[drow] = S.L.id[j]; S.D.end[drow] = S.L.end[j]; S.D.resv[drow] = S.L.resv[j];
    } else {
      const i64 s = S.start[j], l = S.limit[j];
      S.D.id[drow] = S.job_id[j];
      S.D.end[drow] = l > 0 ? (s > INT64_MAX - l ? INT64_MAX : s + l) : (s < INT64_MIN - l ? INT64_MIN : s + l);   // saturating, as k_cc_check
      S.D.resv[drow] = S.jresv ? S.jresv[j] : CNS_RESV_NONE;
    }
    S.D.off[drow] = (u32)dent;
  }
  const bool wide = ok && e - b > kRunLaneMax;
  if (ok && !wide) {
    u64 d = dent;
    for (u64 x = b; x < e; ++x)
      if (run_rec_ok<ADMIT>(S, x)) run_copy<ADMIT>(S, x, d++);
  }
  // the wide rows of this wave, one after the other, 64 entries per step
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 ob = (u64)__shfl((unsigned long long)b, owner), oe = (u64)__shfl((unsigned long long)e, owner);
    u64 d = (u64)__shfl((unsigned long long)dent, owner);
    for (u64 base = ob; base < oe; base += 64) {
      const u64 x = base + lane;
      const bool take = x < oe && run_rec_ok<ADMIT>(S, x);
      const unsigned long long m = __ballot(take);
      const u32 r = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
      if (take) run_copy<ADMIT>(S, x, d + r);
      d += (u64)__popcll(m);
    }
  }
}

// tot: kept rows, kept entries, admitted rows, admitted entries
__global__ void k_run_seal(u32* __restrict__ off, const u32* __restrict__ tot, u32 cap_rows) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const u64 rows = (u64)tot[0] + tot[2];
  if (rows <= cap_rows) off[rows] = tot[1] + tot[3];
}

struct RunExp {
  u32 R, A, N, V, P_real, M;   // ledger rows and entries; nodes, reservations, real partitions of the layout; pairs the arrays hold
  const u32* off;              // [R + 1]
  const u32* node;             // [A]
  const u32* resv;             // [R]
  const u32* ns_off;           // [N + 1] node -> its slots (Layout::node_slots)
  const u32* ns;
  const u32* part_off;         // [P + 1] the device's slot list: a reservation's virtual slots ascend by node
  const u32* slot_node;        // [S]
  u32* wave_cnt;               // the pairs per wave: written by the counting launch, scanned in place, read by the writing one
  u64* keys;                   // [M] slot
  u32* vals;                   // [M] entry
};

template <bool WRITE>
__global__ __launch_bounds__(256) void k_run_expand(const RunExp E) {
  const u32 lane = threadIdx.x & 63u;
  const u32 a = blockIdx.x * kRunBlock + threadIdx.x;
  u32 cnt = 0, sb = 0, one = kNone;
  if (a < E.A) {
    const u32 j = csr_owner(E.off, E.R, a);
    const u32 n = E.node[a], rv = E.resv[j];
    if (n < E.N) {
      if (rv == CNS_RESV_NONE) {                       // every partition's slot of the node; none: not schedulable (JobScheduler.cpp:6685-6686)
        sb = E.ns_off[n]; cnt = E.ns_off[n + 1] - sb;
      } else if (rv < E.V) {                           // the reservation's virtual node, if it lists the node (:6693-6700)
        u32 lo = E.part_off[E.P_real + rv], hi = E.part_off[E.P_real + rv + 1];
        while (lo < hi) {
          const u32 mid = lo + ((hi - lo) >> 1);
          const u32 v = E.slot_node[mid];
          if (v == n) { one = mid; cnt = 1; break; }
          if (v < n) lo = mid + 1; else hi = mid;
        }
      }
    }
  }
  const u64 w = (u64)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  if (!WRITE) {
    u32 sum = cnt;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += (u32)__shfl_xor((int)sum, off);
    if (lane == 0) E.wave_cnt[w] = sum;
  } else {
    u32 inc = cnt;
    #pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
      const u32 t = (u32)__shfl_up((int)inc, (int)off);
      if (lane >= off) inc += t;
    }
    const u64 pos = (u64)E.wave_cnt[w] + (inc - cnt);
    for (u32 k = 0; k < cnt; ++k)
      if (pos + k < E.M) {
        E.keys[pos + k] = one != kNone ? one : E.ns[sb + k];
        E.vals[pos + k] = a;
      }
  }
}

struct RunFill {
  u32 M, S, R, A, tl_cap;
  const u64* keys;             // [M] ascending
  const u32* vals;             // [M]
  const u32* off;              // [R + 1]
  const i64* end;              // [R]
  const Res* res;              // [A]
  const u32* rv_off;           // [S + 1] reservation entries of a slot
  u32* rn_off;                 // [S + 1]
  i64* rn_end;                 // [M]
  Res* rn_res;                 // [M]
  u32* flag;                   // [1] a slot above the time map's capacity
};

__device__ __forceinline__ u32 run_lower_bound(const u64* __restrict__ keys, u32 n, u32 q) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < q) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_run_fill(const RunFill F) {
  const u32 i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i < F.M) {
    const u32 e = F.vals[i];
    if (e < F.A) {
      F.rn_end[i] = F.end[csr_owner(F.off, F.R, e)];
      F.rn_res[i] = F.res[e];
    }
  }
  if (i <= F.S) {
    const u32 lb = run_lower_bound(F.keys, F.M, i);
    F.rn_off[i] = lb;
    if (i < F.S) {
      const u32 cnt = run_lower_bound(F.keys, F.M, i + 1) - lb;
      const u32 nrv = F.rv_off[i + 1] - F.rv_off[i];
      if (nrv ? cnt + 2 * nrv + 2 > F.tl_cap / 2 : cnt + 2 > F.tl_cap) *F.flag = 1u;   // snapshot_host.inc: build_running
    }
  }
}

}  // namespace cns
