// Kernels of include/crane_gpu_running/running_attrs.h: the attribute columns that follow the rows of the device ledger through a
// cycle boundary, the per-row sums the MultiFactorPriority sorter reads of a running job, and the running side of
// cns_priority_order_resident (the input rules, the presence flags, the keys of the per-account CSR and its offsets).  Included by
// engine.hip behind running_kernels.inc, whose kernels stay as they are; host side: running_attrs_host.inc.
//
// A call of cns_running_advance_attrs, beside the launches of cns_running_advance:
//   k_ra_origin<false>   behind the scan of the kept rows' counts: k_run_compact's row position (run_row's verdict, the mbcnt rank, the
//                        scanned per-wave count) and nothing else; origin[position] = the old row
//   k_ra_origin<true>    the same over the queue: origin[position] = the queue index.  Which of the two a position holds follows from
//                        the position: the kept rows come first (tot[0] of them), so no bit marks an admitted row and no size is lost.
//   k_ra_gather          one thread per new row: all five columns from the old row, or from the queue's arrays with start = now
// Once per ledger state (the first consumer behind a seed / advance):
//   k_ra_sums            k_run_keep's shape, one lane per row: node_num, and the cpu and memory of the row's allocations summed in 128
//                        bits (exact whatever the order, so the hand-off of a row wider than kRunLaneMax to its wave, 64 entries per
//                        step, gives the lane's result); the least row whose cpu sum is negative / whose sums leave int64 / uint64 into
//                        two flag words (32-bit atomicMin, as k_rp_mark records its row)
// Per cns_priority_order_resident:
//   k_ra_accounts        one thread per row and per pending job: the least row whose account >= A into a flag word; acc_present
//                        bytes for the others (plain byte stores: equal values from several lanes are harmless); keys[row] = account
//   k_sort_* (sort_index_pairs of sort_call.inc)   the stable argsort of the rows by account, ceil(bits(A - 1) / 8) passes: the
//                        sorted values ARE acc_jobs, ledger order kept inside an account
//   k_ra_accoff          acc_off[a] = the lower bound of a in the sorted keys, as k_run_fill takes rn_off
//   k_ra_pick            (cns_running_select_preempt_attrs) the job ids of the few preempted rows
// No workgroup waits for another; no LDS, no barrier; no atomic hands out a position; every store is a plain vector store; every index
// read from memory is bounded.

namespace cns {

template <bool ADMIT>
__global__ __launch_bounds__(256) void k_ra_origin(const RunSrc S, u32* __restrict__ origin) {
  const u32 lane = threadIdx.x & 63u;
  const u64 j = (u64)blockIdx.x * kRunChunk + threadIdx.x;
  bool keep; u64 b, e; u32 cnt;
  run_row<ADMIT>(S, j, j < S.n, lane, false, keep, b, e, cnt);
  const unsigned long long mk = __ballot(keep);
  const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(mk >> 32), __builtin_amdgcn_mbcnt_lo((u32)mk, 0u));
  const u64 w = (u64)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  const u64 drow = (u64)(S.base ? S.base[0] : 0u) + S.wave_rows[w] + rank;
  if (keep && drow < S.cap_rows) origin[drow] = (u32)j;
}

struct RaCols {   // one copy of the columns
  i64* start;
  u32* qos;
  u32* qprio;
  u32* part;
  u32* account;
};

struct RaGather {
  u32 cap_rows, old_rows;
  u64 queue_jobs;
  i64 now;
  const u32* tot;              // kept rows, kept entries, admitted rows, admitted entries (device)
  const u32* origin;           // [cap_rows]
  RaCols L;                    // the ledger's columns [old_rows]
  const u32 *q_qos, *q_qprio, *q_part, *q_account;   // [queue_jobs]
  RaCols D;                    // [cap_rows]
};

__global__ __launch_bounds__(256) void k_ra_gather(const RaGather G) {
  const u32 i = blockIdx.x * kRunBlock + threadIdx.x;
  const u32 kept = G.tot[0];
  const u64 rows = (u64)kept + G.tot[2];
  if (i >= G.cap_rows || i >= rows) return;
  const u32 o = G.origin[i];
  if (i < kept) {
    if (o >= G.old_rows) return;
    G.D.start[i] = G.L.start[o]; G.D.qos[i] = G.L.qos[o]; G.D.qprio[i] = G.L.qprio[o]; G.D.part[i] = G.L.part[o]; G.D.account[i] = G.L.account[o];
  } else {
    if (o >= G.queue_jobs) return;
    G.D.start[i] = G.now; G.D.qos[i] = G.q_qos[o]; G.D.qprio[i] = G.q_qprio[o]; G.D.part[i] = G.q_part[o]; G.D.account[i] = G.q_account[o];
  }
}

struct RaSums {
  u32 R, A;                    // ledger rows and allocations
  const u32* off;              // [R + 1]
  const Res* res;              // [A]
  u32* node_num;               // [R]
  i64* cpu;                    // [R]
  u64* mem;                    // [R]
  u32* flag;                   // [2] the least row with a negative cpu sum; with a sum outside its type (0xFFFFFFFF: none)
};

__global__ __launch_bounds__(256) void k_ra_sums(const RaSums S) {
  const u32 lane = threadIdx.x & 63u;
  const u64 r = (u64)blockIdx.x * kRunChunk + threadIdx.x;
  const bool valid = r < S.R;
  u32 b = 0, e = 0;
  if (valid) {
    b = S.off[r]; e = S.off[r + 1];
    if (e > S.A) e = S.A;
    if (b > e) b = e;
  }
  const bool wide = valid && e - b > kRunLaneMax;
  __int128 c = 0;
  unsigned __int128 m = 0;
  if (valid && !wide)
    for (u32 x = b; x < e; ++x) { c += S.res[x].cpu; m += S.res[x].mem; }
  // the wide rows of this wave, one after the other, 64 entries per step
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u32 ob = (u32)__shfl((int)b, owner), oe = (u32)__shfl((int)e, owner);
    __int128 pc = 0;
    unsigned __int128 pm = 0;
    for (u64 x = (u64)ob + lane; x < oe; x += 64) { pc += S.res[x].cpu; pm += S.res[x].mem; }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 cl = (u64)__shfl_xor((unsigned long long)(u64)pc, o), ch = (u64)__shfl_xor((unsigned long long)(u64)(pc >> 64), o);
      const u64 ml = (u64)__shfl_xor((unsigned long long)(u64)pm, o), mh = (u64)__shfl_xor((unsigned long long)(u64)(pm >> 64), o);
      pc += (__int128)(((unsigned __int128)ch << 64) | cl);
      pm += ((unsigned __int128)mh << 64) | ml;
    }
    if ((int)lane == owner) { c = pc; m = pm; }
  }
  if (!valid) return;
  S.node_num[r] = e - b;
  S.cpu[r] = (i64)c;
  S.mem[r] = (u64)m;
  const bool range = c > (__int128)INT64_MAX || c < (__int128)INT64_MIN || (u64)(m >> 64) != 0;
  if (range) atomicMin(S.flag + 1, (u32)r);
  else if (c < 0) atomicMin(S.flag + 0, (u32)r);
}

struct RaAccounts {
  u32 R, J, A;
  const u32* r_account;        // [R] the column
  const u32* p_account;        // [J] pending jobs (validated on the host)
  uint8_t* present;            // [max(A, 1)] zeroed
  u64* keys;                   // [R]
  u32* flag;                   // [1] the least row whose account >= A (0xFFFFFFFF: none)
};

__global__ __launch_bounds__(256) void k_ra_accounts(const RaAccounts K) {
  const u32 i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i < K.R) {
    const u32 a = K.r_account[i];
    K.keys[i] = a;
    if (a >= K.A) atomicMin(K.flag, i);
    else K.present[a] = 1;
  }
  if (i < K.J) {
    const u32 a = K.p_account[i];
    if (a < K.A) K.present[a] = 1;
  }
}

// keys: the sorted side
__global__ __launch_bounds__(256) void k_ra_accoff(const u64* __restrict__ keys, u32 R, u32 A, u32* __restrict__ acc_off) {
  const u32 a = blockIdx.x * kRunBlock + threadIdx.x;
  if (a <= A) acc_off[a] = run_lower_bound(keys, R, a);
}

__global__ __launch_bounds__(256) void k_ra_pick(const u32* __restrict__ rows, u32 n, const u32* __restrict__ ledger_id, u32 R, u32* __restrict__ ids) {
  const u32 i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i < n) ids[i] = rows[i] < R ? ledger_id[rows[i]] : 0u;
}

}  // namespace cns
