// Kernels of include/crane_gpu_running/running_preempt.h: the index a cycle with preemption needs of the running set, built from the
// ledger and the sorted (slot, ledger allocation) pairs of the last rebuild (running_kernels.inc) instead of by the host passes of
// cns_select_preempt (preempt_host.inc: running_side).  Included by engine.hip; host side: running_preempt_host.inc.
//
// Once per rebuild (the first cns_running_select_preempt behind a cns_running_seed / cns_running_advance):
//   k_rp_entries   one thread per sorted pair d, which IS entry d of the per-slot tables: ent_slot[d] = the key, ent_job[d] = the ledger
//                  row that owns the allocation (csr_owner over the ledger's offsets), and the (row, d) pair for the sort
//   k_sort_hist / k_sort_rowscan / k_sort_scatter   (sort_pairs of sort_call.inc) the stable LSD sort of (row, d) by row,
//                  ceil(bits(R - 1) / 8) passes: the entries of a row stay in ascending d, which is what the host's counting sort yields
//   k_rp_rows      rj_ent[i] = the sorted value; rj_off[r] = the lower bound of r in the sorted rows, as k_run_fill takes rn_off
// Per call:
//   k_rp_mark      one workgroup per kRunChunk consecutive ledger rows, one lane per row, four independent waves (k_run_keep's shape):
//                  the caller's rn_job_id against the ledger's id (the least row that differs into a flag word, a 32-bit atomicMin as
//                  k_gate_events records its first event), a bisection of the sorted preempting ids (a hit stores found[position] = 1;
//                  equal values from several lanes are harmless), rj_preempting[r], and rj_end[r] from the ledger's end of the row: every
//                  entry of a row carries that one end (k_run_fill), so no walk over the entries and no atomic is needed
//   k_rp_patch     one thread per entry: the end the cycle runs on, now + 1 where the owner row is marked, else the resident end
// No workgroup waits for another; no LDS, no barrier; every store is a plain vector store; every index read from memory is bounded.

namespace cns {

struct RpIndex {
  u32 M, R, A;                 // entries (pairs), ledger rows, ledger allocations
  const u64* keys;             // [M] the rebuild's sorted pairs: slot
  const u32* vals;             // [M] ... ledger allocation
  const u32* off;              // [R + 1] the ledger's allocation offsets
  u32* ent_job;                // [M]
  u32* ent_slot;               // [M]
  u64* skeys;                  // [M] row, for the sort
  u32* svals;                  // [M] d
};

__global__ __launch_bounds__(256) void k_rp_entries(const RpIndex X) {
  const u32 d = blockIdx.x * kRunBlock + threadIdx.x;
  if (d >= X.M) return;
  const u32 a = X.vals[d];
  const u32 r = (X.R && a < X.A) ? csr_owner(X.off, X.R, a) : 0u;
  X.ent_slot[d] = (u32)X.keys[d];
  X.ent_job[d] = r;
  X.skeys[d] = r;
  X.svals[d] = d;
}

// skeys / svals: the sorted side
__global__ __launch_bounds__(256) void k_rp_rows(const u64* __restrict__ skeys, const u32* __restrict__ svals, u32 M, u32 R, u32* __restrict__ rj_off,
                                                 u32* __restrict__ rj_ent) {
  const u32 i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i < M) rj_ent[i] = svals[i] < M ? svals[i] : 0u;
  if (i <= R) rj_off[i] = run_lower_bound(skeys, M, i);
}

struct RpMark {
  u32 R, nset;
  i64 now;
  const u32* ledger_id;        // [R]
  const i64* ledger_end;       // [R]
  const u32* given_id;         // [R] the caller's rn_job_id
  const u32* set;              // [nset] ascending, each id once
  const u32* rj_off;           // [R + 1]
  uint8_t* found;              // [nset]
  uint8_t* rj_preempting;      // [R]
  i64* rj_end;                 // [R]
  u32* flag;                   // [1] the least row whose ids differ (0xFFFFFFFF: none)
};

__global__ __launch_bounds__(256) void k_rp_mark(const RpMark K) {
  const u32 r = blockIdx.x * kRunChunk + threadIdx.x;
  if (r >= K.R) return;
  const u32 id = K.ledger_id[r];
  if (K.given_id[r] != id) atomicMin(K.flag, r);
  u32 lo = 0, hi = K.nset;   // the first id of the set >= id
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (K.set[mid] < id) lo = mid + 1; else hi = mid;
  }
  const bool hit = lo < K.nset && K.set[lo] == id;
  if (hit) K.found[lo] = 1;
  K.rj_preempting[r] = hit ? 1 : 0;
  const i64 soon = K.now + 1, end = hit ? soon : K.ledger_end[r];
  K.rj_end[r] = K.rj_off[r + 1] > K.rj_off[r] ? (end > soon ? end : soon) : 0;   // JobScheduler.cpp:6513-6514
}

__global__ __launch_bounds__(256) void k_rp_patch(const u32* __restrict__ ent_job, const uint8_t* __restrict__ rj_preempting, const i64* __restrict__ rn_end,
                                                  u32 M, u32 R, i64 now, i64* __restrict__ ent_end) {
  const u32 d = blockIdx.x * kRunBlock + threadIdx.x;
  if (d >= M) return;
  const u32 r = ent_job[d];
  ent_end[d] = (r < R && rj_preempting[r]) ? now + 1 : rn_end[d];
}

}  // namespace cns
