// Kernels of include/crane_gpu_amend/running_amend.h (a running job's end time changed on the device-resident running set:
// ChangeJobTimeConstraint's SetEndTime, JobScheduler.cpp:2411-2413, and ResumeSuspendedJobs, :2833-2857).  Included by engine.hip behind
// running_kernels.inc; host side: running_amend_host.inc.
//
// A call of cns_running_amend_ends:
//   k_run_amend      one workgroup per kRunChunk consecutive ledger rows, one lane per row, four independent waves (k_run_keep's shape):
//                    a bisection of the sorted amend ids; a hit stores found[position] = 1 (equal values from several lanes
//                    would be harmless) and writes the new end into the copy of the end column, a miss copies the old end.  Per wave
//                    one count of hits, by ballot and popcount.
//   k_sort_rowscan   (sort_kernels.inc, one workgroup: scan_counts of sort_call.inc) the scan of the counts; its total is the rows written.
//   k_run_refill     one thread per entry d of the per-slot tables: the end of the row that owns allocation vals[d], where vals are the
//                    sorted (slot, allocation) pairs the tables were built from (d_rp[RP_VALS]: position d of the pairs is entry d of
//                    the tables).  k_run_fill's store, without its sort and without its capacity check: no count per slot changes.
// No workgroup waits for another; no LDS, no barrier, no atomic; every store is a plain vector store.

namespace cns {

struct RunAmend {
  u32 R, K;                   // ledger rows; amendments
  const u32* id;              // [R] the ledger's ids
  const i64* end;             // [R] its end column
  const u32* am_id;           // [K] ascending
  const i64* am_end;          // [K] the new end of am_id[k]
  uint8_t* found;             // [K] zeroed
  i64* end_copy;              // [R]
  u32* wave_hits;             // per wave: rows written
};

__global__ __launch_bounds__(256) void k_run_amend(const RunAmend P) {
  const u32 lane = threadIdx.x & 63u;
  const u64 j = (u64)blockIdx.x * kRunChunk + threadIdx.x;
  bool hit = false;
  if (j < P.R) {
    const u32 id = P.id[j];
    u32 lo = 0, hi = P.K;   // the first amend id >= id
    while (lo < hi) {
      const u32 mid = lo + ((hi - lo) >> 1);
      if (P.am_id[mid] < id) lo = mid + 1; else hi = mid;
    }
    hit = lo < P.K && P.am_id[lo] == id;
    if (hit) P.found[lo] = 1;
    P.end_copy[j] = hit ? P.am_end[lo] : P.end[j];
  }
  const u32 hits = (u32)__popcll(__ballot(hit));
  if (lane == 0) P.wave_hits[(u64)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6)] = hits;
}

struct RunRefill {
  u32 M, R, A;                // table entries; ledger rows and allocations
  const u32* vals;            // [M] the allocation behind entry d
  const u32* off;             // [R + 1]
  const i64* end;             // [R] the amended end column
  const i64* rn_end_old;      // [M]
  i64* rn_end;                // [M]
};

__global__ __launch_bounds__(256) void k_run_refill(const RunRefill F) {
  const u32 d = blockIdx.x * kRunBlock + threadIdx.x;
  if (d >= F.M) return;
  const u32 e = F.vals[d];
  F.rn_end[d] = e < F.A ? F.end[csr_owner(F.off, F.R, e)] : F.rn_end_old[d];   // (k_run_fill writes no such entry either)
}

}  // namespace cns
