// The launches of sort_kernels.inc, written once for every caller: the stable pair sort, the same as an argsort, and the ordered scan of
// per-wave counts.  Included by engine.hip next to job_table.inc.  The routines only launch: no synchronize, no memset, and the
// hipGetLastError is the caller's.  The buffers are the callers' too, in their slot arrays (buf_slots.h).

// n_pass stable passes over the low 8 * n_pass bits of the keys, on `stream`.  Afterwards (kin, vin) name the sorted side,
// (kout, vout) the other one.  hist: cns_sort::hist_bytes(tiles(n)) bytes.  Launches nothing for n == 0 or n_pass == 0.
void sort_pairs(hipStream_t stream, u32 n, u32 n_pass, u64*& kin, u32*& vin, u64*& kout, u32*& vout, u32* hist) {
  if (n == 0) return;
  const u32 ntiles = cns_sort::tiles(n, kSortTile);
  u32* rowtot = hist + (size_t)256 * ntiles;
  for (u32 pass = 0; pass < n_pass; ++pass) {
    const u32 shift = pass * cns_sort::kDigitBits;
    hipLaunchKernelGGL(k_sort_hist, dim3(ntiles), dim3(256), 0, stream, (const u64*)kin, n, shift, hist, ntiles);
    hipLaunchKernelGGL(k_sort_rowscan, dim3(256), dim3(256), 0, stream, hist, ntiles, rowtot);
    hipLaunchKernelGGL(k_sort_scatter, dim3(ntiles), dim3(256), 0, stream, (const u64*)kin, (const u32*)vin, kout, vout, n, shift, (const u32*)hist, ntiles,
                       (const u32*)rowtot);
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
}

// the same behind values 0 .. n - 1 written to vin (k_iota): a stable argsort of the keys
void sort_index_pairs(hipStream_t stream, u32 n, u32 n_pass, u64*& kin, u32*& vin, u64*& kout, u32*& vout, u32* hist) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, stream, vin, n);
  sort_pairs(stream, n, n_pass, kin, vin, kout, vout, hist);
}

// the ordered exclusive scan of n counts in place on one workgroup, their sum to *total (k_sort_rowscan as gate and running use it)
void scan_counts(hipStream_t stream, u32* counts, u32 n, u32* total) {
  hipLaunchKernelGGL(k_sort_rowscan, dim3(1), dim3(256), 0, stream, counts, n, total);
}
