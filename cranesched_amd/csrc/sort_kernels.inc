// The stable pair sort every feature shares, and the ordered scan of per-wave counts that runs on one of its kernels.  Included by
// engine.hip ahead of priority_kernels.hip (one translation unit, namespace cns); launched from sort_call.inc only, the pass and buffer
// arithmetic is sort_host.inc.
#pragma once

namespace cns {

// ---- stable LSD radix sort, 8-bit digits, (u64 key, u32 value) ------------------------------------------
// Three kernels per pass: per-tile digit histogram, scan of the [digit][tile] table (one block per digit row),
// stable scatter.  A tile = kSortTile consecutive elements handled by one 256-thread block, in chunks of 256 in
// index order; inside a chunk the rank among equal digits comes from wave ballots (match-any over the 8
// digit bits) + a per-wave count table in LDS, so equal keys never change their relative order.
constexpr u32 kSortTile = 4096;
constexpr u32 kSortScanSpan = 256;   // tiles one step of k_sort_rowscan takes (its 256 threads, one tile each); more tiles: a carry between the steps

__global__ __launch_bounds__(256) void k_sort_hist(const u64* __restrict__ keys, u32 n, u32 shift, u32* __restrict__ hist,
                                                   u32 ntiles) {
  __shared__ u32 s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const u32 base = blockIdx.x * kSortTile;
  for (u32 c = 0; c < kSortTile; c += 256) {
    const u32 i = base + c + threadIdx.x;
    if (i < n) atomicAdd(&s_h[(u32)(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[threadIdx.x * ntiles + blockIdx.x] = s_h[threadIdx.x];  // digit-major: the scan runs over it linearly
}

// Scan of the [digit][tile] table, two levels: every digit row is scanned by its own block (exclusive, in
// place) and leaves its total in rowtot[digit]; the scatter kernel adds the exclusive prefix over rowtot.
__global__ __launch_bounds__(256) void k_sort_rowscan(u32* __restrict__ hist, u32 ntiles, u32* __restrict__ rowtot) {
  __shared__ u32 s_w[4];
  u32* row = hist + (size_t)blockIdx.x * ntiles;
  const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  u32 carry = 0;
  for (u32 c = 0; c < ntiles; c += kSortScanSpan) {
    const u32 i = c + threadIdx.x;
    const u32 v = i < ntiles ? row[i] : 0u;
    u32 inc = v;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
      const u32 t = (u32)__shfl_up((int)inc, (int)off);
      if (lane >= off) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    u32 pre = carry;
    for (u32 w = 0; w < wv; ++w) pre += s_w[w];
    if (i < ntiles) row[i] = pre + inc - v;
    carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) rowtot[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void k_sort_scatter(const u64* __restrict__ kin, const u32* __restrict__ vin,
                                                      u64* __restrict__ kout, u32* __restrict__ vout, u32 n, u32 shift,
                                                      const u32* __restrict__ offs, u32 ntiles,
                                                      const u32* __restrict__ rowtot) {
  __shared__ u32 s_base[256];      // next output slot of each digit for this tile
  __shared__ u32 s_cnt[4][256];    // per wave: elements of the current chunk with that digit
  const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  {  // start of digit d's output range = sum of the totals of the smaller digits (block scan of 256 values)
    const u32 v = rowtot[threadIdx.x];
    u32 inc = v;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
      const u32 t = (u32)__shfl_up((int)inc, (int)off);
      if (lane >= off) inc += t;
    }
    if (lane == 63) s_cnt[0][wv] = inc;
    __syncthreads();
    u32 pre = 0;
    for (u32 w = 0; w < wv; ++w) pre += s_cnt[0][w];
    __syncthreads();
    s_base[threadIdx.x] = pre + inc - v + offs[threadIdx.x * ntiles + blockIdx.x];
  }
  const u32 base = blockIdx.x * kSortTile;
  for (u32 c = 0; c < kSortTile; c += 256) {
    for (u32 w = 0; w < 4; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const u32 i = base + c + threadIdx.x;
    const bool act = i < n;
    u64 k = 0;
    u32 v = 0, d = 0;
    if (act) { k = kin[i]; v = vin[i]; d = (u32)(k >> shift) & 255u; }
    // lanes of this wave holding the same digit
    u64 peers = __ballot(act);
#pragma unroll
    for (u32 b = 0; b < 8; ++b) {
      const u64 m = __ballot(act && ((d >> b) & 1u));
      peers &= ((d >> b) & 1u) ? m : ~m;
    }
    const u32 rank = (u32)__popcll(peers & ((1ull << lane) - 1ull));
    if (act && rank == 0) s_cnt[wv][d] = (u32)__popcll(peers);
    __syncthreads();
    if (act) {
      u32 o = s_base[d] + rank;
      for (u32 w = 0; w < wv; ++w) o += s_cnt[w][d];
      kout[o] = k;
      vout[o] = v;
    }
    __syncthreads();
    s_base[threadIdx.x] += s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_iota(u32* v, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

}  // namespace cns
