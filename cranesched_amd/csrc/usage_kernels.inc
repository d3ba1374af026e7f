// Release / charge of a batch of jobs on the usage tables (include/crane_gpu_usage/usage.h): AccountMetaContainer::DoFreeResource_ /
// DoMallocResource_ (src/CraneCtld/Accounting/AccountMetaContainer.cpp:1126-1208, :1067-1124) for J rows in call order.  Included by
// engine.hip (one translation unit, namespace cns).
//
// The table on the device: NR records of kUseComp u64 components each [cpu | mem | wall | jobs | submit | 4 name totals | 8 class counts],
// the five tables back to back [user x qos | user_acct x partition | account x qos | account x partition | qos], and behind them one
// byte per record (the nested exists byte; 1 for the qos records) and one per entity [user | account | qos].  A record that does not
// exist holds zeros (cns_usage_set_tables normalises, the kernels keep it so).
//
// The closed form (usage.h): every delta is non-negative and non-zero, so the prefix sums P_k over one record's rows are monotone.  The
// record ends as val - T when the total T fits, as zero otherwise; row k is clean while P_k <= val, the first row that does not fit
// over-frees, the rows behind it (and behind a P_k == val on a nested record) find the key gone; the QoS record over-frees again.
//
// Kernels
//   k_use_items  row-parallel, one lane per row: the row's delta as 17 u64, its up to 15 record ids (slot x = bit x of the masks), the
//                bits that need no table value (:1172), and for a charge the entity bytes.  A release reads the entity bytes, which it
//                never changes.
//   k_sort_* / k_iota (sort_kernels.inc): the (record id, row * 15 + slot) items sorted by record id, stable: inside a record the
//                rows stay in call order.  k_use_gather: the sorted streams, and how many items carry a record.
//   k_use_tails, k_use_carry, k_use_eval: the segmented inclusive scan of the 17 components over the sorted items (a segment = one
//                record), in three launches: per chunk its last segment's sums, one workgroup over the chunk tails, the re-walk with the
//                carry.  k_use_eval gives every item its exclusive and inclusive prefix -> its mask bit (atomicOr into the row's word:
//                an OR, so the order of arrival does not matter), and the last item of a segment, whose inclusive prefix is T, writes
//                the record.  Sums wrap with a sticky overflow flag; the number of carries of a sum does not depend on how it is
//                grouped, so neither does the flag.
// The kernels read the tables before the call (src) and write a copy of them (dst): no item reads what another writes.  No workgroup
// waits for another.  Every loop is bounded by an argument or a constant.  All arithmetic is integer.
#pragma once

namespace cns {

constexpr u32 kUseChunk = 256;                         // rows per workgroup of k_use_items (one lane per row)
constexpr u32 kUseSlots = 15;                          // 2 + 2 * CNS_LIM_MAX_CHAIN + 1
constexpr u32 kUseComp = 17;                           // cpu, mem, wall, jobs, submit, 4 names, 8 classes
constexpr u32 kUsePerThread = 4;                       // sorted items a lane walks
constexpr u32 kUseItemChunk = 256 * kUsePerThread;     // sorted items per workgroup of the scan
constexpr u32 kUseCarryLanes = 256;                    // lanes of k_use_carry
static_assert(2 + 2 * CNS_LIM_MAX_CHAIN + 1 == kUseSlots && CNS_USAGE_BIT_QOS == kUseSlots - 1, "one slot per record a row touches, slot = mask bit");
static_assert(5 + CNS_MAX_GRES_NAMES + CNS_MAX_GRES_CLASSES == kUseComp, "the components of a MetaResource");

struct UseParams {
  u32 J, op, Q, Pn, NK;                // NK = records + entities: the key of a slot without a record
  u32 base_uq, base_up, base_aq, base_ap, base_g, ent_user, ent_acct, ent_qos;
  const u32* user; const u32* ua; const u32* account; const u32* qos; const u32* part;
  const i64* cpu; const u64* mem; const i64* wall; const u32* jobs; const u32* submit; const u64* nt; const u64* cc; const uint8_t* skip;   // each may be null
  const u32* acct_parent;
  const uint8_t* src_ex;               // [NK] exists bytes before the call
  uint8_t* dst_ex;                     // [NK] after
  u64* delta;                          // [J * 17]
  u64* sort_key;                       // [J * 15]
  u32* mask;                           // [J] not_found | over_free << 16
};

__global__ __launch_bounds__(256) void k_use_items(const UseParams P) {
  const u32 j = blockIdx.x * kUseChunk + threadIdx.x;
  if (j >= P.J) return;
  u64* key = P.sort_key + (size_t)j * kUseSlots;
  u64* d = P.delta + (size_t)j * kUseComp;
  u32 nf = 0;
  const bool skip = P.skip && P.skip[j];
  d[0] = P.cpu && !skip ? (u64)P.cpu[j] : 0ull;
  d[1] = P.mem && !skip ? P.mem[j] : 0ull;
  d[2] = P.wall && !skip ? (u64)P.wall[j] : 0ull;
  d[3] = P.jobs && !skip ? (u64)P.jobs[j] : 0ull;
  d[4] = P.submit && !skip ? (u64)P.submit[j] : 0ull;
  for (u32 n = 0; n < CNS_MAX_GRES_NAMES; ++n) d[5 + n] = P.nt && !skip ? P.nt[(size_t)j * CNS_MAX_GRES_NAMES + n] : 0ull;
  for (u32 g = 0; g < CNS_MAX_GRES_CLASSES; ++g) d[9 + g] = P.cc && !skip ? P.cc[(size_t)j * CNS_MAX_GRES_CLASSES + g] : 0ull;
  u32 k[kUseSlots];
  for (u32 x = 0; x < kUseSlots; ++x) k[x] = P.NK;
  if (!skip) {
    const bool charge = P.op == CNS_USAGE_CHARGE;
    const u32 u = P.user[j], ua = P.ua[j], qi = P.qos[j], part = P.part[j];
    if (charge) P.dst_ex[P.ent_user + u] = 1;                                  // try_emplace_l, :1086
    if (charge || P.src_ex[P.ent_user + u]) {                                  // if_contains, :1162
      k[0] = P.base_uq + u * P.Q + qi;
      if (ua != kNone) k[1] = P.base_up + ua * P.Pn + part;
      else nf |= 1u << CNS_USAGE_BIT_USER_PART;                                // :1172 (the host check lets no charge get here)
    }
    u32 a = P.account[j];
    for (u32 i = 0; i < CNS_LIM_MAX_CHAIN && a != kNone; ++i) {
      if (charge) P.dst_ex[P.ent_acct + a] = 1;                                // :1107
      if (charge || P.src_ex[P.ent_acct + a]) {                                // :1180
        k[2 + 2 * i] = P.base_aq + a * P.Q + qi;
        k[3 + 2 * i] = P.base_ap + a * P.Pn + part;
      }
      a = P.acct_parent[a];
    }
    if (charge) P.dst_ex[P.ent_qos + qi] = 1;                                  // :1118
    if (charge || P.src_ex[P.ent_qos + qi]) k[CNS_USAGE_BIT_QOS] = P.base_g + qi;   // :1190
  }
  for (u32 x = 0; x < kUseSlots; ++x) key[x] = k[x];
  P.mask[j] = nf;
}

// sorted (key, item) pairs -> streams; ctr[0] = how many items carry a record
__global__ __launch_bounds__(256) void k_use_gather(const u64* __restrict__ keys, const u32* __restrict__ vals, u32 n, u32 NK, u32* s_key, u32* s_item, u64* ctr) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 key = keys[i];
  if (key >= NK) return;
  s_key[i] = (u32)key; s_item[i] = vals[i];
  if (i + 1 == n || keys[i + 1] >= NK) ctr[0] = (u64)i + 1;
}

// ---- the segmented scan ---------------------------------------------------------------------------------------------------------
struct UseAcc { u64 c[kUseComp]; u32 ovf; };   // sums that wrap, and whether one of them left 64 bits

__device__ __forceinline__ void use_zero(UseAcc& a) {
#pragma unroll
  for (u32 c = 0; c < kUseComp; ++c) a.c[c] = 0;
  a.ovf = 0;
}
__device__ __forceinline__ void use_add_row(UseAcc& a, const u64* __restrict__ row) {
#pragma unroll
  for (u32 c = 0; c < kUseComp; ++c) {
    const u64 s = a.c[c] + row[c];
    a.ovf |= s < a.c[c] ? 1u : 0u;
    a.c[c] = s;
  }
}
// a <= b in every component / a == b; an overflowed sum fits nothing
__device__ __forceinline__ bool use_fits(const UseAcc& a, const u64* __restrict__ val) {
  bool f = a.ovf == 0;
#pragma unroll
  for (u32 c = 0; c < kUseComp; ++c) f = f && a.c[c] <= val[c];
  return f;
}
__device__ __forceinline__ bool use_equals(const UseAcc& a, const u64* __restrict__ val) {
  bool f = a.ovf == 0;
#pragma unroll
  for (u32 c = 0; c < kUseComp; ++c) f = f && a.c[c] == val[c];
  return f;
}

struct UsePar {
  u32 n, nchunks, op, base_g;          // n: sorted items that carry a record; records below base_g are nested
  const u32* s_key; const u32* s_item; // [n] record id, row * 15 + slot
  const u64* delta;                    // [J * 17]
  const u64* src_rec; const uint8_t* src_ex;
  u64* dst_rec; uint8_t* dst_ex;
  u64* tails; u32* tflags;             // [nchunks * 17], [nchunks]: bit 0 a segment head lies in the chunk, bit 1 overflow
  u64* carry; u32* cflags;             // [nchunks * 17], [nchunks]: the sums since the last head before the chunk; bit 1 overflow
  u32* mask;                           // [J]
  u64* ctr;                            // 1 records touched, 2 a charge left the formats
};

// Inclusive segmented scan over the N lanes of a workgroup.  In: every lane's own element (v, head).  Out: the lane's exclusive
// prefix (ex, xh: a head lies before this lane), and in s_c[.][N - 1], s_f[N - 1] the total.  (a then b) = b.head ? b : (a + b, a.head).
template <u32 N>
__device__ __forceinline__ void use_block_scan(const UseAcc& v, u32 head, u64 (*s_c)[N], u32* s_f, UseAcc& ex, u32& xh) {
  const u32 t = threadIdx.x;
#pragma unroll
  for (u32 c = 0; c < kUseComp; ++c) s_c[c][t] = v.c[c];
  s_f[t] = head | v.ovf << 1;
  __syncthreads();
  for (u32 d = 1; d < N; d <<= 1) {
    UseAcc p;
    use_zero(p);
    u32 pf = 0;
    const bool take = t >= d && !(s_f[t] & 1u);
    if (take) {
#pragma unroll
      for (u32 c = 0; c < kUseComp; ++c) p.c[c] = s_c[c][t - d];
      pf = s_f[t - d];
    }
    __syncthreads();
    if (take) {
      u32 of = 0;
#pragma unroll
      for (u32 c = 0; c < kUseComp; ++c) {
        const u64 a = s_c[c][t], s = a + p.c[c];
        of |= s < a ? 1u : 0u;
        s_c[c][t] = s;
      }
      s_f[t] = (s_f[t] & 2u) | (pf & 3u) | of << 1;
    }
    __syncthreads();
  }
  use_zero(ex);
  xh = 0;
  if (t) {
#pragma unroll
    for (u32 c = 0; c < kUseComp; ++c) ex.c[c] = s_c[c][t - 1];
    ex.ovf = s_f[t - 1] >> 1 & 1u;
    xh = s_f[t - 1] & 1u;
  }
}

// A lane's kUsePerThread consecutive items: their record ids, which of them open a segment, and the lane's element of the block scan.
struct UseWalk { u32 key[kUsePerThread], item[kUsePerThread]; bool act[kUsePerThread], head[kUsePerThread]; };

__device__ __forceinline__ void use_walk_load(const UsePar& P, u32 beg, UseWalk& W, UseAcc& v, u32& hd) {
  const u32 i0 = beg + threadIdx.x * kUsePerThread;
  u32 prev = i0 > 0 && i0 - 1 < P.n ? P.s_key[i0 - 1] : kNone;
  use_zero(v);
  hd = 0;
#pragma unroll
  for (u32 b = 0; b < kUsePerThread; ++b) {
    const u32 i = i0 + b;
    W.act[b] = i < P.n;
    const u32 x = W.act[b] ? i : 0u;   // clamped: masked afterwards (item 0 exists whenever a workgroup runs)
    W.key[b] = P.s_key[x]; W.item[b] = P.s_item[x];
    W.head[b] = W.act[b] && W.key[b] != prev;
    if (W.head[b]) { use_zero(v); hd = 1; }
    if (W.act[b]) { use_add_row(v, P.delta + (size_t)(W.item[b] / kUseSlots) * kUseComp); prev = W.key[b]; }
  }
}

__global__ __launch_bounds__(256) void k_use_tails(const UsePar P) {
  __shared__ u64 s_c[kUseComp][256];
  __shared__ u32 s_f[256];
  UseWalk W;
  UseAcc v, ex;
  u32 hd, xh;
  use_walk_load(P, blockIdx.x * kUseItemChunk, W, v, hd);
  use_block_scan<256>(v, hd, s_c, s_f, ex, xh);
  if (threadIdx.x < kUseComp) P.tails[(size_t)blockIdx.x * kUseComp + threadIdx.x] = s_c[threadIdx.x][255];
  if (threadIdx.x == 255) P.tflags[blockIdx.x] = s_f[255];
}

// carry[c] = the sums of the items since the last segment head before chunk c.  One workgroup: every lane over `per` consecutive
// chunks, a segmented scan over the lanes, a second sweep that writes.
__device__ __forceinline__ void use_carry_step(const UsePar& P, u32 c, UseAcc& a, u32& hd) {
  const u32 f = P.tflags[c];
  if (f & 1u) { use_zero(a); hd = 1; }
  use_add_row(a, P.tails + (size_t)c * kUseComp);
  a.ovf |= f >> 1 & 1u;
}

__global__ __launch_bounds__(kUseCarryLanes) void k_use_carry(const UsePar P) {
  __shared__ u64 s_c[kUseComp][kUseCarryLanes];
  __shared__ u32 s_f[kUseCarryLanes];
  const u32 t = threadIdx.x, per = (P.nchunks + kUseCarryLanes - 1) / kUseCarryLanes;
  const u32 lo = t * per < P.nchunks ? t * per : P.nchunks, hi = lo + per < P.nchunks ? lo + per : P.nchunks;
  UseAcc a, ex;
  u32 hd = 0, xh;
  use_zero(a);
  for (u32 c = lo; c < hi; ++c) use_carry_step(P, c, a, hd);
  use_block_scan<kUseCarryLanes>(a, hd, s_c, s_f, ex, xh);
  a = ex;
  for (u32 c = lo; c < hi; ++c) {
#pragma unroll
    for (u32 x = 0; x < kUseComp; ++x) P.carry[(size_t)c * kUseComp + x] = a.c[x];
    P.cflags[c] = a.ovf << 1;
    use_carry_step(P, c, a, hd);
  }
}

__global__ __launch_bounds__(256) void k_use_eval(const UsePar P) {
  __shared__ u64 s_c[kUseComp][256];
  __shared__ u32 s_f[256];
  UseWalk W;
  UseAcc acc, ex;
  u32 hd, xh;
  use_walk_load(P, blockIdx.x * kUseItemChunk, W, acc, hd);
  use_block_scan<256>(acc, hd, s_c, s_f, ex, xh);
  acc = ex;
  if (!xh) {   // no head between the chunk's start and this lane: the sums reach back into the chunks before
    use_add_row(acc, P.carry + (size_t)blockIdx.x * kUseComp);
    acc.ovf |= P.cflags[blockIdx.x] >> 1 & 1u;
  }
  const u32 i0 = blockIdx.x * kUseItemChunk + threadIdx.x * kUsePerThread;
  u32 records = 0;
  bool bad = false;
#pragma unroll
  for (u32 b = 0; b < kUsePerThread; ++b) {
    if (!W.act[b]) continue;
    const u32 i = i0 + b, r = W.key[b], row = W.item[b] / kUseSlots, bit = W.item[b] % kUseSlots;
    if (W.head[b]) use_zero(acc);
    const bool first = W.head[b];
    const bool last = i + 1 == P.n || P.s_key[i + 1] != r;
    const bool nested = r < P.base_g;
    const u64* val = P.src_rec + (size_t)r * kUseComp;
    u64* out = P.dst_rec + (size_t)r * kUseComp;
    UseAcc pre = acc;                                         // P_{k-1}
    use_add_row(acc, P.delta + (size_t)row * kUseComp);      // P_k
    records += last ? 1u : 0u;
    if (P.op == CNS_USAGE_CHARGE) {
      if (last) {   // val + T, refused where the reference's formats end (:39-45: 32-bit counts; cpu and wall are signed)
        bool ovf = acc.ovf != 0;
#pragma unroll
        for (u32 c = 0; c < kUseComp; ++c) {
          const u64 s = val[c] + acc.c[c];
          ovf = ovf || s < val[c];
          if (c == 0 || c == 2) ovf = ovf || s > 0x7FFFFFFFFFFFFFFFull;
          if (c == 3 || c == 4) ovf = ovf || s > 0xFFFFFFFFull;
          out[c] = s;
        }
        bad = bad || ovf;
        if (nested) P.dst_ex[r] = 1;
      }
      continue;
    }
    if (nested && !P.src_ex[r]) {                             // map.find(key) == end, :1142: for every row, nothing changes
      atomicOr(P.mask + row, 1u << bit);
      continue;
    }
    const bool fit = use_fits(acc, val);
    if (!fit) {
      // the first row that does not fit over-frees (:1152, :1196); behind it, or behind an exact fit, a nested key is gone (:1143)
      const bool gone = nested && !first && !(use_fits(pre, val) && !use_equals(pre, val));
      atomicOr(P.mask + row, gone ? 1u << bit : 1u << (16 + bit));
    }
    if (last) {
      u64 any = 0;
#pragma unroll
      for (u32 c = 0; c < kUseComp; ++c) {
        const u64 v = fit ? val[c] - acc.c[c] : 0ull;
        out[c] = v;
        any |= v;
      }
      if (nested) P.dst_ex[r] = any ? 1 : 0;                  // val.IsZero() -> erase, :1159
    }
  }
  for (u32 off = 32; off; off >>= 1) records += (u32)__shfl_xor((int)records, (int)off);
  if ((threadIdx.x & 63) == 0 && records) atomicAdd((unsigned long long*)(P.ctr + 1), (unsigned long long)records);
  if (bad) P.ctr[2] = 1;
}

}  // namespace cns
