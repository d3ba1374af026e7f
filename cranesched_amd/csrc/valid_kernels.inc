// Kernels of include/crane_gpu_valid/validity.h (JobScheduler::CheckJobValidity, JobScheduler.cpp:7262-7374, for J jobs at once: can the
// job ever run in its partition, and on how many nodes).  Included by engine.hip; host side: valid_host.inc.
//
// Tables (built at the first call after cns_set_nodes, from the caller's node arrays as they came: schedulable or not):
//   k_valid_prep    one thread per NODE: cpu, mem, the slot count of every GRES class in one 64-bit word (8 classes, a byte each, <= 64),
//                   the slot count of every GRES name in one 32-bit word, the unsupported flag -> a 32-byte VdNode
//   k_valid_totals  one workgroup per PARTITION: 64-bit integer sums of cpu, mem, class and name counts over its node list (register
//                   partial sums, wave reduction, LDS across the four waves), the node count, "lists an unsupported node"
//   membership      is the partition's node list itself, sorted by the host: a bisection says whether the partition lists a node
// A call:
//   k_valid_walk    one workgroup per chunk of kVdChunk jobs of ONE partition (the host groups the job indices by partition); it streams the
//                   partition's node records through LDS, kVdTile at a time; every lane owns a job, reads the tile by LDS broadcast (all
//                   lanes the same address) and counts in a register.  Jobs with lists then correct their count over their lists.
// One workgroup finishes its jobs: no atomics, no workgroup waits for another.  Nothing here knows the cycle's node types, its slots or its
// width limits.  Every store is a plain vector store.

#include "csr_dev.h"

namespace cns {

constexpr u32 kVdBlock = 256;
constexpr u32 kVdTile = 256;      // node records per LDS stage: one per thread, 8 KiB (cns_validate_shape)
constexpr u32 kVdChunk = 256;     // jobs per workgroup: one per lane
constexpr u32 kVdNoPart = 0xFFFFFFFFu;
constexpr u64 kVdHigh = 0x8080808080808080ull;

struct alignas(16) VdNode {
  i64 cpu;
  u64 mem;
  u64 cls;      // byte c: slots of class c on the node
  u32 names;    // byte k: slots of name k on the node, over all its types (PublicHeader.cpp:639-641)
  u32 unsupported;
};
static_assert(sizeof(VdNode) == 32, "two 16-byte LDS reads per node record");

struct alignas(16) VdTotal {   // res_total_inc_dead of a partition (CranedMetaContainer.cpp:364-391) as counts
  i64 cpu;
  u64 mem;
  u64 cls[kMaxClasses];
  u64 name[kMaxNames];
  u32 nodes;
  u32 refused;                 // the partition lists a node flagged unsupported
};
static_assert(kMaxClasses == 8 && kMaxNames == 4, "class counts fill one 64-bit word, name counts one 32-bit word");

struct VdChunkRec { u32 part, first, count, pad; };   // part == kVdNoPart: jobs whose partition index names no partition

struct VdParams {
  // tables
  u32 N, P, V;
  const VdNode* node;
  const VdTotal* total;
  const u32* part_off;     // [P+1]
  const u32* part_nodes;   // ascending inside a partition
  const u32* rv_off;       // [V+1] nodes of every reservation, ascending inside one
  const u32* rv_nodes;
  // jobs: the caller's arrays as they came
  const i64* node_cpu; const u64* node_mem; const i64* task_cpu; const u64* task_mem;
  const u32* node_num; const u32* ntasks; const u32* gres_total; const u64* gres_spec; const u32* reservation;
  const u64* incl_off; const u32* incl;   // the lists sorted inside a job (the host's copy)
  const u64* excl_off; const u32* excl;
  // the call
  const u32* order;        // job indices grouped by partition
  const VdChunkRec* chunks;
  uint8_t* code; u32* eligible;
};

__device__ __forceinline__ u64 vd_sat_add(u64 a, u64 b) { const u64 s = a + b; return s < a ? ~0ull : s; }
__device__ __forceinline__ i64 vd_sat_add_cpu(i64 a, i64 b) { const u64 s = (u64)a + (u64)b; return s > (u64)INT64_MAX ? INT64_MAX : (i64)s; }   // a, b >= 0

__global__ __launch_bounds__(256) void k_valid_prep(u32 N, const i64* __restrict__ cpu, const u64* __restrict__ mem, const u64* __restrict__ gres,
                                                    const uint8_t* __restrict__ unsup, const GresDev G, VdNode* __restrict__ out) {
  const u32 n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const u64 g = gres ? gres[n] : 0ull;
  VdNode r;
  r.cpu = cpu[n];
  r.mem = mem[n];
  r.cls = 0;
  r.names = 0;
  for (u32 c = 0; c < kMaxClasses; ++c)
    if (c < G.num_classes) r.cls |= (u64)popc64(g & G.class_mask[c]) << (8 * c);
  for (u32 k = 0; k < kMaxNames; ++k) r.names |= (u32)popc64(g & G.name_mask[k]) << (8 * k);   // (a 64-slot name: 64 fits its byte)
  r.unsupported = unsup && unsup[n] ? 1u : 0u;
  out[n] = r;
}

constexpr u32 kVdSums = 2 + kMaxClasses + kMaxNames + 1;   // cpu, mem, classes, names, unsupported nodes

__global__ __launch_bounds__(256) void k_valid_totals(u32 P, const u32* __restrict__ part_off, const u32* __restrict__ part_nodes,
                                                      const VdNode* __restrict__ node, VdTotal* __restrict__ total) {
  __shared__ u64 part[kVdBlock / 64][kVdSums];
  const u32 p = blockIdx.x;
  if (p >= P) return;
  const u32 b = part_off[p], e = part_off[p + 1];
  u64 s[kVdSums];
  for (u32 i = 0; i < kVdSums; ++i) s[i] = 0;
  for (u32 i = b + threadIdx.x; i < e; i += kVdBlock) {
    const VdNode r = node[part_nodes[i]];
    s[0] = (u64)vd_sat_add_cpu((i64)s[0], r.cpu);
    s[1] = vd_sat_add(s[1], r.mem);
    for (u32 c = 0; c < kMaxClasses; ++c) s[2 + c] += (r.cls >> (8 * c)) & 0xFFu;      // (<= 64 per node, < 2^32 nodes: no overflow)
    for (u32 k = 0; k < kMaxNames; ++k) s[2 + kMaxClasses + k] += (r.names >> (8 * k)) & 0xFFu;
    s[kVdSums - 1] += r.unsupported;
  }
  for (u32 d = 32; d; d >>= 1)
    for (u32 i = 0; i < kVdSums; ++i) {
      const u64 o = (u64)__shfl_down((unsigned long long)s[i], d, 64);
      s[i] = i == 0 ? (u64)vd_sat_add_cpu((i64)s[0], (i64)o) : i == 1 ? vd_sat_add(s[1], o) : s[i] + o;
    }
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0)
    for (u32 i = 0; i < kVdSums; ++i) part[wave][i] = s[i];
  __syncthreads();
  if (threadIdx.x < kVdSums) {
    const u32 i = threadIdx.x;
    u64 v = part[0][i];
    for (u32 w = 1; w < kVdBlock / 64; ++w) v = i == 0 ? (u64)vd_sat_add_cpu((i64)v, (i64)part[w][i]) : i == 1 ? vd_sat_add(v, part[w][i]) : v + part[w][i];
    VdTotal& T = total[p];
    if (i == 0) { T.cpu = (i64)v; T.nodes = e - b; }
    else if (i == 1) T.mem = v;
    else if (i < 2 + kMaxClasses) T.cls[i - 2] = v;
    else if (i < 2 + kMaxClasses + kMaxNames) T.name[i - 2 - kMaxClasses] = v;
    else T.refused = v ? 1u : 0u;
  }
}

struct VdNeed { i64 cpu; u64 mem; u64 spec; u32 tot; };   // req_node_res_view + req_task_res_view (:7356); count bytes clamped to 65

// PublicHeader.cpp:619-646 on counts.  A byte of `spec` / `tot` is at most 65, a byte of the node at most 64: (node | 0x80) - need keeps
// every byte's borrow to itself, and its top bit stays set exactly where node >= need.  A zero count is no entry (it passes); a positive
// one needs the class / name present on the node (:627,:634), which node >= need > 0 implies.
__device__ __forceinline__ bool vd_fits(const VdNeed& q, const VdNode& r) {
  const u64 c = ((r.cls | kVdHigh) - q.spec) & kVdHigh;
  const u32 t = ((r.names | (u32)kVdHigh) - q.tot) & (u32)kVdHigh;
  return q.cpu <= r.cpu && q.mem <= r.mem && c == kVdHigh && t == (u32)kVdHigh;
}

__global__ __launch_bounds__(256) void k_valid_walk(const VdParams A) {
  __shared__ VdNode tile[kVdTile];
  const VdChunkRec ch = A.chunks[blockIdx.x];
  const u32 tid = threadIdx.x;
  const bool active = tid < ch.count;
  const u32 j = active ? A.order[(u64)ch.first + tid] : 0u;
  const bool found = ch.part != kVdNoPart;
  const u32 pb = found ? A.part_off[ch.part] : 0u, pe = found ? A.part_off[ch.part + 1] : 0u;

  constexpr u32 kPending = 0xFFu;
  u32 code = kPending;
  VdNeed q{0, 0, 0, 0};
  u32 k = 0, rsv = CNS_RESV_NONE;
  u64 ib = 0, ie = 0, eb = 0, ee = 0;
  if (active) {
    const i64 ncpu = A.node_cpu ? A.node_cpu[j] : 0, tcpu = A.task_cpu[j];
    const u64 nmem = A.node_mem[j], tmem = A.task_mem[j];
    k = A.node_num[j];
    const u32 nt = A.ntasks[j];
    const u32 gt = A.gres_total ? A.gres_total[j] : 0u;
    const u64 gs = A.gres_spec ? A.gres_spec[j] : 0ull;
    rsv = A.reservation ? A.reservation[j] : CNS_RESV_NONE;
    if (A.incl_off) { ib = A.incl_off[j]; ie = A.incl_off[(u64)j + 1]; }
    if (A.excl_off) { eb = A.excl_off[j]; ee = A.excl_off[(u64)j + 1]; }
    // req_total_res_view = node * node_num + task * ntasks (:7156-7157); the walk's request = node + task (:7356)
    u64 m1, m2, tot_mem = 0;
    i64 c1, c2, tot_cpu = 0;
    bool bad = k == 0 || nt < k;
    bad |= __builtin_mul_overflow(nmem, (u64)k, &m1) | __builtin_mul_overflow(tmem, (u64)nt, &m2);
    bad |= __builtin_add_overflow(m1, m2, &tot_mem);
    bad |= __builtin_mul_overflow(ncpu, (i64)k, &c1) | __builtin_mul_overflow(tcpu, (i64)nt, &c2);
    bad |= __builtin_add_overflow(c1, c2, &tot_cpu);
    bad |= __builtin_add_overflow(nmem, tmem, &q.mem) | __builtin_add_overflow(ncpu, tcpu, &q.cpu);
    for (u32 c = 0; c < kMaxClasses; ++c) q.spec |= (u64)min((u32)((gs >> (8 * c)) & 0xFFu), 65u) << (8 * c);
    for (u32 n = 0; n < kMaxNames; ++n) q.tot |= min((gt >> (8 * n)) & 0xFFu, 65u) << (8 * n);
    if (bad) code = CNS_VALID_BAD_REQUEST;
    else if (tot_mem == 0) code = CNS_VALID_ZERO_MEM;                          // :7262
    else if (tcpu == 0) code = CNS_VALID_ZERO_CPU;                             // :7266
    else if (!found) code = CNS_VALID_PARTITION_NOT_FOUND;                     // :7278
    else {
      const VdTotal& T = A.total[ch.part];
      if (T.refused) code = CNS_VALID_REFUSED;
      else {
        // req_total <= res_total_inc_dead (:7283): PublicHeader.cpp:648-659, GresCount :57-69 with node_num copies of the node's counts
        bool ok = tot_cpu <= T.cpu && tot_mem <= T.mem;
        for (u32 n = 0; n < kMaxNames; ++n) ok &= (u64)((gt >> (8 * n)) & 0xFFu) * k <= T.name[n];
        for (u32 c = 0; c < kMaxClasses; ++c) ok &= (u64)((gs >> (8 * c)) & 0xFFu) * k <= T.cls[c];
        if (!ok) code = CNS_VALID_NO_RESOURCE;
        else if (k > T.nodes) code = CNS_VALID_NODE_NUM;                       // :7299
        else if (rsv != CNS_RESV_NONE && rsv >= A.V) code = CNS_VALID_RESV_NOT_FOUND;   // :7308
      }
    }
  }

  // the walk (:7354-7357) over the whole partition; lists are applied below
  u32 cnt = 0;
  for (u32 base = pb; base < pe; base += kVdTile) {   // (pb, pe are the same in every thread: every thread reaches both barriers)
    __syncthreads();
    if (tid < pe - base) tile[tid] = A.node[A.part_nodes[base + tid]];
    __syncthreads();
    const u32 n = min(kVdTile, pe - base);
#pragma unroll 4
    for (u32 i = 0; i < n; ++i) cnt += vd_fits(q, tile[i]) ? 1u : 0u;
  }

  if (!active) return;
  if (code == kPending) {
    if (ib < ie) {
      if (rsv != CNS_RESV_NONE) {                                              // :7338-7349
        const u32 rb = A.rv_off[rsv], re = A.rv_off[rsv + 1];
        for (u64 x = ib; x < ie && code == kPending; ++x)
          if (!sorted_contains(A.rv_nodes, rb, re, A.incl[x])) code = CNS_VALID_RESV_NODE;
      }
      // the included nodes the partition lists, that fit and are not excluded (:7356-7361)
      cnt = 0;
      if (code == kPending)
        for (u64 x = ib; x < ie; ++x) {
          const u32 n = A.incl[x];
          if (n < A.N && sorted_contains(A.part_nodes, pb, pe, n) && vd_fits(q, A.node[n]) && !sorted_contains(A.excl, eb, ee, n)) ++cnt;
        }
    } else {
      // every excluded node the partition lists and that fits was counted above (a list names a node once)
      for (u64 x = eb; x < ee; ++x) {
        const u32 n = A.excl[x];
        if (n < A.N && sorted_contains(A.part_nodes, pb, pe, n) && vd_fits(q, A.node[n])) --cnt;
      }
    }
    if (code == kPending) code = cnt < k ? CNS_VALID_NOT_ENOUGH_NODES : CNS_VALID_OK;   // :7368
  }
  A.code[j] = (uint8_t)code;
  A.eligible[j] = code == CNS_VALID_OK || code == CNS_VALID_NOT_ENOUGH_NODES ? cnt : 0u;
}

}  // namespace cns
