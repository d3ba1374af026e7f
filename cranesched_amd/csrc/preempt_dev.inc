// Preemption inside the cycle — device form of LocalScheduler::TryPreempt_ (src/CraneCtld/JobScheduler.cpp:6378-6505),
// PreemptSegTree (src/CraneCtld/JobScheduler.h:867-980) and UpdateNodeSelectorWithPreemptedJob (h:645-670).
// Included from select_kernels.hip (inside namespace cns).  Runs on the WORKER wave of k_select's general path
// (worker_job_slow, Phase B), only when the cycle was started with preemption enabled (KParams::pre.enabled): such a
// cycle never uses the fast paths, k_pipe or k_wide — a preemption RELEASES resources, and every one of them relies on
// the node state being monotone within a cycle.
//
// All 64 lanes execute the same scalar program (the data is wave-uniform); stores are lane 0's.  It is rare and
// sequential by nature: the candidates are sorted, added to the trees one by one until every node is satisfied, then
// taken away again in reverse order where the trees stay satisfied without them.
//
// The segment tree is emulated node for node, INCLUDING what a cleaner implementation would not do: a range that covers
// an inner node completely recomputes that node's `satisfied` from the node's own resource (the value it had when it
// was split plus the complete covers since), not from its children — so a running job that holds resources over the
// whole window satisfies the tree only if it alone covers the request.  The outcome depends on it, so it is kept.
// Times are quarter-nanosecond ticks relative to `now` (absl::Duration's resolution: `(ed - st) / 2` truncates there).

#ifdef CNS_PROF_PRE   // (-DCNS_PROF_PRE: TryPreempt_ by phase and by size, 32 slots per partition in KParams::prof — tools/prof_preempt.py names them)
#define PPROF_T(var) const long long var = clock64()
#define PPROF_ADD(slot, v) do { if (lane == 0) P.prof[(size_t)part * 32 + (slot)] += (u64)(v); } while (0)
#else
#define PPROF_T(var)
#define PPROF_ADD(slot, v)
#endif
constexpr i64 kPreTicks = 4000000000ll;
constexpr u32 kPrePending = 0x80000000u;
// The sizes TryPreempt_ is compiled with (cns_preempt_shape returns them; tests/preempt_seams.py puts a case on each):
constexpr u32 kPreSortLanes = 64;                        // candidates per step: of the collection, of a chunk of the rank sort, of apply()'s registers
constexpr u32 kPreSortChunks = 4;                        // chunks the register rank sort holds: more candidates are ordered block by block
constexpr u32 kPrePoolNodes = 1u << 16;                  // nodes of a partition's segment-tree pool: a call that needs more is CNS_ERR_UNSUPPORTED

#ifndef CNS_PRE_HOST   // (CNS_PRE_HOST: the two tree forms alone, compiled for the HOST by tests/host_seg — the device source itself under the CPU suite)
__device__ __forceinline__ i64 pre_ticks(i64 t, i64 now) {
  const i64 d = t - now;
  if (t == kInf || d > (INT64_MAX / 8) / kPreTicks) return INT64_MAX / 4;
  if (d < -((INT64_MAX / 8) / kPreTicks)) return -(INT64_MAX / 4);
  return d * kPreTicks;
}
// The node's first slot: the key of what is kept per NODE (one NodeState, hence one qos_job_map, per craned however many
// partitions list it: JobScheduler.cpp:6585-6615).
__device__ __forceinline__ u32 pre_prim(const KParams& P, u32 q) { return P.slot_block ? P.slot_block[q] : q; }
#endif
__device__ __forceinline__ bool pre_is_zero(const Res& r) { return r.cpu == 0 && r.mem == 0 && cores_empty(r) && r.gres == 0; }

// The tree's nodes live in a direct-mapped WRITE-BACK cache in the workgroup's LDS (slot = node index % kPreCacheN); this partition's
// pool in HBM (200 bytes per node, bump-allocated) only backs the nodes that lost their slot.  The emulation walks ~70 levels per range
// end and a visit used to be three to four dependent round trips to L2 (header, resource, tags, the store's acknowledgement in front of
// the next load: ~1 us per visit, 4.4 ms per TryPreempt_ call on C4rp: profiles/r04_preempt_phases.txt).  A node that loses its slot
// is written out with one coalesced store (50 lanes), a node that is not resident is fetched with one coalesced load.  Reads COPY what
// they need into registers and writes re-establish residency (pre_in) right in front of them: two nodes may share a slot.
constexpr u32 kPreCacheN = 512;                          // entries
constexpr u32 kPreNodeDw = (u32)(sizeof(PreNode) / 4);   // 50
constexpr u32 kPreStack = 160;                           // frames of pre_range's explicit stack (depth <= ~2 x 56 levels)
constexpr u32 kPreCacheDw = kPreCacheN * (kPreNodeDw + 1u) + kPreStack;   // dwords of LDS: the entries, the tags, the stack
enum : u32 { kPnSt = 0, kPnEd = 2, kPnLs = 4, kPnRs = 5, kPnSat = 6, kPnFl = 7 /* PreNode::pad: bit 0 add_tag != 0, bit 1 sub_tag != 0 (saves reading 28 dwords per visit) */, kPnRes = 8, kPnAdd = kPnRes + (u32)(sizeof(Res) / 4), kPnSub = kPnAdd + (u32)(sizeof(Res) / 4) };
static_assert(sizeof(PreNode) == 200 && sizeof(Res) == 56 && offsetof(PreNode, res) == 32 && offsetof(PreNode, sub_tag) == 4 * kPnSub, "PreNode as dwords");
static_assert(offsetof(Res, cpu) == 0 && offsetof(Res, mem) == 8 && offsetof(Res, clo) == 16 && offsetof(Res, chi) == 24 && offsetof(Res, gres) == 32 &&
              offsetof(Res, c2) == 40 && offsetof(Res, c3) == 48, "Res as seven 64-bit words");
#ifdef CNS_PRE_HOST
typedef u32 pre_l32;
typedef u64 pre_l64;
static u32 g_pre_cache[kPreCacheDw] __attribute__((aligned(16)));
#define PRE_FOR_LANES(l, n) for (u32 l = 0; l < (n); ++l)          // (the host build is one thread: it plays the lanes in turn)
#else
#define PRE_FOR_LANES(l, n) if (const u32 l = lane; l < (n))         // lanes 0 .. n-1 of the wave, one element each
typedef __attribute__((address_space(3))) u32 pre_l32;
// (at namespace scope: allocated in the kernels that reach pre_try — k_select's — and nowhere else)
__shared__ __attribute__((aligned(16))) u32 g_pre_cache[kPreCacheDw];
typedef __attribute__((address_space(3))) u64 pre_l64;
#endif

struct PreTree {
  PreNode* pool;     // this partition's pool (HBM)
  pre_l32* cdat;     // LDS: kPreNodeDw dwords per slot (8-byte aligned)
  pre_l32* ctag;     // LDS: node index + 1 per slot (0: empty); behind them: pre_range's stack
#ifdef CNS_PROF_PRE
  u32 n_ops, n_visits, n_miss;
#endif
  u32 cap;
  u32 used;          // bump allocator (index 0 is the first root: never a child)
  bool overflow;
};
__device__ __forceinline__ u32 pre_r32(const pre_l32* p) { return *(const volatile pre_l32*)p; }
__device__ __forceinline__ u64 pre_r64(const pre_l32* p) { return *(const volatile pre_l64*)p; }
__device__ __forceinline__ void pre_w32(pre_l32* p, u32 v) { *(volatile pre_l32*)p = v; }
__device__ __forceinline__ void pre_w64(pre_l32* p, u64 v) { *(volatile pre_l64*)p = v; }
__device__ __forceinline__ Res pre_r_res(const pre_l32* p) {
  Res r;
  r.cpu = (i64)pre_r64(p); r.mem = pre_r64(p + 2); r.clo = pre_r64(p + 4); r.chi = pre_r64(p + 6); r.gres = pre_r64(p + 8);
  r.c2 = pre_r64(p + 10); r.c3 = pre_r64(p + 12);
  return r;
}
__device__ __forceinline__ void pre_w_res(pre_l32* p, const Res& r) {   // (the caller's lane 0)
  pre_w64(p, (u64)r.cpu); pre_w64(p + 2, r.mem); pre_w64(p + 4, r.clo); pre_w64(p + 6, r.chi); pre_w64(p + 8, r.gres);
  pre_w64(p + 10, r.c2); pre_w64(p + 12, r.c3);
}
// slot of node ni, its previous occupant written back; `fetch`: with the node's dwords from the pool (else the caller writes all of them)
__device__ __forceinline__ pre_l32* pre_claim(PreTree& T, u32 ni, bool fetch, u32 lane) {
  const u32 s = ni & (kPreCacheN - 1u);
  pre_l32* const d = T.cdat + s * kPreNodeDw;
  const u32 t = uni32(pre_r32(&T.ctag[s]));
  if (t != ni + 1u) {
#ifdef CNS_PROF_PRE
    if (fetch) ++T.n_miss;
#endif
    if (fetch) drain_stores();   // (the node's own write-back, issued when it lost its slot)
    if (t != 0u) PRE_FOR_LANES(l, kPreNodeDw) ((u32*)&T.pool[t - 1u])[l] = pre_r32(d + l);
    if (fetch) PRE_FOR_LANES(l, kPreNodeDw) pre_w32(d + l, *as_global((const u32*)&T.pool[ni] + l));
    if (lane == 0) pre_w32(&T.ctag[s], ni + 1u);
  }
  return d;
}
// node ni resident: its dwords in LDS.  Valid until the next pre_in / pre_new.
__device__ __forceinline__ pre_l32* pre_in(PreTree& T, u32 ni, u32 lane) { return pre_claim(T, ni, true, lane); }

__device__ __forceinline__ u32 pre_new(PreTree& T, i64 st, i64 ed, u32 sat, const Res& res, u32 lane) {
  if (T.used >= T.cap) { T.overflow = true; return 0; }
  const u32 i = T.used++;
  pre_l32* const d = pre_claim(T, i, false, lane);
  if (lane == 0) {
    pre_w64(d + kPnSt, (u64)st); pre_w64(d + kPnEd, (u64)ed); pre_w64(d + kPnLs, 0ull); pre_w64(d + kPnSat, (u64)sat);
    pre_w_res(d + kPnRes, res); pre_w_res(d + kPnAdd, res_zero()); pre_w_res(d + kPnSub, res_zero());
  }
  return i;
}
// add_res_ / sub_res_ (h:879-889) on node ni, resident at d
__device__ __forceinline__ void pre_apply_at(pre_l32* const d, const Res& target, const Res& r, bool add, u32 lane) {
  Res v = pre_r_res(d + kPnRes);
  const u64 lr = pre_r64(d + kPnLs);
  if (add) res_add(v, r); else res_sub(v, r);
  const u32 sat = res_le(target, v) ? 1u : 0u;
  if ((u32)lr) {   // an inner node remembers it for its children
    const u32 fl = pre_r32(d + kPnFl);
    Res tag = pre_r_res(d + (add ? kPnAdd : kPnSub));
    res_add(tag, r);
    const u32 bit = add ? 1u : 2u;
    if (lane == 0) {
      pre_w_res(d + (add ? kPnAdd : kPnSub), tag);
      pre_w32(d + kPnFl, pre_is_zero(tag) ? (fl & ~bit) : (fl | bit));
    }
  }
  if (lane == 0) {
    pre_w_res(d + kPnRes, v);
    pre_w32(d + kPnSat, sat);
  }
}
__device__ __forceinline__ void pre_apply(PreTree& T, u32 ni, const Res& target, const Res& r, bool add, u32 lane) {
  pre_apply_at(pre_in(T, ni, lane), target, r, add, lane);
}
// add_ / sub_ (h:914-938) without recursion: a stack of (node, children done?) frames; depth <= ~2 x 56 levels
// (the tree's descriptor travels by value, in registers: by reference every T.cdat / T.ctag would be a load from the caller's stack)
// A visit is a chain of dependent LDS reads (~120 cycles each): the frame, the slot's tag, then the node's header in ONE batch
// (interval, children, satisfied + tag flags) — the usual revisit of an inner node without pending tags needs nothing else.
__device__ __noinline__ PreTree pre_range_v(PreTree T, u32 root, const Res target, i64 st, i64 ed, const Res r, bool add) {
  const u32 lane = threadIdx.x & 63u;
  pre_l32* const stack = T.ctag + kPreCacheN;   // (in LDS: a frame in scratch memory is a trip to the vector L1 per push and pop)
  int sp = 0;
  if (lane == 0) pre_w32(stack, root << 1);
  sp = 1;
#ifdef CNS_PROF_PRE
  ++T.n_ops;
#endif
  while (sp > 0 && !T.overflow) {
    const u32 f = uni32(pre_r32(stack + --sp));
#ifdef CNS_PROF_PRE
    ++T.n_visits;
#endif
    const u32 ni = f >> 1;
    pre_l32* d = pre_in(T, ni, lane);
    const i64 nst = (i64)pre_r64(d + kPnSt), ned = (i64)pre_r64(d + kPnEd);
    u64 lr = pre_r64(d + kPnLs);
    const u64 sf = pre_r64(d + kPnSat);   // satisfied | tag flags << 32
    if (f & 1u) {   // push_up_ (h:912)
      const u32 sl = pre_r32(pre_in(T, (u32)lr, lane) + kPnSat);
      const u32 sr = pre_r32(pre_in(T, (u32)(lr >> 32), lane) + kPnSat);
      d = pre_in(T, ni, lane);
      if (lane == 0) pre_w32(d + kPnSat, (sl && sr) ? 1u : 0u);
      continue;
    }
    if (ned <= st || ed <= nst) continue;
    if (st <= nst && ned <= ed) { pre_apply_at(d, target, r, add, lane); continue; }
    // push_down_ (h:891-910)
    if ((u32)lr == 0u) {
      const i64 mid = nst + (ned - nst) / 2;
      const Res res = pre_r_res(d + kPnRes);
      const u32 ls = pre_new(T, nst, mid, (u32)sf, res, lane);
      const u32 rs = pre_new(T, mid, ned, (u32)sf, res, lane);
      if (T.overflow) break;
      lr = ((u64)rs << 32) | ls;
      d = pre_in(T, ni, lane);
      if (lane == 0) pre_w64(d + kPnLs, lr);
    } else if ((u32)(sf >> 32) != 0u) {   // tags to hand down (else: the usual revisit)
      const u32 fl = (u32)(sf >> 32);
      const Res at = pre_r_res(d + kPnAdd);
      const Res sb = pre_r_res(d + kPnSub);   // (nothing below changes it: pre_apply touches the children's)
      if (fl & 1u) {
        pre_apply(T, (u32)lr, target, at, true, lane);
        pre_apply(T, (u32)(lr >> 32), target, at, true, lane);
        d = pre_in(T, ni, lane);
        if (lane == 0) pre_w_res(d + kPnAdd, res_zero());
      }
      if (fl & 2u) {
        pre_apply(T, (u32)lr, target, sb, false, lane);
        pre_apply(T, (u32)(lr >> 32), target, sb, false, lane);
        d = pre_in(T, ni, lane);
        if (lane == 0) pre_w_res(d + kPnSub, res_zero());
      }
      if (lane == 0) pre_w32(d + kPnFl, 0u);
    }
    if (sp + 3 > (int)kPreStack) { T.overflow = true; break; }
    if (lane == 0) {
      pre_w32(stack + sp, (ni << 1) | 1u);              // after the children: push_up_
      pre_w32(stack + sp + 1, (u32)(lr >> 32) << 1);    // rs (popped second)
      pre_w32(stack + sp + 2, (u32)lr << 1);            // ls (popped first: ls before rs, as the reference recurses)
    }
    sp += 3;
  }
  return T;
}
__device__ __forceinline__ void pre_range(PreTree& T, u32 root, const Res& target, i64 st, i64 ed, const Res& r, bool add, u32 lane) {
  T = pre_range_v(T, root, target, st, ed, r, add);
}
__device__ __forceinline__ u32 pre_sat(PreTree& T, u32 ni, u32 lane) { return pre_r32(pre_in(T, ni, lane) + kPnSat); }

// ---------------------------------------------------------------------------------------------------------------------
// The same tree in COMPRESSED form (the device's first choice; tests/seg_compact.py is its executable description, fuzzed against
// the node-for-node tree in tests/test_seg_compact.py).  The reference's tree is split down to quarter-nanosecond ticks: the walk to
// ONE range end visits ~45 levels, and on each of them one child carries the end on while the other is a leaf that an operation
// covers completely or not at all.  All nodes of such a run that carry the same set of range ends ("chain") go through the same
// operations in the same order, and so do all their sibling leaves of one side: a chain is ONE record — the head node (which alone
// can be covered completely, and alone holds tags between operations), the resource of every other chain node, one (resource,
// satisfied) pair per side for the siblings, the two children of its last node.  What the reference does that a cleaner tree would
// not is reproduced: a node covered completely takes `satisfied` from its OWN resource, children inherit flag and resource when
// their parent is split, tags go down add first, then sub, as accumulated sums.  A new range end inside a chain cuts it where
// the end leaves the others (or sits on a midpoint); no node changes state by that.  ~10 records per walk instead of ~72 nodes.
// Records live in the LDS block of the node cache; a call that needs more than fit is run again on the node-for-node tree.
constexpr u32 kPcDw = 104;
enum : u32 { kPcSt = 0, kPcEd = 2, kPcXmin = 4, kPcXmax = 6, kPcKind = 8 /* 0 leaf, 1 chain */, kPcSat = 9, kPcSl = 10, kPcSr = 11, kPcNl = 12,
              kPcNr = 13, kPcCl = 14 /* record + 1, 0: none */, kPcCr = 15, kPcRes = 16, kPcTa = 30, kPcTs = 44, kPcRc = 58, kPcRl = 72, kPcRr = 86,
              kPcBp = 100, kPcBq = 102 /* the chain's last node */ };
constexpr u32 kPcCap = (kPreCacheDw - kPreStack) / kPcDw;
struct PreC {
  pre_l32* base;     // LDS: kPcDw dwords per record
  pre_l32* stack;
  u32 used, cap;
  bool overflow;     // more records than fit: the caller falls back to the node-for-node tree
#ifdef CNS_PROF_PRE
  u32 n_ops, n_visits;
  u32 n_sec[6];          // visits by kind: push_up | outside | covered completely | leaf split | end inserted into a chain | (all partial visits)
  long long c_sec[6];    // ... and their cycles
#endif
};
__device__ __forceinline__ pre_l32* pc_at(const PreC& T, u32 i) { return T.base + i * kPcDw; }
__device__ __forceinline__ u32 pc_leaf(PreC& T, i64 st, i64 ed, const Res& res, u32 sat, u32 lane) {
  if (T.used >= T.cap) { T.overflow = true; return 0; }
  const u32 i = T.used++;
  pre_l32* const d = pc_at(T, i);
  if (lane == 0) {
    pre_w64(d + kPcSt, (u64)st); pre_w64(d + kPcEd, (u64)ed); pre_w64(d + kPcKind, (u64)sat << 32);   // kind 0 | sat
    pre_w_res(d + kPcRes, res);
  }
  return i;
}
// add_res_ / sub_res_ on a record covered completely (a leaf, or the head of a chain)
__device__ __forceinline__ void pc_apply(PreC& T, u32 i, const Res& target, const Res& r, bool add, u32 lane) {
  pre_l32* const d = pc_at(T, i);
  Res v = pre_r_res(d + kPcRes);
  const u32 kind = pre_r32(d + kPcKind);
  if (add) res_add(v, r); else res_sub(v, r);
  const u32 sat = res_le(target, v) ? 1u : 0u;
  if (kind) {
    Res tag = pre_r_res(d + (add ? kPcTa : kPcTs));
    res_add(tag, r);
    if (lane == 0) pre_w_res(d + (add ? kPcTa : kPcTs), tag);
  }
  if (lane == 0) { pre_w_res(d + kPcRes, v); pre_w32(d + kPcSat, sat); }
}
// push_up_ of a chain: every chain node = its sibling and what is below it
__device__ __forceinline__ u32 pc_and_below(const PreC& T, u32 nl, u32 sl, u32 nr, u32 sr, u32 cl, u32 cr) {
  bool ok = (nl == 0u || sl) && (nr == 0u || sr);
  if (cl) ok = ok && pre_r32(pc_at(T, cl - 1u) + kPcSat) != 0u;
  if (cr) ok = ok && pre_r32(pc_at(T, cr - 1u) + kPcSat) != 0u;
  return ok ? 1u : 0u;
}
// one level of a chain: the midpoint of [p, q) and where the ends [xmin, xmax] go on: -1 left child, +1 right child, 0 this is the last node
__device__ __forceinline__ int pc_step(i64 p, i64 q, i64 xmin, i64 xmax, i64& mid) {
  mid = p + (q - p) / 2;
  return xmax < mid ? -1 : (xmin > mid ? 1 : 0);
}
// the leaf record i = [p, q) is split for the first time, by an operation with the ends e1 / e2 (h1 / h2: there is one) strictly inside
__device__ __forceinline__ void pc_chain_of_leaf(PreC& T, u32 i, i64 p, i64 q, bool h1, i64 e1, bool h2, i64 e2, u32 lane) {
  pre_l32* const d = pc_at(T, i);
  const Res res = pre_r_res(d + kPcRes);
  const u32 sat = pre_r32(d + kPcSat);
  const i64 xmin = h1 && h2 ? (e1 < e2 ? e1 : e2) : (h1 ? e1 : e2), xmax = h1 && h2 ? (e1 < e2 ? e2 : e1) : (h1 ? e1 : e2);
  u32 nl = 0, nr = 0, cl = 0, cr = 0;
  i64 lp = p, lq = q, mid = 0;
  int side = 1;
  for (u32 guard = 0; guard < 200u; ++guard) {   // (an interval halves per level: 64 levels at most)
    side = pc_step(lp, lq, xmin, xmax, mid);
    if (side == 0) break;
    if (side < 0) { ++nr; lq = mid; } else { ++nl; lp = mid; }
  }
  if (side != 0) { T.overflow = true; return; }   // (cannot happen; the caller would redo the call node for node)
  const bool in_l = (h1 && lp < e1 && e1 < mid) || (h2 && lp < e2 && e2 < mid), in_r = (h1 && mid < e1 && e1 < lq) || (h2 && mid < e2 && e2 < lq);
  if (in_l) cl = pc_leaf(T, lp, mid, res, sat, lane) + 1u; else ++nl;     // (children inherit the parent's resource and flag)
  if (in_r) cr = pc_leaf(T, mid, lq, res, sat, lane) + 1u; else ++nr;
  if (lane == 0) {
    pre_w64(d + kPcXmin, (u64)xmin); pre_w64(d + kPcXmax, (u64)xmax);
    pre_w32(d + kPcKind, 1u); pre_w32(d + kPcSl, sat); pre_w32(d + kPcSr, sat); pre_w32(d + kPcNl, nl); pre_w32(d + kPcNr, nr);
    pre_w32(d + kPcCl, cl); pre_w32(d + kPcCr, cr);
    pre_w_res(d + kPcTa, res_zero()); pre_w_res(d + kPcTs, res_zero());
    pre_w_res(d + kPcRc, res); pre_w_res(d + kPcRl, res); pre_w_res(d + kPcRr, res);
    pre_w64(d + kPcBp, (u64)lp); pre_w64(d + kPcBq, (u64)lq);
  }
}
// a range end e strictly inside the head of chain i that may be new to it: the chain is cut where e leaves the others
__device__ __forceinline__ void pc_insert_end(PreC& T, u32 i, i64 e, u32 lane) {
  pre_l32* const d = pc_at(T, i);
  const i64 xmin = (i64)pre_r64(d + kPcXmin), xmax = (i64)pre_r64(d + kPcXmax);
  if (e == xmin || e == xmax) return;
  const u32 cnl = pre_r32(d + kPcNl), cnr = pre_r32(d + kPcNr), ccl = pre_r32(d + kPcCl), ccr = pre_r32(d + kPcCr);
  const u32 sl = pre_r32(d + kPcSl), sr = pre_r32(d + kPcSr);
  u32 nl = 0, nr = 0;
  i64 p = (i64)pre_r64(d + kPcSt), q = (i64)pre_r64(d + kPcEd), mid = 0;
  bool done = false;
  for (u32 guard = 0; guard < 200u && !done; ++guard) {
    const int side = pc_step(p, q, xmin, xmax, mid);
    done = true;
    if (side == 0) {   // e goes with the others down to the last node: into one of its children (or onto its midpoint)
      if (e < mid && ccl == 0u) {
        const u32 c = pc_leaf(T, p, mid, pre_r_res(d + kPcRl), sl, lane) + 1u;      // that child was a leaf of the left group: now on its own
        if (lane == 0) { pre_w32(d + kPcCl, c); pre_w32(d + kPcNl, cnl - 1u); }
      } else if (e > mid && ccr == 0u) {
        const u32 c = pc_leaf(T, mid, q, pre_r_res(d + kPcRr), sr, lane) + 1u;
        if (lane == 0) { pre_w32(d + kPcCr, c); pre_w32(d + kPcNr, cnr - 1u); }
      }
      break;
    }
    if (side < 0 ? e < mid : e > mid) {
      if (side > 0) { ++nl; p = mid; } else { ++nr; q = mid; }
      done = false;
      continue;
    }
    // e == mid, or e strictly inside this level's sibling: this node becomes the last one of the upper part, the rest a chain of its own
    if (T.used >= T.cap) { T.overflow = true; return; }
    const u32 lo = T.used++;
    pre_l32* const w = pc_at(T, lo);
    const Res rc = pre_r_res(d + kPcRc), rl = pre_r_res(d + kPcRl), rr = pre_r_res(d + kPcRr);
    const u32 lnl = cnl - nl - (side > 0 ? 1u : 0u), lnr = cnr - nr - (side < 0 ? 1u : 0u);
    const u32 lsat = pc_and_below(T, lnl, sl, lnr, sr, ccl, ccr);
    const u64 bp = pre_r64(d + kPcBp), bq = pre_r64(d + kPcBq);
    if (lane == 0) {
      pre_w64(w + kPcSt, (u64)(side < 0 ? p : mid)); pre_w64(w + kPcEd, (u64)(side < 0 ? mid : q));
      pre_w64(w + kPcXmin, (u64)xmin); pre_w64(w + kPcXmax, (u64)xmax);
      pre_w32(w + kPcKind, 1u); pre_w32(w + kPcSat, lsat); pre_w32(w + kPcSl, sl); pre_w32(w + kPcSr, sr);
      pre_w32(w + kPcNl, lnl); pre_w32(w + kPcNr, lnr); pre_w32(w + kPcCl, ccl); pre_w32(w + kPcCr, ccr);
      pre_w_res(w + kPcRes, rc); pre_w_res(w + kPcTa, res_zero()); pre_w_res(w + kPcTs, res_zero());
      pre_w_res(w + kPcRc, rc); pre_w_res(w + kPcRl, rl); pre_w_res(w + kPcRr, rr);
      pre_w64(w + kPcBp, bp); pre_w64(w + kPcBq, bq);
    }
    const bool sib_in = e != mid;
    u32 sib = 0;
    if (sib_in) sib = (side < 0 ? pc_leaf(T, mid, q, rr, sr, lane) : pc_leaf(T, p, mid, rl, sl, lane)) + 1u;
    if (lane == 0) {
      if (side < 0) {     // the others go left: the sibling is the right child
        pre_w32(d + kPcCl, lo + 1u); pre_w32(d + kPcCr, sib); pre_w32(d + kPcNl, nl); pre_w32(d + kPcNr, nr + (sib_in ? 0u : 1u));
      } else {
        pre_w32(d + kPcCr, lo + 1u); pre_w32(d + kPcCl, sib); pre_w32(d + kPcNl, nl + (sib_in ? 0u : 1u)); pre_w32(d + kPcNr, nr);
      }
      pre_w64(d + kPcBp, (u64)p); pre_w64(d + kPcBq, (u64)q);
    }
    break;
  }
  if (!done) { T.overflow = true; return; }   // (cannot happen: see pc_chain_of_leaf)
  if (lane == 0) { pre_w64(d + kPcXmin, (u64)(e < xmin ? e : xmin)); pre_w64(d + kPcXmax, (u64)(e > xmax ? e : xmax)); }
}
// add_ / sub_ of [a, b) on the tree whose root is record `root`
__device__ __noinline__ PreC pre_crange_v(PreC T, u32 root, const Res target, i64 a, i64 b, const Res r, bool add) {
  const u32 lane = threadIdx.x & 63u;
  int sp = 0;
  if (lane == 0) pre_w32(T.stack, root << 1);
  sp = 1;
#ifdef CNS_PROF_PRE
  ++T.n_ops;
#endif
  while (sp > 0 && !T.overflow) {
    const u32 f = uni32(pre_r32(T.stack + --sp));
#ifdef CNS_PROF_PRE
    ++T.n_visits;
#endif
    const u32 i = f >> 1;
    pre_l32* const d = pc_at(T, i);
#ifdef CNS_PROF_PRE   // (record visits by kind: tools/prof_preempt.py)
    const long long v0 = clock64();
#define PC_SEC(k) do { T.n_sec[k] += 1u; T.c_sec[k] += clock64() - v0; } while (0)
#else
#define PC_SEC(k) do {} while (0)
#endif
    if (f & 1u) {   // push_up_
      const u32 sat = pc_and_below(T, pre_r32(d + kPcNl), pre_r32(d + kPcSl), pre_r32(d + kPcNr), pre_r32(d + kPcSr), pre_r32(d + kPcCl), pre_r32(d + kPcCr));
      if (lane == 0) pre_w32(d + kPcSat, sat);
      PC_SEC(0);
      continue;
    }
    const i64 p = (i64)pre_r64(d + kPcSt), q = (i64)pre_r64(d + kPcEd);
    if (q <= a || b <= p) { PC_SEC(1); continue; }
    if (a <= p && q <= b) { pc_apply(T, i, target, r, add, lane); PC_SEC(2); continue; }
    const bool h1 = p < a && a < q, h2 = p < b && b < q;
    if (pre_r32(d + kPcKind) == 0u) { pc_chain_of_leaf(T, i, p, q, h1, a, h2, b, lane); PC_SEC(3); }
    else {
      if (h1) pc_insert_end(T, i, a, lane);
      if (h2 && !T.overflow) pc_insert_end(T, i, b, lane);
      PC_SEC(4);
    }
    if (T.overflow) break;
    // push_down_ along the chain: the head's tags reach every node below it, add first, then sub
    Res rc = pre_r_res(d + kPcRc), rl = pre_r_res(d + kPcRl), rr = pre_r_res(d + kPcRr);
    u32 sl = pre_r32(d + kPcSl), sr = pre_r32(d + kPcSr);
    const u32 cl = pre_r32(d + kPcCl), cr = pre_r32(d + kPcCr);
    const Res ta = pre_r_res(d + kPcTa), ts = pre_r_res(d + kPcTs);
    if (!pre_is_zero(ta)) {
      res_add(rc, ta); res_add(rl, ta); res_add(rr, ta);
      sl = res_le(target, rl) ? 1u : 0u; sr = res_le(target, rr) ? 1u : 0u;
      if (cl) pc_apply(T, cl - 1u, target, ta, true, lane);
      if (cr) pc_apply(T, cr - 1u, target, ta, true, lane);
      if (lane == 0) pre_w_res(d + kPcTa, res_zero());
    }
    if (!pre_is_zero(ts)) {
      res_sub(rc, ts); res_sub(rl, ts); res_sub(rr, ts);
      sl = res_le(target, rl) ? 1u : 0u; sr = res_le(target, rr) ? 1u : 0u;
      if (cl) pc_apply(T, cl - 1u, target, ts, false, lane);
      if (cr) pc_apply(T, cr - 1u, target, ts, false, lane);
      if (lane == 0) pre_w_res(d + kPcTs, res_zero());
    }
    // the operation itself: the sibling leaves of a side are covered all or none
    if (a <= p) { if (add) res_add(rl, r); else res_sub(rl, r); sl = res_le(target, rl) ? 1u : 0u; }
    if (b >= q) { if (add) res_add(rr, r); else res_sub(rr, r); sr = res_le(target, rr) ? 1u : 0u; }
    if (lane == 0) {
      pre_w_res(d + kPcRc, rc); pre_w_res(d + kPcRl, rl); pre_w_res(d + kPcRr, rr);
      pre_w32(d + kPcSl, sl); pre_w32(d + kPcSr, sr);
    }
    // ... and the children of the chain's last node, then the chain's push_up_
    if (sp + 3 > (int)kPreStack) { T.overflow = true; break; }
    if (lane == 0) pre_w32(T.stack + sp, (i << 1) | 1u);
    ++sp;
    if (cr) { if (lane == 0) pre_w32(T.stack + sp, (cr - 1u) << 1); ++sp; }
    if (cl) { if (lane == 0) pre_w32(T.stack + sp, (cl - 1u) << 1); ++sp; }
    PC_SEC(5);
  }
  return T;
}
#undef PC_SEC

#ifndef CNS_PRE_HOST
// What TryPreempt_ needs to know about a candidate
struct PreJobView { bool pending; u32 idx; u32 qprio; bool preempting; double prio; i64 start, end; };
__device__ __forceinline__ PreJobView pre_view(const KParams& P, u32 ref) {
  PreJobView v;
  v.pending = (ref & kPrePending) != 0;
  v.idx = ref & ~kPrePending;
  if (v.pending) {
    v.qprio = P.pre.pj_qprio[v.idx]; v.prio = P.pre.pj_prio[v.idx]; v.preempting = false;
    v.start = P.o_start[v.idx]; v.end = P.pre.pj_end[v.idx];
  } else {
    v.qprio = P.pre.rj_qprio[v.idx]; v.prio = 0.0; v.preempting = P.pre.rj_preempting[v.idx] != 0;
    v.start = P.pre.rj_start[v.idx]; v.end = P.pre.rj_end[v.idx];
  }
  return v;
}
// the comparator of :6401-6432, with the canonical order (ascending index) where it leaves candidates unordered
__device__ __forceinline__ bool pre_before(const PreJobView& a, const PreJobView& b) {
  if (a.preempting != b.preempting) return a.preempting;
  if (a.pending != b.pending) return a.pending;
  if (a.qprio != b.qprio) return a.qprio < b.qprio;
  if (a.pending) { if (a.prio != b.prio) return a.prio < b.prio; }
  else if (a.start != b.start) return a.start > b.start;
  return a.idx < b.idx;
}

// TryPreempt_ for job J whose res_total selection sits in H[0..k) (allocations in H[i].res, slot codes in H[i].p).
// Returns the number of preempted jobs written to chosen[] (in the reference's push_back order), or -1: no preemption.
template <u32 kS>
__device__ __noinline__ int pre_try(const KParams& P, const JobCtx& J, const HeapEnt* H, u32 qbeg, u32 part, u32* fault) {
  const u32 lane = threadIdx.x & 63u;
  const PreParams& Q = P.pre;
  drain_stores();   // (the records and list heads of the jobs committed before this one — also by the inline path — are read below)
  const u32 jq = Q.pj_qos[J.orig];
  if (jq >= Q.num_qos || Q.qp_off[jq] == Q.qp_off[jq + 1]) return -1;   // :6384-6385
  const u32 lb = Q.qp_off[jq], le = Q.qp_off[jq + 1];
  auto listed = [&](u32 qos) { for (u32 x = lb; x < le; ++x) if (Q.qp[x] == qos) return true; return false; };
  u32* const cand = Q.cand + (size_t)part * Q.cand_cap;
  u32* const chosen = Q.chosen + (size_t)part * Q.cand_cap;
  PPROF_T(p0);
  // ---- the candidates: every job of a listed qos on one of the k nodes (:6387-6397), each once -------------------------
  // Lane-parallel (round 6): the entries of a list are tested 64 at a time (gone? its job's qos listed? seen under an earlier node?)
  // and the hits appended in one pass; only the walk along rec_next itself is serial.  The order in cand[] does not matter: the
  // comparator below is a strict total order.  (Entry by entry this phase took 166 us per call on C4rp: 4 dependent loads each.)
  u32 nc = 0;
  bool full = false;
  auto put_many = [&](bool ok, u32 ref) {
    if (J.k != 1 && nc) {   // a job holds resources on several of the k nodes: listed once
      bool dup = false;
      for (u32 x = 0; x < nc; ++x) dup = dup || cand[x] == ref;
      ok = ok && !dup;
    }
    const u64 m = __ballot(ok);
    if (!m) return;
    const u32 pos = nc + (u32)__popcll(m & ((1ull << lane) - 1ull));
    if (ok) { if (pos < Q.cand_cap) cand[pos] = ref; }
    const u32 add = (u32)__popcll(m);
    if (nc + add > Q.cand_cap) { full = true; nc = Q.cand_cap; } else nc += add;
    __threadfence_block();
  };
  for (u32 i = 0; i < J.k; ++i) {
    const u32 q = qbeg + slot_of_code_t<kS>(H[i].p);
    const u32 d1 = P.rn_off[q + 1];
    for (u32 base = P.rn_off[q]; base < d1; base += 64) {
      const u32 d = base + lane;
      bool ok = d < d1 && !Q.ent_gone[d];
      u32 r = 0;
      if (ok) { r = Q.rn_job[d]; ok = listed(Q.rj_qos[r]); }
      put_many(ok, r);
    }
    u32 rec = Q.slot_head[pre_prim(P, q)];
    while (rec != kNone) {
      u32 mine = kNone;   // lane n: the n-th record from here
      for (u32 n = 0; n < 64 && rec != kNone; ++n) {
        if (lane == n) mine = rec;
        rec = Q.rec_next[rec];
      }
      bool ok = mine != kNone && !Q.rec_gone[mine];
      u32 o = 0;
      if (ok) { o = Q.rec_orig[mine]; ok = listed(Q.pj_qos[o]); }
      put_many(ok, o | kPrePending);
    }
  }
  if (full) { *fault = 31; return -1; }
  PPROF_T(p1);
  PPROF_ADD(0, 1); PPROF_ADD(1, p1 - p0); PPROF_ADD(6, nc);
  if (nc == 0) return -1;
  // ---- order (:6399-6432) --------------------------------------------------------------------------------------------
  if (nc <= kPreSortLanes * kPreSortChunks && Q.literal_tree == 0u) {   // (the debug settings CNS_PREEMPT_TREE=literal | tiny also send every call through the block-by-block form below: the tests of those settings cover it on small cases)
    // up to 256 candidates: lane l holds candidates l, l + 64, ... and counts the candidates that come before each of them (the
    // comparator is a strict total order, so the counts are the positions) — one gather of the views instead of ~nc^2 / 4
    // dependent trips to HBM
    u32 ref[kPreSortChunks], rank[kPreSortChunks];
    PreJobView v[kPreSortChunks];
#pragma unroll
    for (u32 c = 0; c < kPreSortChunks; ++c) {
      const u32 x = lane + 64u * c;
      ref[c] = x < nc ? cand[x] : 0u;
      v[c].pending = false; v[c].idx = 0; v[c].qprio = 0; v[c].preempting = false; v[c].prio = 0.0; v[c].start = 0; v[c].end = 0;
      if (x < nc) v[c] = pre_view(P, ref[c]);
      rank[c] = 0;
    }
#pragma unroll
    for (u32 cy = 0; cy < kPreSortChunks; ++cy) {
      if (64u * cy >= nc) break;
      const u32 ny = nc - 64u * cy < 64u ? nc - 64u * cy : 64u;
      for (u32 y = 0; y < ny; ++y) {
        PreJobView w;
        w.pending = rl32(v[cy].pending ? 1u : 0u, y) != 0; w.idx = rl32(v[cy].idx, y); w.qprio = rl32(v[cy].qprio, y);
        w.preempting = rl32(v[cy].preempting ? 1u : 0u, y) != 0;
        w.prio = __longlong_as_double((long long)rl64((u64)__double_as_longlong(v[cy].prio), y));
        w.start = (i64)rl64((u64)v[cy].start, y); w.end = 0;
#pragma unroll
        for (u32 c = 0; c < kPreSortChunks; ++c) rank[c] += pre_before(w, v[c]) ? 1u : 0u;
      }
    }
#pragma unroll
    for (u32 c = 0; c < kPreSortChunks; ++c)
      if (lane + 64u * c < nc) cand[rank[c]] = ref[c];
    __threadfence_block();
  } else {
    // more candidates than the registers hold at once (a job over many nodes): the same rank sort block by block — 64 candidates
    // count, against the views of 64 at a time, how many come before them; the ranks scatter into chosen[] (free until the tree phase
    // has run) and come back.  (An insertion sort with its ~n^2/4 dependent trips to HBM took 9.5 ms per such call on C4rp.)
    for (u32 mb = 0; mb < nc; mb += 64) {
      const u32 xm = mb + lane;
      const u32 refm = xm < nc ? cand[xm] : 0u;
      PreJobView vm;
      vm.pending = false; vm.idx = 0; vm.qprio = 0; vm.preempting = false; vm.prio = 0.0; vm.start = 0; vm.end = 0;
      if (xm < nc) vm = pre_view(P, refm);
      u32 rank = 0;
      for (u32 wb = 0; wb < nc; wb += 64) {
        const u32 xw = wb + lane;
        PreJobView vw;
        vw.pending = false; vw.idx = 0; vw.qprio = 0; vw.preempting = false; vw.prio = 0.0; vw.start = 0; vw.end = 0;
        if (xw < nc) vw = pre_view(P, cand[xw]);
        const u32 ny = nc - wb < 64u ? nc - wb : 64u;
        for (u32 y = 0; y < ny; ++y) {
          PreJobView w;
          w.pending = rl32(vw.pending ? 1u : 0u, y) != 0; w.idx = rl32(vw.idx, y); w.qprio = rl32(vw.qprio, y);
          w.preempting = rl32(vw.preempting ? 1u : 0u, y) != 0;
          w.prio = __longlong_as_double((long long)rl64((u64)__double_as_longlong(vw.prio), y));
          w.start = (i64)rl64((u64)vw.start, y); w.end = 0;
          rank += pre_before(w, vm) ? 1u : 0u;
        }
      }
      if (xm < nc) chosen[rank] = refm;
    }
    __threadfence_block();
    for (u32 x = lane; x < nc; x += 64) cand[x] = chosen[x];
    __threadfence_block();
  }
  // ---- one tree per node over [now, now + time_limit) holding the node's time map (:6434-6461) --------------------------
  PPROF_T(p2);
  PPROF_ADD(2, p2 - p1); PPROF_ADD(11, 1);
  if (nc > 64u * kPreSortChunks) { PPROF_ADD(19, 1); PPROF_ADD(20, p2 - p1); }   // calls past the rank sort's capacity | their ordering time
  if (nc > 64u) { PPROF_ADD(21, 1); PPROF_ADD(22, p2 - p1); }
  const i64 seg_end = pre_ticks(P.now + J.L, P.now);
  // What the tree phase needs of the first 64 candidates (in their order), gathered by lane x for candidate x in one round of loads
  // (round 6): its interval, and — when it holds resources on exactly one node, the common case — that allocation and the tree it
  // goes into.  apply() then takes a candidate from the registers instead of five dependent trips to HBM (7 us per candidate).
  u32 pl_n = 0, pl_tree = kNone;
  i64 pl_st = 0, pl_ed = 0;
  Res pl_res = res_zero();
  if (lane < nc) {
    const PreJobView v = pre_view(P, cand[lane]);
    pl_st = pre_ticks(v.start, P.now); pl_ed = pre_ticks(v.end, P.now);
    u32 q1 = kNone;
    if (v.pending) {
      pl_n = Q.pj_k[v.idx];
      if (pl_n == 1u) {
        const u32 rec = Q.pj_rec0[v.idx];
        q1 = Q.rec_slot[rec];
        pl_res.cpu = P.o_cpu[rec]; pl_res.mem = P.o_mem[rec]; pl_res.clo = P.o_clo[rec]; pl_res.chi = P.o_chi[rec]; pl_res.gres = P.o_gres[rec];
        pl_res.c2 = P.o_c2 ? P.o_c2[rec] : 0; pl_res.c3 = P.o_c2 ? P.o_c3[rec] : 0;
      }
    } else {
      const u32 x0 = Q.rj_off[v.idx];
      pl_n = Q.rj_off[v.idx + 1] - x0;
      if (pl_n == 1u) {
        const u32 d = Q.rj_ent[x0];
        q1 = Q.ent_slot[d];
        if (pre_prim(P, q1) != q1) q1 = kNone;   // (an allocation is listed under every slot of its node: once — as the walk below skips it)
        else pl_res = P.rn_res[d];
      }
    }
    if (q1 != kNone) {
      const u32 pq = pre_prim(P, q1);
      for (u32 i = 0; i < J.k; ++i)
        if (pre_prim(P, qbeg + slot_of_code_t<kS>(H[i].p)) == pq) { pl_tree = i; break; }
    }
  }
  // The tree phase, first on the compressed trees (records in LDS), and — should a call need more records than fit — again from the
  // start on the node-for-node trees (LDS cache over the HBM pool).  Both give the reference's answers (tests/test_seg_compact.py).
  // -> number of chosen jobs, -1: no preemption, -2: the compressed form ran out of records
  auto tree_phase = [&](const bool compact) -> int {
    PreTree T;
    T.pool = (PreNode*)Q.pool + (size_t)part * Q.pool_nodes;
    T.cap = Q.pool_nodes; T.used = 0; T.overflow = false;
    T.cdat = (pre_l32*)g_pre_cache; T.ctag = T.cdat + kPreCacheN * kPreNodeDw;
    PreC C;
    C.base = (pre_l32*)g_pre_cache; C.stack = C.base + kPcCap * kPcDw; C.used = 0; C.overflow = false;
    C.cap = Q.literal_tree == 2u ? (J.k + 5u < kPcCap ? J.k + 5u : kPcCap) : kPcCap;   // (CNS_PREEMPT_TREE=tiny: room for a handful of records, so that calls DO run out)
#ifdef CNS_PROF_PRE
    T.n_ops = 0; T.n_visits = 0; T.n_miss = 0; C.n_ops = 0; C.n_visits = 0;
    for (u32 k = 0; k < 6u; ++k) { C.n_sec[k] = 0; C.c_sec[k] = 0; }
#endif
    if (compact) {
      for (u32 i = 0; i < J.k; ++i) pc_leaf(C, 0, seg_end, res_zero(), 0u, lane);      // the roots are records 0 .. k-1
    } else {
      for (u32 x = lane; x < kPreCacheN; x += 64) pre_w32(&T.ctag[x], 0u);
      for (u32 i = 0; i < J.k; ++i) pre_new(T, 0, seg_end, 0u, res_zero(), lane);      // the roots are nodes 0 .. k-1 of the pool
    }
    auto range = [&](u32 i, const Res& target, i64 st, i64 ed, const Res& r, bool add) {
      if (compact) {
        PPROF_T(rc1);
        if (st < ed) C = pre_crange_v(C, i, target, st, ed, r, add); else C.overflow = true;   // (an empty range: never produced; the literal walk defines it)
        PPROF_T(rc2);
        PPROF_ADD(30, rc2 - rc1);
      }
      else pre_range(T, i, target, st, ed, r, add, lane);
    };
    auto failed = [&]() { return compact ? C.overflow : T.overflow; };
    for (u32 i = 0; i < J.k && !failed(); ++i) {
      const u32 q = qbeg + slot_of_code_t<kS>(H[i].p);
      NodeHdr* hd = hdr_of(P, q);
      const TlMap M = tl_of(P, hd);
      const u32 len = hd->len;
      const Res target = H[i].res;
      for (u32 e = 0; e < len && !failed(); ++e) {
        const i64 st = pre_ticks(M[e].t(), P.now);
        const i64 ed = e + 1 < len ? pre_ticks(M[e + 1].t(), P.now) : seg_end;
        range(i, target, st, ed, M[e].r(), true);
        if (ed >= seg_end) break;
      }
    }
    // one candidate into / out of the trees of the nodes it holds resources on (:6463-6477)
    auto apply = [&](u32 x, bool add) {
      if (x < 64u && rl32(pl_n, x) == 1u) {   // from the registers of lane x
        const u32 ti = rl32(pl_tree, x);
        if (ti != kNone) range(ti, H[ti].res, (i64)rl64((u64)pl_st, x), (i64)rl64((u64)pl_ed, x), rl_res(pl_res, x), add);
        return;
      }
      const u32 ref = cand[x];
      const PreJobView v = pre_view(P, ref);
      const i64 st = pre_ticks(v.start, P.now), ed = pre_ticks(v.end, P.now);
      auto on_slot = [&](u32 q, const Res& r) {   // (by node: q may be the node's slot in another partition of the group)
        const u32 pq = pre_prim(P, q);
        for (u32 i = 0; i < J.k; ++i)
          if (pre_prim(P, qbeg + slot_of_code_t<kS>(H[i].p)) == pq) { range(i, H[i].res, st, ed, r, add); return; }
      };
      if (v.pending) {
        const u32 r0 = Q.pj_rec0[v.idx], kk = Q.pj_k[v.idx];
        for (u32 rec = r0; rec < r0 + kk; ++rec) {
          Res r; r.cpu = P.o_cpu[rec]; r.mem = P.o_mem[rec]; r.clo = P.o_clo[rec]; r.chi = P.o_chi[rec]; r.gres = P.o_gres[rec];
          r.c2 = P.o_c2 ? P.o_c2[rec] : 0; r.c3 = P.o_c2 ? P.o_c3[rec] : 0;
          on_slot(Q.rec_slot[rec], r);
        }
      } else {
        for (u32 x = Q.rj_off[v.idx]; x < Q.rj_off[v.idx + 1]; ++x) {
          const u32 d = Q.rj_ent[x];
          if (pre_prim(P, Q.ent_slot[d]) != Q.ent_slot[d]) continue;   // an allocation is listed under every slot of its node: once
          on_slot(Q.ent_slot[d], P.rn_res[d]);
        }
      }
    };
    auto all_satisfied = [&]() {
      for (u32 i = 0; i < J.k; ++i)
        if (!(compact ? pre_r32(pc_at(C, i) + kPcSat) : pre_sat(T, i, lane))) return false;
      return true;
    };
#ifdef CNS_PROF_PRE
    auto counters = [&]() { if (compact) for (u32 k = 0; k < 6u; ++k) { PPROF_ADD(23 + k, C.n_sec[k] | ((u64)C.c_sec[k] << 24)); } PPROF_ADD(7, compact ? C.n_ops : T.n_ops); PPROF_ADD(8, compact ? C.n_visits : T.n_visits); PPROF_ADD(9, compact ? C.used : T.used); PPROF_ADD(17, T.n_miss); };
#else
    auto counters = [&]() {};
#endif
    PPROF_T(p3);
    PPROF_ADD(3, p3 - p2); PPROF_ADD(12, compact ? C.n_ops : T.n_ops); PPROF_ADD(13, compact ? C.n_visits : T.n_visits); PPROF_ADD(14, compact ? C.used : T.used);
    int preempt_idx = -1;
    for (u32 x = 0; x < nc && !failed() && !all_satisfied(); ++x) {   // :6484-6488
      PPROF_T(ap0);
      apply(x, true);
      PPROF_T(ap1);
      PPROF_ADD(31, ap1 - ap0);
      preempt_idx = (int)x;
    }
    if (failed()) { counters(); return compact ? -2 : -3; }
    PPROF_T(p4);
    PPROF_ADD(4, p4 - p3); PPROF_ADD(15, preempt_idx + 1);
    if (!all_satisfied()) { counters(); return -1; }
    u32 nch = 0;
    if (preempt_idx >= 0) { if (lane == 0) chosen[nch] = cand[preempt_idx]; ++nch; }   // :6490
    for (int x = preempt_idx - 1; x >= 0 && !failed(); --x) {        // :6491-6497
      apply((u32)x, false);
      if (failed()) break;
      if (!all_satisfied()) {
        apply((u32)x, true);
        if (lane == 0) chosen[nch] = cand[x];
        ++nch;
      }
    }
    if (failed()) { counters(); return compact ? -2 : -3; }
    PPROF_T(p5);
    PPROF_ADD(5, p5 - p4); counters(); PPROF_ADD(10, 1); PPROF_ADD(16, nch);
    return (int)nch;
  };
  int nch = Q.literal_tree == 1u ? -2 : tree_phase(true);
  if (nch == -2) { if (Q.literal_tree != 1u) PPROF_ADD(18, 1); nch = tree_phase(false); }   // (the compressed form ran out of records: once more, node for node)
  if (nch == -3) { *fault = 32; return -1; }
  if (nch < 0) return -1;
  __threadfence_block();
  return (int)nch;
}

// UpdateNodeSelectorWithPreemptedJob (h:645-670) for the `nch` jobs in chosen[]: release their resources on the nodes of
// this partition, take them out of the nodes' job lists, mark / report them.  Every touched slot is appended to
// touched[] (for the scanners' refresh).  Returns the number of touched slots.
__device__ __noinline__ u32 pre_release(const KParams& P, const JobCtx& J, u32 qbeg, u32 nn, u32 part, u32 nch, u32* touched) {
  const u32 lane = threadIdx.x & 63u;
  const PreParams& Q = P.pre;
  const u32* const chosen = Q.chosen + (size_t)part * Q.cand_cap;
  u32 nt = 0;
  // ReleaseResourceIfPresent (h:577-587) acts on the nodes of THIS scheduler: the slot the node has in the job's own
  // partition (kNone: the node is not in it).  Without shared nodes that is the slot itself, if it lies in this partition.
  const u32 jt = (J.flags >> 8) & 0xFFu;
  auto own_slot = [&](u32 q) -> u32 {
    if (q < qbeg || q >= qbeg + nn) return kNone;
    if (!P.slot_tag || P.slot_tag[q] == jt) return q;
    for (u32 a = P.sib_off[q]; a < P.sib_off[q + 1]; ++a) if (P.slot_tag[P.sib[a]] == jt) return P.sib[a];
    return kNone;
  };
  auto release_on = [&](u32 q, i64 st, i64 en, const Res& r) {
    NodeHdr* hd = hdr_of(P, q);
    const Res tot = hd->total;
    tl_commit<true>(P, hd, st, en, r, lane, J.orig);
    const double ratio = ((double)r.cpu / 256.0) / ((double)tot.cpu / 256.0);
    const double delta = (double)(en - st) * ratio;
    const Res e0 = tl_of(P, hd)[0].r();
    bool seen = false;
    for (u32 y = 0; y < nt; ++y) seen = seen || touched[y] == q;
    if (lane == 0) {
      P.cost[q] = P.cost[q] - delta;                                   // UpdateCost(..., is_release), h:49-52
      P.f_cpu[q] = clamp_cpu(e0.cpu); P.f_mem[q] = mem_mib_ceil(e0.mem); P.f_cnt[q] = class_counts(e0.gres, P.gres);
      if (P.sib_off)   // the node's slots in the other partitions of the group: same time map, own cost
        for (u32 a = P.sib_off[q]; a < P.sib_off[q + 1]; ++a) {
          const u32 qs = P.sib[a];
          P.f_cpu[qs] = P.f_cpu[q]; P.f_mem[qs] = P.f_mem[q]; P.f_cnt[qs] = P.f_cnt[q];
        }
      if (!seen) touched[nt] = q;
    }
    if (!seen) ++nt;
    drain_stores();
    __threadfence_block();
  };
  for (u32 c = 0; c < nch; ++c) {
    const u32 ref = chosen[c];
    const u32 idx = ref & ~kPrePending;
    if (ref & kPrePending) {
      const u32 r0 = Q.pj_rec0[idx], kk = Q.pj_k[idx];
      const i64 st = P.o_start[idx], en = Q.pj_end[idx];
      const bool scheduled = P.o_reason[idx] == 0;                     // is_scheduled() at this moment (h:662)
      for (u32 rec = r0; rec < r0 + kk; ++rec) {
        const u32 q = own_slot(Q.rec_slot[rec]);
        if (q == kNone) continue;
        Res r; r.cpu = P.o_cpu[rec]; r.mem = P.o_mem[rec]; r.clo = P.o_clo[rec]; r.chi = P.o_chi[rec]; r.gres = P.o_gres[rec];
        r.c2 = P.o_c2 ? P.o_c2[rec] : 0; r.c3 = P.o_c2 ? P.o_c3[rec] : 0;
        release_on(q, st, en, r);
        if (scheduled && lane == 0) Q.rec_gone[rec] = 1;
      }
      if (lane == 0) P.o_reason[idx] = CNS_REASON_PREEMPTED;           // cpp:6783
    } else {
      const i64 en = Q.rj_end[idx];
      for (u32 x = Q.rj_off[idx]; x < Q.rj_off[idx + 1]; ++x) {
        const u32 d = Q.rj_ent[x];
        const u32 qe = Q.ent_slot[d];
        if (pre_prim(P, qe) != qe) { if (lane == 0 && own_slot(qe) != kNone) Q.ent_gone[d] = 1; continue; }   // (listed under every slot of its node)
        const u32 q = own_slot(qe);
        if (q == kNone) continue;
        release_on(q, P.now, en, P.rn_res[d]);                         // h:651
        if (lane == 0) Q.ent_gone[d] = 1;
      }
    }
    if (lane == 0) {                                                   // job->preempted_jobs, in push_back order
      const u32 at = atomicAdd(Q.out_cnt, 1u);
      if (at < Q.out_cap) { Q.out[2 * at] = J.orig; Q.out[2 * at + 1] = ref; }
    }
  }
  __threadfence();
  return nt;
}
#endif   // CNS_PRE_HOST
